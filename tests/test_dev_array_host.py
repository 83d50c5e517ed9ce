"""CPU test of the typed device array (csrc/mempool.h DevArr<T>, compiled for the host): tests/dev_array_check.cpp holds the byte
counts and the element types as static assertions, so building it is most of the test; no HIP call is made."""
import ctypes
import os

from host_build import build_check

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_dev_array_byte_counts_and_element_types(tmp_path):
    lib = ctypes.CDLL(build_check("dev_array_check", tmp_path, extra=("-I" + os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__")))
    lib.dev_array_bytes_for.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.dev_array_bytes_for.restype = ctypes.c_ulonglong
    for kind, size in enumerate((1, 8, 16, 32)):        # uint8_t, double, float4, a 32-byte struct
        assert lib.dev_array_bytes_for(kind, 0) == 8
        for n in (1, 7, 1000, (1 << 29) + 3, (1 << 33) + 1):
            assert lib.dev_array_bytes_for(kind, n) == n * size, (kind, n)
