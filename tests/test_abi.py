"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol include/lvba_hip.h
declares, and refuses to compute without a HIP device (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, make_problem


@pytest.fixture(scope="module")
def lib(pkg):
    import __graft_entry__ as ge
    ge.build()
    return pkg._lib.load()


def test_header_symbols_are_exported(lib, pkg):
    hdr = open(os.path.join(ROOT, "include", "lvba_hip.h")).read()
    declared = set(re.findall(r"\b(lvba_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(pkg._lib.SYMBOLS), declared ^ set(pkg._lib.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.lvba_version() >= 100


def test_struct_layouts_match_header(pkg):
    L = pkg._lib
    assert ctypes.sizeof(L.BalmOpts) == 32 and ctypes.sizeof(L.LmTrace) == 64
    assert ctypes.sizeof(L.BalmInfo) == 136 and ctypes.sizeof(L.Prof) == 80 and ctypes.sizeof(L.NdModel) == 40
    assert ctypes.sizeof(L.PairLayout) == 56          # a struct of its own: lvba_balm_info_t did not grow
    o = pkg.BalmProblem.default_opts()
    assert (o.max_iter, o.u0, o.v0, o.rel_tol) == (10, 0.01, 2.0, 1e-6)      # bavoxel.hpp:664,686,760


def header_structs():
    """[(C type name, [(base type, field name, array dimensions)])] of every struct typedef of include/lvba_hip.h, in declaration order"""
    hdr = open(os.path.join(ROOT, "include", "lvba_hip.h")).read()
    out = []
    for body, name in re.findall(r"typedef struct\s*\w*\s*\{(.*?)\}\s*(\w+);", hdr, re.S):
        body = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, declarators = decl.split(None, 1)
            for d in declarators.split(","):
                m = re.fullmatch(r"\s*(\w+)((?:\[\d+\])*)\s*", d)
                assert m, (name, decl)
                fields.append((base, m.group(1), [int(n) for n in re.findall(r"\d+", m.group(2))]))
        out.append((name, fields))
    return out


# sizeof, and the offsetof of the fields a stage's test used to pin by number: they guard against header and mirror drifting together
PINNED_SIZES = {
    "lvba_balm_opts": 32, "lvba_lm_trace": 64, "lvba_balm_info_t": 136, "lvba_prof_t": 80, "lvba_nd_model_t": 40,
    "lvba_pair_layout_t": 56, "lvba_eval_layout_t": 72, "lvba_loss": 16, "lvba_loop_opts": 24, "lvba_loop_candidate": 24,
    "lvba_place_opts": 64, "lvba_place_candidate": 32, "lvba_register_opts": 64, "lvba_register_result": 56,
    "lvba_closure_opts": 40, "lvba_posegraph_opts": 64, "lvba_posegraph_report": 56, "lvba_covis_opts": 56,
    "lvba_dynamic_opts": 80, "lvba_dynamic_summary": 56, "lvba_mapq_opts": 16, "lvba_mapq_summary": 80, "lvba_sift_opts": 56,
    "lvba_trackgraph_info": 64,
}
PINNED_OFFSETS = {
    ("lvba_loss", "scale"): 8, ("lvba_closure_opts", "trans_tol"): 16, ("lvba_closure_opts", "n_seeds"): 32,
    ("lvba_closure_opts", "min_set"): 36, ("lvba_posegraph_opts", "rel_tol"): 40, ("lvba_posegraph_opts", "closure_loss"): 48,
    ("lvba_posegraph_report", "solver_kind"): 12, ("lvba_posegraph_report", "max_step_last"): 48,
}


def test_every_struct_matches_the_header_field_for_field(pkg, tmp_path):
    """Every struct typedef of the header has a mirror in _lib.STRUCTS and the reverse; for each, from the header compiled as C99
    (it must stay plain C): sizeof, the names of the fields in declaration order, and every field's offsetof, sizeof and type."""
    import subprocess
    L = pkg._lib
    structs = header_structs()
    assert [n for n, _ in structs if n not in L.STRUCTS] == [] and set(L.STRUCTS) == {n for n, _ in structs}
    rows = "".join(f'printf("%zu", sizeof({n}));' +
                   "".join(f'printf(" %zu %zu", offsetof({n}, {f}), sizeof((({n} *)0)->{f}));' for _, f, _ in fields) + 'printf("\\n");'
                   for n, fields in structs)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lvba_hip.h"\nint main(void){' + rows + "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    scalars = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double,
               "float": ctypes.c_float}
    n_fields, sizes, offsets = 0, {}, {}
    for (name, fields), line in zip(structs, subprocess.check_output([exe]).decode().splitlines()):
        cls, got = L.STRUCTS[name], [int(v) for v in line.split()]
        assert ctypes.sizeof(cls) == got[0], (name, ctypes.sizeof(cls), got[0])
        assert [f for f, _ in cls._fields_] == [f for _, f, _ in fields], name
        for k, ((f, ctype), (base, _, dims)) in enumerate(zip(cls._fields_, fields)):
            want = scalars.get(base) or L.STRUCTS[base]
            for d in reversed(dims):
                want = want * d
            assert ctype == want, (name, f, ctype, want)            # ctypes caches array types: equal means the same type
            assert (getattr(cls, f).offset, getattr(cls, f).size) == (got[1 + 2 * k], got[2 + 2 * k]), (name, f)
            offsets[name, f] = got[1 + 2 * k]
        sizes[name] = got[0]
        n_fields += len(fields)
    print(f"{len(structs)} structs, {n_fields} fields, no mismatch")
    assert {n: sizes[n] for n in PINNED_SIZES} == PINNED_SIZES
    assert {k: offsets[k] for k in PINNED_OFFSETS} == PINNED_OFFSETS


def test_pair_layout_entry_points(lib, pkg):
    """lvba_balm_pair_layout / lvba_visual_pair_layout: exported, declared in the header with one signature, mirrored by the package,
    and they refuse NULL arguments before anything touches a device."""
    hdr = open(os.path.join(ROOT, "include", "lvba_hip.h")).read()
    for name, handle in (("lvba_balm_pair_layout", "lvba_balm_t"), ("lvba_visual_pair_layout", "lvba_visual_t")):
        assert name in pkg._lib.SYMBOLS and hasattr(lib, name)
        assert re.search(name + r"\(" + handle + r" h, lvba_pair_layout_t \*out, int64_t \*item_len, int64_t \*item_slot, int64_t cap\);", hdr)
        out = pkg._lib.PairLayout()
        assert getattr(lib, name)(None, ctypes.byref(out), None, None, 0) == pkg._lib.ERR_ARG
    assert [f for f, _ in pkg._lib.PairLayout._fields_] == ["form", "cut", "n_items", "n_multi", "n_partial", "window_voxels",
                                                            "longest_item", "longest_multi"]
    assert hasattr(pkg.BalmProblem, "pair_layout") and hasattr(pkg.VisualProblem, "pair_layout")


def test_eval_layout_entry_points(lib, pkg):
    """lvba_balm_eval_layout / lvba_visual_eval_layout: exported, declared with one signature, mirrored field for field by the
    package, and they refuse NULL arguments before anything touches a device."""
    hdr = open(os.path.join(ROOT, "include", "lvba_hip.h")).read()
    for name, handle in (("lvba_balm_eval_layout", "lvba_balm_t"), ("lvba_visual_eval_layout", "lvba_visual_t")):
        assert name in pkg._lib.SYMBOLS and hasattr(lib, name)
        assert re.search(name + r"\(" + handle + r" h, lvba_eval_layout_t \*out\);", hdr)
        out = pkg._lib.EvalLayout()
        assert getattr(lib, name)(None, ctypes.byref(out)) == pkg._lib.ERR_ARG
    struct = re.search(r"typedef struct \{([^}]*)\} lvba_eval_layout_t;", hdr).group(1)
    declared = re.findall(r"^\s*int(?:32|64)_t (\w+);", struct, re.M)
    assert [f for f, _ in pkg._lib.EvalLayout._fields_] == declared == [
        "slices", "unit_form", "units", "unit_grid", "point_groups", "back_groups", "point_grid", "back_grid", "n_groups",
        "n_factors", "n_chunks"]
    assert ctypes.sizeof(pkg._lib.EvalLayout) == 72
    assert hasattr(pkg.BalmProblem, "eval_layout") and hasattr(pkg.VisualProblem, "eval_layout")


def test_shard_range_matches_reference_slicing(pkg):
    from oracle import balm_oracle as bo
    for V in (7, 16, 100, 12345, 2_000_000):
        ref = bo.thread_slices(V) if V >= 16 else None
        got = [pkg.shard_range(V, r, 16) for r in range(16)]
        assert got[0][0] == 0 and got[-1][1] == V and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        if ref:
            assert got == ref                                               # bavoxel.hpp:621-624


def test_no_cpu_fallback(lib, pkg):
    if lib.lvba_device_count() > 0:
        pytest.skip("a HIP device is present")
    d = make_problem(12, 60, band=4, seed=1)
    with pytest.raises(pkg._lib.LvbaError) as e:
        pkg.BalmProblem(d["n_poses"], d["voxel_off"], d["pose_idx"], d["clusters"])
    assert e.value.code == pkg._lib.ERR_DEVICE and "no CPU fallback" in str(e.value)


def test_product_does_not_import_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/."""
    pk = os.path.join(ROOT, "global-lvba_amd")
    for dirpath, _, files in os.walk(pk):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                for pat in (r"^\s*(import|from)\s+oracle", r"libbalm_oracle", r"balm_oracle", r"oracle/", r"import_module\([\"']oracle"):
                    assert not re.search(pat, src, re.M), (os.path.join(dirpath, f), pat)


def test_vox_hess_mirror_packs_like_the_reference(pkg):
    N = 5
    vh = pkg.VOX_HESS(N)
    sig = np.zeros((N, 10)); sig[1, 9] = 20; sig[3, 9] = 15; sig[1, :9] = 1.0; sig[3, :9] = 2.0
    vh.push_voxel(sig)
    one = np.zeros((N, 10)); one[2, 9] = 30
    vh.push_voxel(one)                                   # only one observer: dropped (bavoxel.hpp:52)
    off, idx, clu = vh.pack()
    assert off.tolist() == [0, 2] and idx.tolist() == [1, 3] and clu.shape == (2, 10) and clu[1, 9] == 15


def test_cpp_adapter_compiles_and_links(lib, tmp_path):
    """include/lvba_adapter.hpp (the reference-side binding of INTEGRATION.md) against stand-in types."""
    import subprocess
    exe = str(tmp_path / "adapter_check")
    libdir = os.path.join(ROOT, "global-lvba_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "adapter_check.cpp"), "-o", exe,
                           "-L", libdir, "-llvba_hip", f"-Wl,-rpath,{libdir}"])
    assert subprocess.call([exe]) == 0


def test_window_split_deals_out_whole_windows():
    """lvba_window_split (host only, no device needed): contiguous runs of whole windows, every frame in exactly one share,
    the thread split of bavoxel.hpp:621-624 applied to windows; shares may be empty when there are fewer windows than shares."""
    import ctypes as C
    import importlib
    L = importlib.import_module("global-lvba_amd._lib")
    lib = L.load()
    for n, w, k in ((320, 20, 8), (26, 4, 3), (26, 4, 2), (5, 10, 4), (0, 10, 2), (64, 16, 1), (1000, 7, 8)):
        fb = np.zeros(k + 1, np.int32)
        assert lib.lvba_window_split(n, w, k, fb) == 0
        assert fb[0] == 0 and fb[-1] == n and (np.diff(fb) >= 0).all()
        assert all(int(b) % w == 0 for b in fb[:-1])
        nw = (n + w - 1) // w
        per = [(-(-int(fb[i + 1] - fb[i]) // w)) for i in range(k)]
        assert sum(per) == nw and max(per) - min(per) <= 1
    assert lib.lvba_window_split(10, 0, 2, np.zeros(3, np.int32)) != 0
