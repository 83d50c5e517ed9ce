"""CPU tests of the map-quality metrics (lvba_mapq_*): the device header (csrc/map_quality_device.h) compiled for the host
against the brute-force restatement (tests/mapq_oracle.py), the lattice against its closed form, the struct layouts, and the
restatement's own sanity: a map at the true poses is sharper than at the noisy ones."""
import ctypes

import numpy as np
import pytest

from host_build import build_check

import mapq_oracle as mo


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = ctypes.CDLL(build_check("mapq_check", tmp_path_factory.mktemp("emul_mapq")))
    f64 = np.ctypeslib.ndpointer(np.float64, flags="C")
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    i64 = np.ctypeslib.ndpointer(np.int64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    u8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
    lib.emul_cell_edge.restype = ctypes.c_double
    lib.emul_cell_edge.argtypes = [ctypes.c_double]
    lib.emul_cells.argtypes = [ctypes.c_int64, f32, ctypes.c_double, i64, u8]
    lib.emul_pack.restype = ctypes.c_uint64
    lib.emul_pack.argtypes = [ctypes.c_int64] * 3
    lib.emul_metrics.argtypes = [ctypes.c_int64, f32, ctypes.c_double, ctypes.c_int, ctypes.c_int64, i32, u8, f64, f64, f32]
    return lib


def host_metrics(emul, xyz, radius, min_neighbors, stride=1):
    xyz = np.ascontiguousarray(xyz, np.float32)
    nq = -(-len(xyz) // stride)
    out = dict(count=np.zeros(nq, np.int32), valid=np.zeros(nq, np.uint8), entropy=np.zeros(nq), plane_var=np.zeros(nq),
               normal=np.zeros((nq, 3), np.float32))
    emul.emul_metrics(len(xyz), xyz, radius, min_neighbors, stride, out["count"], out["valid"], out["entropy"], out["plane_var"],
                      out["normal"])
    return out


def test_cell_index_floors_and_keeps_neighbours_within_one_cell(emul):
    r = 0.25
    edge = emul.emul_cell_edge(r)
    assert r < edge <= r * (1 + 2.0 ** -19)                               # strictly larger than the radius
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(-40, 40, (20000, 3)), np.round(rng.uniform(-40, 40, (20000, 3)) / r) * r])  # on cell faces too
    x = np.concatenate([x, [[-1e-30, 0.0, -0.0], [np.nan, 0, 0], [0, np.inf, 0], [3.0e5, 0, 0], [0, 0, -3.0e5]]]).astype(np.float32)
    cells, ok = np.zeros((len(x), 3), np.int64), np.zeros(len(x), np.uint8)
    emul.emul_cells(len(x), x, r, cells, ok)
    assert ok[:-4].all() and list(ok[-4:]) == [0, 0, 2, 2]               # 3e5 m / 0.25 m > 2^20 - 1 cells
    want = np.floor(x[:-4].astype(np.float64) / edge).astype(np.int64)    # floor, not truncation
    assert np.array_equal(cells[:-4], want) and (cells[:-4] < 0).any()
    assert list(cells[-5]) == [-1, 0, 0]
    # points one radius apart (exactly, on a lattice of cell faces, near and far from the origin) never land two cells apart
    for off in (0.0, 1000.25, -517.5, 2.0e4):
        g = (off + np.arange(-200, 200) * r).astype(np.float32)
        assert np.all(np.diff(g.astype(np.float64)) == r)
        p = np.stack([g, g, g], 1)
        c, o = np.zeros((len(p), 3), np.int64), np.zeros(len(p), np.uint8)
        emul.emul_cells(len(p), np.ascontiguousarray(p), r, c, o)
        assert o.all() and np.diff(c[:, 0]).max() <= 1 and np.diff(c[:, 0]).min() >= 0
    # the packing orders lexicographically by (x, y, z): (x, y, z-1 .. z+1) is one contiguous key range
    assert emul.emul_pack(-3, 5, 7) + 1 == emul.emul_pack(-3, 5, 8) and emul.emul_pack(-3, 5, 2 ** 20 - 1) < emul.emul_pack(-3, 6, -2 ** 20)
    assert emul.emul_pack(-3, 2 ** 20 - 1, 0) < emul.emul_pack(-2, -2 ** 20, 0)


def test_host_chain_matches_oracle_on_random_neighbourhoods(emul):
    """Random clouds of every shape the finish has to take: planar with noise, volumetric, line-like and sparse (too few
    neighbours)."""
    rng = np.random.default_rng(12)
    plane = np.c_[rng.uniform(-1, 1, (700, 2)), 0.01 * rng.standard_normal(700)]
    Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    blob = rng.uniform(-0.6, 0.6, (500, 3))
    line = np.c_[rng.uniform(-1, 1, 300), 0.01 * rng.standard_normal((300, 2))] @ Q.T + 2.0
    sparse = rng.uniform(5, 9, (60, 3))
    xyz = np.concatenate([plane @ Q.T - 3.0, blob, line, sparse]).astype(np.float32)
    ref = mo.metrics(xyz, 0.3, 8)
    got = host_metrics(emul, xyz, 0.3, 8)
    got["entropy"] = np.where(got["valid"] > 0, got["entropy"], np.nan)
    fig = mo.check_parity(got, ref, 0.3)
    assert 0.5 < ref["valid"].mean() < 0.99 and fig["sharp_share"] > 0.4, fig


def test_lattice_against_closed_form(emul):
    for shift in ((0, 0, 0), (1000.25, -517.5, 0)):
        p = mo.lattice(shift)
        got = host_metrics(emul, p, 0.25, 4)
        ref = mo.metrics(p, 0.25, 4)
        assert np.array_equal(got["count"], ref["count"])
        assert [int((got["count"] == c).sum()) for c in (4, 5, 6, 7)] == [8, 48, 96, 64]
        assert np.array_equal(got["valid"] > 0, ref["valid"]) and ref["valid"].all()
        inner = got["count"] == 7
        assert np.abs(got["entropy"][inner] - mo.LATTICE_INTERIOR_ENTROPY).max() <= 1e-12
        assert abs(mo.LATTICE_INTERIOR_ENTROPY - (-1.781211936)) < 1e-9
        assert np.abs(got["plane_var"][inner] - 2 * 0.0625 / 7).max() <= 1e-15


def test_oracle_true_poses_give_the_sharper_map(emul):
    """The shared case: 6 000 points, 87.9 % of the queries valid at the true poses, MME -4.003 there against -3.453 at the
    noisy poses (MPV 1.77e-3 against 2.25e-3).  The host-built device chain meets the GPU test's bars on it."""
    c = mo.scan_case()
    gt, noisy = c["ref"]["gt"], c["ref"]["noisy"]
    assert gt["n_points"] == 6000 and abs(gt["n_valid"] / 6000 - 0.879) < 0.002
    assert abs(gt["mme"] - (-4.003)) < 2e-3 and abs(noisy["mme"] - (-3.453)) < 2e-3
    assert abs(gt["mpv"] - 1.77e-3) < 1e-5 and abs(noisy["mpv"] - 2.25e-3) < 1e-5
    assert gt["mme"] < noisy["mme"] - 0.2 and gt["mpv"] < noisy["mpv"]
    for name in ("gt", "noisy"):
        got = host_metrics(emul, c["world"][name], 0.3, 8)
        got["entropy"] = np.where(got["valid"] > 0, got["entropy"], np.nan)
        fig = mo.check_parity(got, c["ref"][name], 0.3)
        assert fig["sharp_share"] >= 0.7, fig
        s3 = mo.strided(c["ref"][name], 3)
        assert s3["n_queries"] == 2000 and np.array_equal(s3["count"], mo.metrics(c["world"][name], 0.3, 8, 3)["count"])
