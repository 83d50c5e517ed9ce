"""CPU tests of the dynamic-point labels: the device header (csrc/dynamic_device.h) compiled for the host against the numpy
restatement (tests/dynamic_oracle.py) on every shared fixture and option set (tests/dynamic_cases.py), the conditions on the
fixtures and the struct layouts."""
import ctypes
import importlib

import numpy as np
import pytest

from host_build import build_check

import dynamic_cases as dc
import dynamic_oracle as do


class EmulOpts(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int32), ("n_cols", ctypes.c_int32), ("halo", ctypes.c_int32), ("window", ctypes.c_int32),
                ("min_free", ctypes.c_int32), ("batch_frames", ctypes.c_int32), ("el_min", ctypes.c_double), ("el_max", ctypes.c_double),
                ("min_range", ctypes.c_double), ("max_range", ctypes.c_double), ("abs_tol", ctypes.c_double), ("rel_tol", ctypes.c_double),
                ("free_ratio", ctypes.c_double)]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = ctypes.CDLL(build_check("dynamic_check", tmp_path_factory.mktemp("emul_dynamic")))
    f32, f64, i32, i64, u8 = (np.ctypeslib.ndpointer(t, flags="C") for t in (np.float32, np.float64, np.int32, np.int64, np.uint8))
    lib.emul_image.argtypes = [ctypes.c_int64, f32, ctypes.POINTER(EmulOpts), i32, f32, f32]
    lib.emul_image.restype = None
    lib.emul_labels.argtypes = [ctypes.c_int, i64, f32, f64, ctypes.POINTER(EmulOpts), ctypes.c_int, u8, i32, i32]
    lib.emul_labels.restype = None
    return lib


def host_image(emul, cloud, **kw):
    o = EmulOpts(batch_frames=0, **do.options(**kw))
    xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    cell = np.zeros(max(len(xyz), 1), np.int32)
    I, M = np.zeros((o.n_rows, o.n_cols), np.float32), np.zeros((o.n_rows, o.n_cols), np.float32)
    emul.emul_image(len(xyz), xyz if len(xyz) else np.zeros((1, 3), np.float32), ctypes.byref(o), cell, I, M)
    return cell[:len(xyz)], I, M


def host_labels(emul, c, batch=0):
    o = EmulOpts(batch_frames=0, **do.options(**c["opts"]))
    use = c["clouds"][c["frame_begin"]:c["frame_begin"] + c["n_frames"]]
    off = np.concatenate([[0], np.cumsum([len(x) for x in use])]).astype(np.int64)
    xyz = np.ascontiguousarray(np.concatenate(use + [np.zeros((1, 3), np.float32)]))
    P = int(off[-1])
    label, nf, ns = np.zeros(P + 1, np.uint8), np.zeros(P + 1, np.int32), np.zeros(P + 1, np.int32)
    emul.emul_labels(len(use), off, xyz, np.ascontiguousarray(c["poses"]).reshape(-1), ctypes.byref(o), batch, label, nf, ns)
    return label[:P], nf[:P], ns[:P]


@pytest.mark.parametrize("k", range(len(dc.CASES)), ids=[c[0] for c in dc.CASES])
def test_host_header_matches_oracle(emul, k):
    """Cells and both images bit for bit, votes and labels equal, whatever the batching; and every decision of the case has a
    margin >= 1e-9 (condition 1)."""
    c = dc.case(k)
    ref = c["ref"]
    for f in range(c["n_frames"]):
        cell, I, M = host_image(emul, c["clouds"][c["frame_begin"] + f], **c["opts"])
        assert np.array_equal(cell, ref["own_cell"][f])
        assert I.tobytes() == ref["I"][f].tobytes() and M.tobytes() == ref["M"][f].tobytes()
    for batch in (0, 1, 2):
        label, nf, ns = host_labels(emul, c, batch)
        assert np.array_equal(nf, ref["n_free"]) and np.array_equal(ns, ref["n_support"]) and np.array_equal(label, ref["label"]), batch
    print(f"{c['name']}: {ref['n_points']} points, {ref['n_judged']} judged, {ref['n_dynamic']} dynamic, margin {ref['margin']:.2e}")
    assert ref["margin"] >= 1e-9


def test_scene_meets_its_conditions():
    """Conditions 2 and 3 of tests/dynamic_cases.py, and the measured shares."""
    sc, c = dc.scene(), dc.case(0)
    ref, planted = c["ref"], sc["planted"]
    assert c["opts"] == dc.SCENE and len(sc["clouds"]) == 8 and all(len(x) == 1200 for x in sc["clouds"])
    # every cell of every frame's own image holds a sample: the 3 x 3 neighbourhoods read the room, not +inf
    assert all(np.isfinite(i).all() for i in ref["I"])
    assert int(ref["label"][~planted].sum()) == 0                                                  # 2
    seen = dc.seen_through(sc, c["opts"])
    counted = planted & (seen >= do.options(**c["opts"])["min_free"])
    hit = int(ref["label"][counted].sum())
    print(f"planted {int(planted.sum())}, counted {int(counted.sum())}, labelled dynamic {hit}; static points {int((~planted).sum())}, "
          f"labelled dynamic 0; judged {ref['n_judged']} of {ref['n_points']}")
    assert counted.sum() >= 30 and hit >= 0.9 * counted.sum()                                      # 3
    assert np.array_equal(np.flatnonzero(ref["label"]), np.flatnonzero(planted & (ref["label"] != 0)))


def test_edge_fixture_holds_every_special_point():
    e = dc.edge()
    o = do.options(**e["opts"])
    assert tuple(len(c) for c in e["clouds"]) == dc.EDGE_SIZES == (63, 1, 64, 0, 65, 257)
    info = do.cells(e["clouds"][5][:e["n_special"]].astype(np.float64), **o)
    cell = info["cell"]
    nc, nr = o["n_cols"], o["n_rows"]
    assert [int(c % nc) for c in cell[:4]] == [0, nc - 1, 0, nc - 1]                               # the halo wraps
    assert [int(c // nc) for c in cell[4:8]] == [0, nr - 1, 0, nr - 1]                             # the halo is clipped
    assert [int(c // nc) if c >= 0 else -1 for c in cell[8:12]] == [0, -1, nr - 1, -1]             # el_min, el_max: inside, outside
    q = do.to_body(do.world_points(e["clouds"][5][12:14], e["poses"][5]), e["poses"][2])
    assert (q[:, :2] == 0.0).all() and list(do.cells(q, **o)["cell"]) == [-1, -1]                  # on the axis of frame 2
    assert list(cell[12:14] >= 0) == [True, True]                                                  # but off their own frame's
    assert list(cell[14:18] >= 0) == [False, False, True, False]                                   # min_range, max_range
    assert list(cell[18:22]) == [-1] * 4                                                           # NaN, inf
    ref = dc.case(2)["ref"]
    bad = sum(dc.EDGE_SIZES[:5]) + np.arange(18, 22)
    assert not ref["n_free"][bad].any() and not ref["n_support"][bad].any()
    # both kinds of vote, both labels, and points without any evidence occur in every all-frames case
    assert ref["n_dynamic"] > 0 and (ref["n_support"] > 0).any() and ref["n_judged"] < ref["n_points"]
    names = [c[0] for c in dc.CASES]
    assert any("window 1" in n for n in names) and any("window 2 of 5" in n for n in names) and any("window 0" in n for n in names)
    assert {dc.case(k)["opts"].get("halo", 1) for k in range(len(dc.CASES))} >= {0, 1, 3}
    assert any(c[3] == 1 for c in dc.CASES) and any(c[2] > 0 for c in dc.CASES)


def test_selection_equals_boolean_indexing():
    e = dc.edge()
    rng = np.random.default_rng(3)
    P = sum(dc.EDGE_SIZES)
    masks = [rng.integers(0, 2, P).astype(np.uint8), np.zeros(P, np.uint8), np.ones(P, np.uint8), (np.arange(P) >= 63 + 1 + 64).astype(np.uint8) * 7]
    for keep in masks:
        got = do.select(e["clouds"], keep)
        at = 0
        for c, g in zip(e["clouds"], got):
            want = c[keep[at:at + len(c)] != 0]
            assert g.shape == want.shape and g.tobytes() == want.tobytes()
            at += len(c)


def test_dynamic_struct_sizes_match_the_header():
    L = importlib.import_module("global-lvba_amd._lib")
    # the mirrors against the header: tests/test_abi.py, every struct at once; here the check program's own copy of the options
    assert ctypes.sizeof(L.DynamicOpts) == 80 == ctypes.sizeof(EmulOpts) and ctypes.sizeof(L.DynamicSummary) == 56
    assert [f for f, _ in L.DynamicOpts._fields_] == [f for f, _ in EmulOpts._fields_]
    assert all(s in L.SYMBOLS for s in ("lvba_dynamic_default_opts", "lvba_dynamic_labels", "lvba_scans_select"))
    dyn = importlib.import_module("global-lvba_amd.dynamic")
    assert set(dyn.OPTIONS) == {f for f, _ in L.DynamicOpts._fields_} and set(do.DEFAULTS) == set(dyn.OPTIONS) - {"batch_frames"}
