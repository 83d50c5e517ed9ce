"""GPU tests of the dynamic-point labels and the scan selection (lvba_dynamic_labels, lvba_scans_select;
global-lvba_amd/dynamic.py): every point of every shared fixture and option set (tests/dynamic_cases.py) EQUAL to the numpy
restatement (tests/dynamic_oracle.py) -- the fixtures keep every decision 1e-9 away from its boundary, so no point is left out --,
independence of the output pointers, of the frame batching and of the run, a frame sub-range against a set of its own, the
selection against numpy's boolean indexing and through its consumers, and the argument checks."""
import ctypes as C
import importlib

import numpy as np
import pytest

import dynamic_cases as dc

pytestmark = pytest.mark.gpu

PER_POINT = ("label", "n_free", "n_support")
COUNTS = ("n_points", "n_judged", "n_dynamic")


@pytest.fixture(scope="module")
def dyn(pkg):
    return importlib.import_module("global-lvba_amd.dynamic")


@pytest.fixture(scope="module")
def sets(pkg):
    with pkg.Scans(dc.scene()["clouds"]) as scene, pkg.Scans(dc.edge()["clouds"]) as edge:
        yield dict(scene=scene, edge=edge)


def run(dyn, sets, k, **kw):
    c = dc.case(k)
    return dyn.dynamic_labels(sets[dc.CASES[k][1]], c["poses"], frame_begin=c["frame_begin"], n_frames=c["n_frames"], **dict(c["opts"], **kw))


@pytest.mark.parametrize("k", range(len(dc.CASES)), ids=[c[0] for c in dc.CASES])
def test_every_point_equals_the_oracle(dyn, sets, k):
    ref = dc.case(k)["ref"]
    got = run(dyn, sets, k)
    for key in PER_POINT:
        assert got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (key, np.flatnonzero(got[key] != ref[key])[:10])
    assert {key: got[key] for key in COUNTS} == {key: ref[key] for key in COUNTS}
    print(dc.CASES[k][0], {key: got[key] for key in COUNTS}, got["ms"])


@pytest.mark.parametrize("k", [0, 2, 9])
def test_outputs_do_not_depend_on_pointers_batching_or_the_run(pkg, dyn, sets, k):
    L = pkg._lib
    lib = L.load()
    c = dc.case(k)
    base = run(dyn, sets, k)
    again = run(dyn, sets, k)
    for batch in (1, 2):
        b = run(dyn, sets, k, batch_frames=batch)
        for key in PER_POINT:
            assert b[key].tobytes() == base[key].tobytes() == again[key].tobytes(), (batch, key)
        assert all(b[key] == base[key] == again[key] for key in COUNTS)
    sc, x, o = sets[dc.CASES[k][1]], np.ascontiguousarray(c["poses"]).reshape(-1), dyn._opts(c["opts"])
    P = base["n_points"]
    for which in ((0,), (1,), (2,), (0, 2), ()):
        arr = [np.full(P, 77, t) for t in (np.uint8, np.int32, np.int32)]
        s = L.DynamicSummary()
        ptr = [arr[j].ctypes.data if j in which else None for j in range(3)]
        assert lib.lvba_dynamic_labels(sc._h, x, c["frame_begin"], c["n_frames"], C.byref(o), C.byref(s), *ptr) == L.OK
        for j in which:
            assert arr[j].tobytes() == base[PER_POINT[j]].tobytes(), which
        assert (s.n_points, s.n_judged, s.n_dynamic) == tuple(base[key] for key in COUNTS)
    none = dyn.dynamic_labels(sc, c["poses"], frame_begin=c["frame_begin"], n_frames=c["n_frames"], per_point=False, **c["opts"])
    assert "label" not in none and all(none[key] == base[key] for key in COUNTS)


def test_default_options_and_a_sub_range_against_a_set_of_its_own(pkg, dyn, sets):
    o = dyn.default_opts()
    assert (o.n_rows, o.n_cols, o.halo, o.window, o.min_free, o.batch_frames) == (240, 720, 1, 20, 3, 0)
    assert (o.el_min, o.el_max) == (-dc.PI / 3.0, dc.PI / 3.0)
    assert (o.min_range, o.max_range, o.abs_tol, o.rel_tol, o.free_ratio) == (0.5, 80.0, 0.2, 0.02, 0.5)
    k = 9                                                                          # frame_begin 1
    c = dc.case(k)
    assert c["frame_begin"] > 0
    sub = run(dyn, sets, k)
    with pkg.Scans(c["clouds"][c["frame_begin"]:c["frame_begin"] + c["n_frames"]]) as own:
        alone = dyn.dynamic_labels(own, c["poses"], **c["opts"])
    for key in PER_POINT:
        assert sub[key].tobytes() == alone[key].tobytes()
    # NULL options are the defaults
    L = pkg._lib
    s1, s2 = L.DynamicSummary(), L.DynamicSummary()
    sc = dc.scene()
    x = np.ascontiguousarray(sc["poses"]).reshape(-1)
    a, b = np.zeros(9600, np.uint8), np.zeros(9600, np.uint8)
    assert L.load().lvba_dynamic_labels(sets["scene"]._h, x, 0, 8, None, C.byref(s1), a.ctypes.data, None, None) == L.OK
    assert L.load().lvba_dynamic_labels(sets["scene"]._h, x, 0, 8, C.byref(o), C.byref(s2), b.ctypes.data, None, None) == L.OK
    assert a.tobytes() == b.tobytes() and (s1.n_judged, s1.n_dynamic) == (s2.n_judged, s2.n_dynamic) and s1.n_judged > 0


def _frames(scans):
    return [scans.download(f) for f in range(scans.n_frames)]


def test_selection_equals_numpy_and_feeds_every_consumer(pkg, dyn, sets):
    mq = importlib.import_module("global-lvba_amd.mapq")
    e = dc.edge()
    P = sum(dc.EDGE_SIZES)
    rng = np.random.default_rng(3)
    first_three = 63 + 1 + 64
    masks = dict(random=rng.integers(0, 2, P).astype(np.uint8), none=np.zeros(P, np.uint8), all=np.ones(P, np.uint8),
                 frames_0_to_2_empty=(np.arange(P) >= first_three).astype(np.uint8) * 7)
    for name, keep in masks.items():
        with dyn.select_scans(sets["edge"], keep) as got:
            at = 0
            assert got.n_frames == 6, name
            for f, c in enumerate(e["clouds"]):
                want = c[keep[at:at + len(c)] != 0]
                at += len(c)
                assert got.counts[f] == len(want) and got.download(f).tobytes() == want.tobytes(), (name, f)
    # the static scans of the scene through a voxel map and the map quality, against a set made from the selected host arrays
    sc = dc.scene()
    label = dc.case(0)["ref"]["label"]
    at, host = 0, []
    for c in sc["clouds"]:
        host.append(np.ascontiguousarray(c[label[at:at + len(c)] == 0]))
        at += len(c)
    with dyn.static_scans(sets["scene"], label) as st, pkg.Scans(host) as want:
        assert [len(h) for h in host] == list(st.counts) and sum(st.counts) == 9600 - 34
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_frames(st), host))
        qa = mq.map_quality_scans(st, sc["poses"], radius=0.8, min_neighbors=6, per_point=True)
        qb = mq.map_quality_scans(want, sc["poses"], radius=0.8, min_neighbors=6, per_point=True)
        assert qa["n_valid"] == qb["n_valid"] > 0 and qa["entropy"].tobytes() == qb["entropy"].tobytes() and qa["mme"] == qb["mme"]
        with st.voxel_map(sc["poses"], voxel_size=2.0) as ma, want.voxel_map(sc["poses"], voxel_size=2.0) as mb:
            ea, eb = ma.export(), mb.export()
            counts = ("n_points", "n_roots", "n_planes", "n_voxels", "n_factors")
            assert [ma.info[key] for key in counts] == [mb.info[key] for key in counts] and ma.info["n_points"] == 9600 - 34
            for a, b in zip(ea, eb):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        # and the labels of the static scans hold no planted point any more
        assert dyn.dynamic_labels(st, sc["poses"], **sc["opts"])["n_dynamic"] == 0


def test_argument_errors_leave_the_scans_usable(pkg, dyn, sets):
    L = pkg._lib
    lib = L.load()
    sc, c = sets["edge"], dc.case(2)
    x = c["poses"]
    nan, inf = float("nan"), float("inf")
    bad_opts = (dict(n_rows=0), dict(n_rows=1025), dict(n_cols=0), dict(n_cols=4097), dict(halo=-1), dict(halo=4),
                dict(el_min=0.5, el_max=0.5), dict(el_min=0.6, el_max=0.5), dict(el_min=-1.6), dict(el_max=1.6), dict(el_min=nan),
                dict(min_range=-0.1), dict(min_range=8.0), dict(min_range=9.0), dict(min_range=nan), dict(max_range=nan),
                dict(abs_tol=-0.1), dict(abs_tol=nan), dict(abs_tol=inf), dict(rel_tol=-0.1), dict(rel_tol=nan), dict(rel_tol=inf),
                dict(min_free=0), dict(free_ratio=0.0), dict(free_ratio=1.5), dict(free_ratio=nan), dict(batch_frames=-1))
    for kw in bad_opts:
        with pytest.raises(L.LvbaError) as e:
            dyn.dynamic_labels(sc, x, **dict(c["opts"], **kw))
        assert e.value.code == L.ERR_ARG, kw
    for fb, nf in ((-1, 1), (5, 2), (0, 0), (0, 7), (6, 1)):
        with pytest.raises(L.LvbaError) as e:
            dyn.dynamic_labels(sc, np.tile(x[:1], (max(nf, 0), 1)), frame_begin=fb, n_frames=nf, **c["opts"])
        assert e.value.code == L.ERR_ARG, (fb, nf)
    for v in (nan, inf):
        bad = x.copy(); bad[3, 10] = v
        with pytest.raises(L.LvbaError) as e:
            dyn.dynamic_labels(sc, bad, **c["opts"])
        assert e.value.code == L.ERR_ARG
    o, s = dyn._opts(c["opts"]), L.DynamicSummary()
    flat = np.ascontiguousarray(x).reshape(-1)
    assert lib.lvba_dynamic_labels(None, flat, 0, 6, C.byref(o), C.byref(s), None, None, None) == L.ERR_ARG
    assert lib.lvba_dynamic_labels(sc._h, flat, 0, 6, C.byref(o), None, None, None, None) == L.ERR_ARG
    typed = lib.lvba_dynamic_labels.argtypes
    try:                                                                           # (the array type of the poses refuses None)
        lib.lvba_dynamic_labels.argtypes = [C.c_void_p] * 2 + list(typed[2:])
        assert lib.lvba_dynamic_labels(sc._h, None, 0, 6, C.byref(o), C.byref(s), None, None, None) == L.ERR_ARG
    finally:
        lib.lvba_dynamic_labels.argtypes = typed
    h = C.c_void_p()
    keep = np.ones(sum(dc.EDGE_SIZES), np.uint8)
    assert lib.lvba_scans_select(None, keep.ctypes.data, C.byref(h)) == L.ERR_ARG
    assert lib.lvba_scans_select(sc._h, keep.ctypes.data, None) == L.ERR_ARG
    assert lib.lvba_scans_select(sc._h, None, C.byref(h)) == L.ERR_ARG and not h.value
    with pytest.raises(ValueError):
        dyn.select_scans(sc, keep[:-1])
    with pytest.raises(TypeError):
        dyn.dynamic_labels(sc, x, no_such_option=1)
    ok = dyn.dynamic_labels(sc, x, **c["opts"])
    assert np.array_equal(ok["label"], c["ref"]["label"])
