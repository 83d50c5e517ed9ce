"""CPU tests of the three shared pieces of the Python binding (_lib.Handle, _lib.make_opts, Struct.as_dict).  The
lvba_*_default_opts functions are host only, so none of this needs a device."""
import ctypes
import importlib

import pytest

HANDLE_CLASSES = {          # module -> the classes that own a library handle
    "balm": ("BalmProblem",), "visual": ("VisualProblem", "DepthImages"), "voxel": ("Scans", "VoxelMap", "SubmapSet"),
    "trackgraph": ("TrackGraph",), "colorize": ("ColorMap",), "match": ("Matcher",), "verify": ("Verifier",),
}
# the option tuples as they were typed out before they were derived from the structs
TUPLES = {
    ("verify", "OPTION_NAMES"): ("method", "hypotheses", "refine_rounds", "min_inliers", "max_error_px", "seed"),
    ("resect", "OPTION_NAMES"): ("hypotheses", "refine_rounds", "min_inliers", "max_error_px", "seed"),
    ("match", "OPTION_NAMES"): ("max_distance", "max_ratio", "mutual", "guided", "max_epipolar_px", "max_reproj_px"),
    ("covis", "INT_OPTIONS"): ("grid_x", "grid_y", "search_radius", "occlusion", "both_ways", "max_per_image", "min_shared"),
    ("covis", "FLOAT_OPTIONS"): ("min_overlap", "occlusion_rel", "occlusion_abs"),
    ("covis", "OPTION_NAMES"): ("grid_x", "grid_y", "search_radius", "occlusion", "both_ways", "max_per_image", "min_shared",
                                "min_overlap", "occlusion_rel", "occlusion_abs"),
    ("features", "OPTION_NAMES"): ("first_octave", "n_intervals", "sigma0", "dog_threshold", "edge_threshold", "orientation_window",
                                   "max_orientations", "max_features", "chunk_images"),
    ("posegraph", "POSEGRAPH_OPTS"): ("anchor", "max_iter", "odom_sigma_rot", "odom_sigma_pos", "anchor_sigma_rot",
                                      "anchor_sigma_pos", "rel_tol", "closure_loss"),
    ("dynamic", "OPTIONS"): ("n_rows", "n_cols", "halo", "window", "min_free", "batch_frames", "el_min", "el_max", "min_range",
                             "max_range", "abs_tol", "rel_tol", "free_ratio"),
    ("register", "OPTS"): ("max_iterations", "max_distance", "min_inliers", "min_eigenvalue", "tol_rot", "tol_pos"),
    ("register", "LOOP_OPTS"): ("submap_size", "min_gap", "max_per_frame", "query_stride", "radius"),
    ("register", "PLACE_OPTS"): ("n_rings", "n_sectors", "min_range", "max_range", "z_offset", "submap_size", "min_gap",
                                 "n_key_candidates", "max_per_frame", "query_stride", "max_distance"),
    ("register", "CLOSURE_OPTS"): ("rot_tol", "rot_rate", "trans_tol", "trans_rate", "n_seeds", "min_set"),
}


def module(name):
    return importlib.import_module("global-lvba_amd." + name)


@pytest.fixture(scope="module")
def L(pkg):
    import __graft_entry__ as ge
    ge.build()
    pkg._lib.load()
    return pkg._lib


class CountingLib:
    """stands in for the loaded library: counts the calls of every lvba_* name"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("lvba_"):
            raise AttributeError(name)
        return lambda h: self.calls.append((name, getattr(h, "value", h)))


def make_thing(L, handle):
    class Thing(L.Handle):
        _destroy = "lvba_thing_destroy"

        def __init__(self, lib, handle, fail=False):
            self.lib = lib
            if fail:
                raise ValueError("before the handle")
            self._h = handle
    lib = CountingLib()
    return Thing, lib, Thing(lib, handle)


def test_handle_close_twice_destroys_once(L):
    _, lib, t = make_thing(L, ctypes.c_void_p(0x1234))
    t.close()
    t.close()
    assert lib.calls == [("lvba_thing_destroy", 0x1234)] and not t._h
    del t
    assert len(lib.calls) == 1


@pytest.mark.parametrize("none", [None, 0, "empty"])
def test_handle_without_a_handle_destroys_nothing(L, none):
    _, lib, t = make_thing(L, ctypes.c_void_p() if none == "empty" else none)
    t.close()
    t.__del__()
    assert lib.calls == []


def test_handle_closes_on_exit_and_on_exception(L):
    Thing, lib, t = make_thing(L, ctypes.c_void_p(7))
    with t as inside:
        assert inside is t and lib.calls == []
    assert lib.calls == [("lvba_thing_destroy", 7)]
    u = Thing(lib, 9)                                   # a plain integer is a handle too
    with pytest.raises(KeyError):
        with u:
            raise KeyError("inside")
    assert lib.calls[1:] == [("lvba_thing_destroy", 9)]


def test_handle_del_after_a_failed_init_is_silent(L):
    Thing, lib, _ = make_thing(L, None)
    t = Thing.__new__(Thing)                            # what is left when __init__ raises before _h (and lib) exist
    t.__del__()
    with pytest.raises(ValueError):
        Thing(lib, 5, fail=True)
    broken = Thing.__new__(Thing)
    broken._h = ctypes.c_void_p(5)                      # a handle but no library: close raises, __del__ swallows it
    with pytest.raises(AttributeError):
        broken.close()
    broken.__del__()
    assert lib.calls == []


def test_every_handle_class_names_an_exported_destroy_symbol(L):
    seen = set()
    for mod, names in HANDLE_CLASSES.items():
        for name in names:
            cls = getattr(module(mod), name)
            assert issubclass(cls, L.Handle) and cls._destroy in L.SYMBOLS and cls._destroy.endswith("_destroy"), name
            assert all(m not in vars(cls) for m in ("close", "__del__", "__enter__", "__exit__")), name
            seen.add(cls._destroy)
    assert module("voxel").SubmapSet._destroy == module("voxel").VoxelMap._destroy
    assert seen == {s for s in L.SYMBOLS if s.endswith("_destroy")}


def opts_structs(L):
    """every struct with an lvba_*_default_opts: each of those symbols takes a pointer to one"""
    found = [getattr(L.load(), s).argtypes[0]._type_ for s in L.SYMBOLS if s.endswith("_default_opts")]
    assert len(found) >= 20 and all(c in L.STRUCTS.values() for c in found)
    return found


def test_make_opts_gives_the_library_defaults_byte_for_byte(L):
    lib = L.load()
    for cls in opts_structs(L):
        c_name = next(n for n, c in L.STRUCTS.items() if c is cls)
        want = cls()
        getattr(lib, c_name.replace("_opts", "_default_opts"))(ctypes.byref(want))
        assert bytes(L.make_opts(cls, "test")) == bytes(want), c_name
        assert any(bytes(want)), c_name                 # the defaults are not all zero: the call did write


def test_make_opts_rejects_what_is_not_an_option(L):
    for cls in opts_structs(L):
        names = L.option_names(cls)
        others = [f for f, _ in cls._fields_ if f not in names]       # padding, losses, arrays, nested structs
        assert all(f in L.PADDING or not issubclass(t, ctypes._SimpleCData) for f, t in cls._fields_ if f in others)
        for bad in ["no_such_option", "reserved", "pad"] + others:
            with pytest.raises(TypeError) as e:
                L.make_opts(cls, "test-kind", **{bad: 1})
            assert "test-kind" in str(e.value) and repr(bad) in str(e.value) and all(n in str(e.value) for n in names)
    with pytest.raises(TypeError) as e:
        L.make_opts(L.RegisterOpts, "registration", ("loss",), bogus=1)
    assert "'loss'" in str(e.value)


def test_make_opts_coerces_by_the_field_type(L):
    floats = (ctypes.c_double, ctypes.c_float)
    for cls in opts_structs(L):
        types = dict(cls._fields_)
        for name in L.option_names(cls):
            o = L.make_opts(cls, "test", **{name: 2} if types[name] in floats else {name: 3.0})
            v = getattr(o, name)
            assert (type(v), v) == ((float, 2.0) if types[name] in floats else (int, 3)), (cls.__name__, name)
    for cls in (L.VerifyOpts, L.ResectOpts):
        assert dict(cls._fields_)["seed"] is ctypes.c_uint64
        assert L.make_opts(cls, "test", seed=2**63 + 5).seed == 2**63 + 5


def test_option_tuples_are_what_was_typed_out(L):
    for (mod, name), want in TUPLES.items():
        assert getattr(module(mod), name) == want, (mod, name)


def test_losses_keep_their_two_meanings_of_none(L):
    default = module("register")._opts({})
    assert bytes(module("register")._opts(dict(loss=None))) == bytes(default)            # None: the library's default
    assert module("register")._opts(dict(loss=("huber", 0.5))).loss.kind == L.LOSS_KINDS["huber"]
    pg = module("posegraph")
    none = pg.posegraph_opts(closure_loss=None)
    assert (none.closure_loss.kind, none.closure_loss.scale) == (0, 0.0)                 # None: TRIVIAL, whatever the default
    some = pg.posegraph_opts(closure_loss=("cauchy", 2.0), max_iter=7.0)
    assert (some.closure_loss.kind, some.closure_loss.scale, some.max_iter) == (L.LOSS_KINDS["cauchy"], 2.0, 7)


def fill(struct):
    """distinct values in every scalar and array element: 1, 2, 3, ... in declaration order"""
    k = 0
    for f, t in struct._fields_:
        if issubclass(t, ctypes.Array):
            for i in range(t._length_):
                k += 1
                getattr(struct, f)[i] = k
        else:
            k += 1
            setattr(struct, f, k)
    return struct


def test_as_dict_of_the_seven_structs(L):
    assert fill(L.LmTrace()).as_dict() == dict(iter=1, accepted=2, evaluated=3, status=4, residual1=5.0, residual2=6.0, u=7.0,
                                               v=8.0, q=9.0, q1=10.0)
    assert fill(L.VisualTrace()).as_dict() == dict(iter=1, accepted=2, valid=3, cost=5.0, cost_change=6.0, step_norm=7.0,
                                                   radius=8.0, rho=9.0, gradient_max_norm=10.0)              # no `reserved`
    assert fill(L.PosegraphReport()).as_dict() == dict(iterations=1, accepted=2, status=3, solver_kind=4, cost_first=5.0,
                                                       cost_last=6.0, odom_cost_last=7.0, closure_cost_last=8.0,
                                                       max_step_last=9.0)
    assert fill(L.RegisterResult()).as_dict() == dict(status=1, iterations=2, inliers=3, points=4, cost_first=5.0, cost_last=6.0,
                                                      rmse=7.0, min_eigenvalue=8.0)
    assert fill(L.TrackGraphInfo()).as_dict() == dict(n_nodes=1, n_edges=2, n_skipped=3, n_components_all=4, n_components=5,
                                                      n_observations=6, largest_component=7, cc_rounds=8)    # no `reserved`
    assert fill(L.WindowInfo()).as_dict() == dict(start=1, n_frames=2, skipped=3, anchor=4, n_iter=5, lm_status=6, n_voxels=7,
                                                  n_factors=8, n_anchor_points=9, cost_first=10.0, cost_last=11.0, map_ms=12.0,
                                                  solve_ms=13.0, merge_ms=14.0, setup_ms=15.0)
    got = fill(L.LidarBaReport()).as_dict()
    assert got == dict(n_frames=1, n_windows=2, n_windows_skipped=3, n_anchors=4, stage_ran=[5, 6], stage_iters=[7, 8],
                       stage_status=[9, 10], reserved=11, stage_voxels=[12, 13], stage_factors=[14, 15],
                       stage_cost_first=[16.0, 17.0], stage_cost_last=[18.0, 19.0], window_ms=20.0, stage_ms=[21.0, 22.0])
    assert list(got) == [f for f, _ in L.LidarBaReport._fields_] and all(type(v) is list for v in got.values() if not isinstance(v, (int, float)))
