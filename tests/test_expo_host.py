"""CPU tests of the per-image exposure compensation (include/lvba_hip.h "per-image exposure compensation of the colour fusion",
DESIGN.md §10r): the oracle against the rule as plain loops, the device header compiled for the host against the oracle bit for
bit, the solve and the gauge against Python integers -- on the fixture, at the 2^64 bound and with negative numerators --, a closed
form that needs no oracle, the claim -- the compensated spread gets past the geometric mean of the raw and the clean one, and
still tells planted cameras from turned ones --, and the wiring of the pipeline."""
import ctypes
import importlib
import json
import sqlite3
import sys

import numpy as np
import pytest

import covis_cases as cc
import expo_cases as ec
import expo_oracle as eo
import match_cases as mc
import photo_cases as pc
import photo_oracle as po
from host_build import build_check


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """csrc/expo_device.h compiled for the host with g++ -ffp-contract=off -Wall -Werror (tests/expo_check.cpp)"""
    lib = ctypes.CDLL(build_check("expo_check", tmp_path_factory.mktemp("emul_expo")))
    P, I, Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.emul_apply.argtypes = [Q, Q, Q, P, P]
    lib.emul_sums.argtypes = [Q, P, P, P, I, I, I, P, P, P, P, P, P, P, P, P]
    lib.emul_fuse.argtypes = [Q, P, I, I, I, P, P, P, P, P, P, P, P, P, P, P]
    lib.emul_solve.argtypes = [Q, P, P, P, P, P]
    lib.emul_gains_ok.argtypes = [P, Q]
    lib.emul_apply.restype = lib.emul_sums.restype = lib.emul_fuse.restype = lib.emul_solve.restype = None
    return lib


def ptr(x):
    return x.ctypes.data


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host_sums(emul, points, images, depth, intr, Rcw, tcw, ref16, valid, gains=None, **kw):
    o = dict(eo.DEFAULTS, **kw)
    M, H, W = images.shape[:3]
    out = np.zeros((M, eo.N_SUMS), np.uint64)
    bounds = np.array([o["occlusion_rel"], o["occlusion_abs"], o["max_depth"]], np.float64)
    flags = np.array([o["holes"], o["sat_lo"], o["sat_hi"], o["gate"]], np.int32)
    g = None if gains is None else np.ascontiguousarray(gains, np.int64)
    emul.emul_sums(len(points), ptr(points), ptr(np.ascontiguousarray(ref16, np.uint16)), ptr(np.ascontiguousarray(valid, np.uint8)), M, W, H,
                   None if depth is None else ptr(depth), ptr(np.ascontiguousarray(Rcw)), ptr(np.ascontiguousarray(tcw)), ptr(images),
                   ptr(np.ascontiguousarray(intr, np.float64)), ptr(bounds), ptr(flags), None if g is None else ptr(g), ptr(out))
    return out


def host_fuse(emul, points, images, depth, intr, Rcw, tcw, gains, **kw):
    o = dict(eo.DEFAULTS, **kw)
    M, H, W = images.shape[:3]
    n = len(points)
    nv, s1, s2 = np.zeros(n, np.int32), np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.int64)
    bounds = np.array([o["occlusion_rel"], o["occlusion_abs"], o["max_depth"]], np.float64)
    flags = np.array([o["holes"]], np.int32)
    g = np.ascontiguousarray(gains, np.int64)
    emul.emul_fuse(n, ptr(points), M, W, H, None if depth is None else ptr(depth), ptr(np.ascontiguousarray(Rcw)), ptr(np.ascontiguousarray(tcw)),
                   ptr(images), ptr(np.ascontiguousarray(intr, np.float64)), ptr(bounds), ptr(flags), ptr(g), ptr(nv), ptr(s1), ptr(s2))
    return nv, s1, s2


def host_solve(emul, sums, **kw):
    o = dict(eo.DEFAULTS, **kw)
    s = np.ascontiguousarray(sums, np.uint64).reshape(-1, eo.N_SUMS)
    gains, status = np.zeros((len(s), 3, 2), np.int64), np.zeros(len(s), np.int32)
    ints = np.array([o["model"], o["min_samples"], o["min_spread"]], np.int32)
    lims = np.array(eo.limits(o), np.int64)
    emul.emul_solve(len(s), ptr(s), ptr(ints), ptr(lims), ptr(gains), ptr(status))
    return gains, status


# ------------------------------------------------------------------------------------------------------ 1. the compensated sample
def test_identity_gains_return_the_sample(emul):
    """c' under (65536, 0) is c16 for every value 0 .. 65 280; and the clamp and the floor of a negative numerator, header against
    Python integers"""
    c = np.arange(eo.C_MAX + 1, dtype=np.int32)
    out = np.zeros_like(c)
    emul.emul_apply(len(c), eo.ONE, 0, ptr(c), ptr(out))
    assert same_bytes(out, c) and (eo.apply(eo.ONE, 0, c) == c).all()
    rng = np.random.default_rng(1)
    probe = np.ascontiguousarray(np.concatenate([[0, 1, 255, 256, 32640, 65279, 65280], rng.integers(0, eo.C_MAX + 1, 500)]).astype(np.int32))
    for A, B in ((eo.A_MIN, -eo.B_MAX), (eo.A_MAX, eo.B_MAX), (eo.A_MIN, 0), (eo.A_MAX, -eo.B_MAX), (65535, -32769), (65537, -1), (70000, -3 * 65536 - 1),
                 (40000, 7 * 65536 * 256 + 12345), (eo.ONE, -32768), (eo.ONE, -32769)):
        emul.emul_apply(len(probe), A, B, ptr(probe), ptr(out[:len(probe)]))
        want = [eo.loops_apply(A, B, int(v)) for v in probe]
        assert out[:len(probe)].tolist() == want and eo.apply(A, B, probe).tolist() == want, (A, B)
    assert eo.loops_apply(eo.ONE, -32769, 0) == 0 and (-1) // 65536 == -1       # the numerator -1 floors to -1, then the clamp
    ok = np.array([[eo.A_MIN, eo.B_MAX], [eo.A_MAX, -eo.B_MAX]], np.int64)
    assert emul.emul_gains_ok(ptr(ok), 2) == 1
    for bad in ([eo.A_MIN - 1, 0], [eo.A_MAX + 1, 0], [eo.ONE, eo.B_MAX + 1], [eo.ONE, -eo.B_MAX - 1]):
        g = np.array([[eo.ONE, 0], bad], np.int64)
        assert emul.emul_gains_ok(ptr(g), 2) == 0, bad


# ------------------------------------------------------------------------------------------------------------- 2. the oracle
def test_oracle_equals_the_rule_as_loops():
    """the 37 x 29 images, every 7th point, all 21 images, every option set, under the gains of a first round: the 20 sums"""
    s = ec.scene(1)
    take = np.arange(0, cc.N_PLANTED, 7)
    for kw in ec.OPTION_SETS:
        with_depth, opts = ec.split(kw)
        ref16, valid, gains, _ = ec.second_round(1, **kw)
        depth = s["depth"] if with_depth else None
        args = (s["points"][take], s["images"], depth, s["intr"], s["Rcw"], s["tcw"], ref16[take], valid[take], gains)
        want = eo.loops_sums(*args, **opts)
        got = eo.sums(*args, **opts)
        assert got.tolist() == want, kw
        assert got[:, 18].sum() > 300 and got[:, 0].sum() > 200


def test_fixture_conditions():
    worst = pc.check_margins()                                                  # where a point is located does not depend on the colours
    assert worst["compare"] >= mc.MIN_MARGIN and worst["texel"] >= pc.TEXEL_MARGIN
    for size in range(len(cc.SIZES)):
        s = ec.scene(size)
        clipped = (s["images"] == 255).mean()
        assert 0.002 < clipped < 0.05 and (s["images"] > 251).mean() > clipped  # some texels clip, most do not
        ref16, valid, gains, sums = ec.second_round(size, **ec.BASE)
        located = int(sums[:, 18].sum())
        assert (gains != eo.identity(cc.N_IMAGES)).any() and valid.any() and not valid.all()
        assert 0 < int(sums[:, 19].sum())                                       # the gate refuses some terms
        assert 3 * located > int(sums[:, 0:18:6].sum()) + int(sums[:, 19].sum())  # and the saturation test some others
        assert int(sums[:, 0:18:6].sum()) > 2 * located                         # most samples remain
        _, _, _, open_gate = ec.second_round(size, **dict(ec.BASE, gate=0))
        assert not open_gate[:, 19].any() and int(open_gate[:, 0].sum()) > int(sums[:, 0].sum())
        st = ec.estimate(size, **ec.BASE)["status"]
        assert (st == eo.OK).sum() >= 15 and (st == eo.TOO_FEW_SAMPLES).any()
        assert (ec.estimate(size)["status"] == eo.TOO_FEW_SAMPLES).sum() > (st == eo.TOO_FEW_SAMPLES).sum()     # the default of 200


# -------------------------------------------------------------------------------------------------- 3. the header on the host
def test_device_header_on_the_host_equals_the_oracle(emul):
    """every set of 20 sums and every compensated sample of the fusion, bit for bit: both sizes, both models, gate on and off, with
    and without a depth set, under identity gains and under a first round's"""
    for size in range(len(cc.SIZES)):
        s = ec.scene(size)
        for kw in ec.OPTION_SETS:
            with_depth, opts = ec.split(kw)
            depth = s["depth"] if with_depth else None
            ref16, valid, gains, want = ec.second_round(size, **kw)
            args = (s["points"], s["images"], depth, s["intr"], s["Rcw"], s["tcw"])
            assert same_bytes(host_sums(emul, *args, ref16, valid, gains, **opts), want), (size, kw)
            plain = eo.sums(*args, ref16, valid, None, **opts)
            assert same_bytes(host_sums(emul, *args, ref16, valid, None, **opts), plain), (size, kw)
            assert same_bytes(host_sums(emul, *args, ref16, valid, eo.identity(cc.N_IMAGES), **opts), plain), (size, kw)
            nv, s1, s2 = host_fuse(emul, *args, gains, **opts)
            wv, w1, w2 = eo.fuse(*args, gains, **opts)
            assert same_bytes(nv, wv) and same_bytes(s1, w1) and same_bytes(s2, w2), (size, kw)
        e = pc.expected(size)                                                   # identity gains: the plain fusion's bytes
        nv, s1, s2 = host_fuse(emul, s["points"], s["clean"], s["depth"], s["intr"], s["Rcw"], s["tcw"], eo.identity(cc.N_IMAGES))
        assert same_bytes(nv, e["n_views"]) and same_bytes(s1, e["s1"]) and same_bytes(s2, e["s2"])


# --------------------------------------------------------------------------------------------------- 4. the solve and the gauge
def test_solve_equals_python_integers_on_the_fixture(emul):
    for size in range(len(cc.SIZES)):
        for kw in ec.OPTION_SETS:
            _, opts = ec.split(kw)
            e = ec.estimate(size, **kw)
            for sums in (e["sums"], ec.second_round(size, **kw)[3]):
                for extra in (dict(), dict(min_spread=60), dict(max_gain=1.05), dict(max_offset=2.0), dict(min_samples=120)):
                    o = dict(opts, **extra)
                    gains, status = host_solve(emul, sums, **o)
                    want_g, want_s = eo.solve(sums, **o)
                    assert same_bytes(gains, want_g) and same_bytes(status, want_s), (size, kw, extra)
    # every state appears somewhere above
    sums = ec.estimate(0, **ec.BASE)["sums"]
    assert set(eo.solve(sums, **dict(ec.BASE, min_spread=60))[1].tolist()) >= {eo.FALLBACK_GAIN, eo.TOO_FEW_SAMPLES}
    assert eo.OUT_OF_BOUNDS in eo.solve(sums, **dict(ec.BASE, max_gain=1.05))[1].tolist()
    assert eo.OUT_OF_BOUNDS in eo.solve(sums, **dict(ec.BASE, max_offset=2.0))[1].tolist()


def channel(n, sc, sr, scc, scr, see=0):
    return [n, sc, sr, scc, scr, see]


def test_solve_at_the_bound_and_with_negative_numerators(emul):
    """hand-built sums: 2^32 - 1 samples of 65 280 (every sum at its bound, below 2^64); a negative N; a negative B; the gauge"""
    n, c = 2 ** 32 - 1, 65280
    top = channel(n, n * c, n * c, n * c * c, n * c * c, n * c * c)
    assert max(top) < 2 ** 64 and (n + 1) * c * c < 2 ** 64 and c * c < 2 ** 32
    # two images at the bound: D = 0 -> the gain-only form, A = 65536 exactly; both models agree
    half = channel(n, n * c, n * (c // 2), n * c * c, n * c * (c // 2))
    rows = np.array([top * 3 + [n, 0], half * 3 + [n, 0]], np.uint64)
    for model in (0, 1):
        gains, status = host_solve(emul, rows, model=model)
        want_g, want_s = eo.solve(rows, model=model)
        assert same_bytes(gains, want_g) and same_bytes(status, want_s)
        assert status.tolist() == [eo.FALLBACK_GAIN if model == 0 else eo.OK] * 2
        # before the gauge A = (65536, 32768); S = (2 2^32 + 49152) // 98304 and the mean gain becomes 1
        S = (2 * 2 ** 32 + 98304 // 2) // 98304
        assert gains[:, 0, 0].tolist() == [(65536 * S + 32768) >> 16, (32768 * S + 32768) >> 16] and not gains[:, :, 1].any()
        assert abs(int(gains[:, 0, 0].sum()) - 2 * 65536) <= 2
    # the widest D the sums can hold: half the samples at 0, half at 65 280, the reference the other way round: N < 0
    m = 2 ** 31
    anti = channel(2 * m, m * c, m * c, m * c * c, 0)
    D, N = 2 * m * m * c * c - (m * c) ** 2, -(m * c) ** 2
    assert N < 0 < D and (N * 65536 + D // 2) // D == -65536
    rows = np.array([anti * 3 + [2 * m, 0]], np.uint64)
    gains, status = host_solve(emul, rows)
    assert status.tolist() == [eo.OUT_OF_BOUNDS] and same_bytes(gains, eo.identity(1)) and same_bytes(gains, eo.solve(rows)[0])
    # a negative B, floor towards minus infinity: c in {100, 200} x 256 seen as ref = c - 10.3 grey levels (odd numerators)
    lo, hi, k = 100 * 256, 200 * 256, 1000
    for shift in (2637, 2638, 1, 12801):
        sr = k * (lo - shift) + k * (hi - shift)
        neg = channel(2 * k, k * (lo + hi), sr, k * (lo * lo + hi * hi), k * (lo * (lo - shift) + hi * (hi - shift)))
        pos = channel(2 * k, k * (lo + hi), k * (lo + hi) + 2 * k * shift, k * (lo * lo + hi * hi), k * (lo * (lo + shift) + hi * (hi + shift)))
        rows = np.array([neg * 3 + [2 * k, 0], pos * 3 + [2 * k, 0], neg * 3 + [2 * k, 0]], np.uint64)
        gains, status = host_solve(emul, rows, min_samples=2)
        want_g, want_s = eo.solve(rows, min_samples=2)
        assert same_bytes(gains, want_g) and same_bytes(status, want_s) and status.tolist() == [eo.OK] * 3
        assert (gains[0, :, 1] < 0).all() and (gains[1, :, 1] > 0).all()
        # the gauge: mean gain 1 within the rounding, mean offset 0 within one unit per image
        assert abs(int(gains[:, 0, 0].sum()) - 3 * 65536) <= 3 and abs(int(gains[:, 0, 1].sum())) <= 3
    # before the gauge, alone: B = -shift 65536 exactly, and one image's gauge moves it to 0
    gains, _ = host_solve(emul, np.array([neg * 3 + [2 * k, 0]], np.uint64), min_samples=2)
    assert gains[0].tolist() == [[65536, 0]] * 3


# -------------------------------------------------------------------------------------------------------- 5. the closed form
def test_constant_colour_closed_form(emul):
    """image j one colour v_j, the reference one colour r: D = 0, so every image with samples is FALLBACK_GAIN and, before the gauge,
    A_j = (r 2^16 + v_j / 2) // v_j in the 1/256 units both are held in"""
    for size in range(len(cc.SIZES)):
        s = ec.scene(size)
        c = ec.constant_case(size)
        sums = host_sums(emul, s["points"], c["images"], s["depth"], s["intr"], s["Rcw"], s["tcw"], c["ref16"], c["valid"], gate=0)
        seen = pc.expected(size)["seen"].sum(1)
        v, r = 256 * c["colours"], 256 * c["ref"]
        for j in range(cc.N_IMAGES):
            n = int(seen[j])
            for k in range(3):
                vv, rr = int(v[j, k]), int(r[k])
                assert sums[j, 6 * k:6 * k + 6].tolist() == [n, n * vv, n * rr, n * vv * vv, n * vv * rr, n * (vv - rr) ** 2], (j, k)
            assert sums[j, 18] == n and sums[j, 19] == 0
        gains, status = host_solve(emul, sums, min_samples=ec.MIN_SAMPLES)
        live = seen >= ec.MIN_SAMPLES
        assert live.sum() >= 15 and (status[live] == eo.FALLBACK_GAIN).all() and (status[~live] == eo.TOO_FEW_SAMPLES).all()
        for k in range(3):
            A = [(int(r[k]) * 65536 + int(v[j, k]) // 2) // int(v[j, k]) for j in np.flatnonzero(live)]
            assert all(eo.limits(eo.DEFAULTS)[0] <= a <= eo.limits(eo.DEFAULTS)[1] for a in A)
            S = (len(A) * 2 ** 32 + sum(A) // 2) // sum(A)
            assert gains[live, k, 0].tolist() == [(a * S + 32768) >> 16 for a in A] and not gains[live, k, 1].any()
        assert same_bytes(gains[~live], eo.identity(int((~live).sum())))


# ------------------------------------------------------------------------------------------------- 6. the measure means something
# The largest error of a recovered gain against the planted inverse in the solve's gauge, measured on the oracle after the default
# three rounds: 0.096 / 0.141 in the gain and 14.4 / 17.6 grey levels in the offset at 160 x 128 / 37 x 29.  The
# bars are those values with a margin of 0.02 and 3 grey levels: an exposed byte is rounded once more than a clean one (half a
# grey level on colours about 100 grey levels wide: 0.005 in the gain, 0.5 + 0.005 255 = 1.8 grey levels in the offset) and about
# 2 % of the texels clip, which takes the brightest samples out of the images with the highest gains.  What the values themselves
# say is in DESIGN.md: the room's images overlap wall by wall, so after three rounds the walls have not yet agreed on one gauge.
GAIN_BAR = (0.096 + 0.02, 0.141 + 0.02)
OFFSET_BAR = (14.4 + 3.0, 17.6 + 3.0)


def test_the_measure_means_something():
    """orderings on the oracle: compensation lowers the spread past the geometric mean of the raw and the clean one, round by round,
    and a pose error still shows"""
    N = cc.N_CAMERAS
    for size in range(len(cc.SIZES)):
        s = ec.scene(size)
        e = ec.estimate(size, **ec.BASE)
        s_raw, s_comp = e["mean_sigma"][0], e["mean_sigma"][-1]
        s_clean = pc.expected(size)["summary"]["mean_sigma"]
        raw = po.evaluate(s["points"], s["images"], s["depth"], s["intr"], s["Rcw"], s["tcw"])["summary"]["mean_sigma"]
        assert s_raw == raw and len(e["mean_sigma"]) == 4                       # round 0 is the uncompensated fusion
        got = np.stack([e["gains"][..., 0] / 65536.0, e["gains"][..., 1] / (65536.0 * 256.0)], -1)
        want = ec.planted_inverse(e["status"])
        ok = e["status"] <= eo.FALLBACK_GAIN
        err_a, err_b = np.abs(got[ok, :, 0] - want[ok, :, 0]).max(), np.abs(got[ok, :, 1] - want[ok, :, 1]).max()
        print(f"size {cc.SIZES[size]}: spread raw {s_raw:.3f}, compensated {s_comp:.3f} (per round {[round(v, 3) for v in e['mean_sigma']]}), "
              f"clean {s_clean:.3f} grey levels; largest gain error {err_a:.4f}, offset error {err_b:.2f} grey levels over {int(ok.sum())} images")
        assert s_comp < s_raw
        assert s_comp ** 2 < s_raw * s_clean
        assert all(b <= a for a, b in zip(e["mean_sigma"], e["mean_sigma"][1:]))
        assert err_a <= GAIN_BAR[size] and err_b <= OFFSET_BAR[size]
        R, t, depth = pc.turned(size, 0.5, 11)
        turned = eo.estimate(s["points"], s["images"][:N], depth, s["intr"], R, t, **ec.BASE)["mean_sigma"][-1]
        planted = eo.estimate(s["points"], s["images"][:N], s["depth"][:N], s["intr"], s["Rcw"][:N], s["tcw"][:N], **ec.BASE)["mean_sigma"][-1]
        print(f"   18 cameras: compensated spread planted {planted:.3f}, turned by 0.5 degrees {turned:.3f}")
        assert turned > planted                                                 # compensation does not hide a pose error


# ------------------------------------------------------------------------------------------------------------ 7. the binding
def test_struct_size_and_defaults(pkg):
    L = pkg._lib
    assert ctypes.sizeof(L.ExpoOpts) == 80
    EX = importlib.import_module("global-lvba_amd.expo")
    import __graft_entry__ as ge
    ge.build()
    o = EX.expo_opts()
    assert {k: getattr(o, k) for k in EX.OPTION_NAMES} == eo.DEFAULTS
    with pytest.raises(TypeError, match="exposure compensation"):
        EX.expo_opts(no_such=1)
    assert EX.ExposureEstimator._destroy == "lvba_expo_free" and "lvba_expo_free" in L.SYMBOLS
    # the solve needs no device: the library's bytes are the oracle's
    sums = ec.estimate(1, **ec.BASE)["sums"]
    for kw in (ec.BASE, dict(ec.BASE, model=1), dict(), dict(ec.BASE, min_spread=60)):
        gains, status = EX.solve_gains(sums, **kw)
        want_g, want_s = eo.solve(sums, **kw)
        assert same_bytes(gains, want_g) and same_bytes(status, want_s), kw
    assert same_bytes(EX.gains_float(eo.identity(2)), np.tile(np.array([1.0, 0.0]), (2, 3, 1)))
    bad = sums.copy()
    bad[0, 1] = np.uint64(2 ** 63)                                               # a sum no image can have
    with pytest.raises(L.LvbaError):
        EX.solve_gains(bad)
    for kw in (dict(model=2), dict(sat_lo=-1), dict(sat_hi=256), dict(sat_lo=9, sat_hi=8), dict(gate=-1), dict(gate=256), dict(min_samples=1),
               dict(min_spread=-1), dict(min_spread=256), dict(min_gain=0.2), dict(min_gain=1.5), dict(max_gain=0.9), dict(max_gain=4.5),
               dict(max_offset=-1.0), dict(max_offset=256.0), dict(min_gain=float("nan"))):
        with pytest.raises(L.LvbaError):
            EX.solve_gains(sums, **kw)


# ------------------------------------------------------------------------------------------------------------ 8. the pipeline
class _FakeScans:
    device = 0

    def __init__(self, *a, **k):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *e):
        pass


ARGS = ([np.zeros((3, 3), np.float32)], np.zeros((1, 12)), np.zeros(1), np.zeros(2), np.zeros((2, 12)), np.eye(3), np.zeros(3),
        np.ones(8), 640, 512, [np.zeros((5, 2), np.float32)] * 2, [(0, 1)], [np.array([[0, 1], [2, 3]], np.int32)])


def _one(p, tag):
    return dict(summary=dict(n_points=len(p), mean_sigma=tag), n_views=np.zeros(len(p), np.int32), rgb=np.zeros((len(p), 3), np.uint8),
                sigma=np.zeros(len(p)), options=dict(min_views=2))


def test_the_default_path_calls_no_exposure_entry_point(monkeypatch):
    """exposure=None (the default) neither imports the expo module nor looks an lvba_expo_* symbol or lvba_photo_add_images_gains
    up -- in the pipeline with photo_consistency on, and in photo.PhotoMap.add_images / photo.photo_consistency without gains"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    L = importlib.import_module("global-lvba_amd._lib")
    PH = importlib.import_module("global-lvba_amd.photo")
    looked_up = []

    class NoExpoLib:
        def __getattr__(self, name):
            if name.startswith("lvba_expo") or name == "lvba_photo_add_images_gains":
                pytest.fail(f"{name} looked up on the default path")
            if name.startswith("lvba_"):
                looked_up.append(name)
                return lambda *a: 0
            raise AttributeError(name)

    class FakeDepth:
        def __enter__(self):
            return self

        def __exit__(self, *e):
            pass

        _h = None

    visual = dict(Rcw=np.zeros((2, 3, 3)), tcw=np.zeros((2, 3)), Rcw_before=np.zeros((2, 3, 3)), tcw_before=np.zeros((2, 3)))
    cloud = (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8))
    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: dict(visual))
    monkeypatch.setattr(pl, "colorize_maps", lambda *a, **k: dict(after=cloud, before=cloud))
    monkeypatch.setattr(pl.V.DepthImages, "render", staticmethod(lambda *a, **k: FakeDepth()))
    monkeypatch.setattr(L, "load", lambda: NoExpoLib())
    monkeypatch.setattr(L, "make_opts", lambda cls, what, **kw: cls())
    sys.modules.pop("global-lvba_amd.expo", None)
    images = np.zeros((2, 512, 640, 3), np.uint8)
    for kw in (dict(), dict(exposure=None), dict(exposure=False)):
        out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, images=images, photo_consistency=True, **kw)
        assert "exposure" not in out and "photo_consistency_raw" not in out and "photo_consistency" in out
    assert "lvba_photo_add_images" in looked_up and "lvba_photo_finish" in looked_up         # the real photo module did run
    assert "global-lvba_amd.expo" not in sys.modules
    PH.photo_consistency(np.zeros((4, 3), np.float32), images, np.zeros((2, 3, 3)), np.zeros((2, 3)), np.ones(8), 640, 512, gains=None)
    with pytest.raises(ValueError, match="photo_consistency"):
        pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, images=images, exposure=True)


def test_run_full_pipeline_report_keys(monkeypatch):
    """exposure=dict(...) goes to pipeline.photo_consistency as its `exposure` keyword; the output holds the compensated
    summaries, the raw ones and the report"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    visual = dict(Rcw=np.ones((2, 3, 3)), tcw=np.ones((2, 3)), Rcw_before=np.zeros((2, 3, 3)), tcw_before=np.zeros((2, 3)))
    after, before = (np.ones((4, 3), np.float32), np.zeros((4, 3), np.uint8)), (np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8))
    calls = []
    report = dict(gains=eo.identity(2), gains_float=np.zeros((2, 3, 2)), status=np.zeros(2, np.int32), status_names=["OK", "OK"],
                  mean_sigma=[3.0, 2.0, 1.5, 1.2], rounds=[], options=dict(eo.DEFAULTS))

    def fake(scans, scan_times, image_times, images, intr, width, height, after, before, points_after, points_before, **kw):
        calls.append(kw)
        return dict(after=dict(_one(points_after, 1.0), summary_raw=dict(n_points=4, mean_sigma=3.0)),
                    before=dict(_one(points_before, 2.0), summary_raw=dict(n_points=5, mean_sigma=4.0)), exposure=report)

    monkeypatch.setattr(pl, "Scans", _FakeScans)
    monkeypatch.setattr(pl, "run_visual_ba_with_lidar_assist", lambda *a, **k: dict(visual))
    monkeypatch.setattr(pl, "colorize_maps", lambda *a, **k: dict(after=after, before=before))
    monkeypatch.setattr(pl, "_photo_consistency", fake)
    out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, images=np.zeros((2, 512, 640, 3), np.uint8), photo_consistency=True,
                               exposure=dict(rounds=2, gate=0))
    assert calls[0]["exposure"] == dict(rounds=2, gate=0)
    assert out["photo_consistency"] == dict(after=dict(n_points=4, mean_sigma=1.0), before=dict(n_points=5, mean_sigma=2.0))
    assert out["photo_consistency_raw"] == dict(after=dict(n_points=4, mean_sigma=3.0), before=dict(n_points=5, mean_sigma=4.0))
    assert out["exposure"] is report and out["fused_after"][0] is after[0]
    out = pl.run_full_pipeline(*ARGS, enable_lidar_ba=False, images=np.zeros((2, 512, 640, 3), np.uint8), photo_consistency=True, exposure=True)
    assert calls[1]["exposure"] is True


def test_photo_consistency_applies_the_after_gains_to_both_sets(monkeypatch):
    """pipeline.photo_consistency: the gains are estimated once, on the `after` set, and both sets are evaluated raw and with them"""
    pl = importlib.import_module("global-lvba_amd.pipeline")
    PH = importlib.import_module("global-lvba_amd.photo")
    EX = importlib.import_module("global-lvba_amd.expo")
    gains = eo.identity(2) + 5
    calls, est = [], []

    class FakeDepth:
        def __enter__(self):
            return self

        def __exit__(self, *e):
            pass

    def evaluate(points, images, Rcw, tcw, intr, width, height, depth=None, chunk=16, device=0, gains=None, **opts):
        calls.append((len(points), gains, opts))
        return _one(points, 1.0 if gains is not None else 9.0)

    def estimate(points, images, Rcw, tcw, intr, width, height, **kw):
        est.append((len(points), kw))
        return dict(gains=gains, mean_sigma=[9.0, 1.0])

    monkeypatch.setattr(pl.V.DepthImages, "render", staticmethod(lambda *a, **k: FakeDepth()))
    monkeypatch.setattr(PH, "photo_consistency", evaluate)
    monkeypatch.setattr(EX, "estimate_exposure", estimate)
    cams = (np.zeros((1, 12)), np.zeros((2, 3, 3)), np.zeros((2, 3)))
    out = pl.photo_consistency(_FakeScans(), np.zeros(1), np.zeros(2), np.zeros((2, 8, 8, 3), np.uint8), np.ones(8), 8, 8, after=cams, before=cams,
                               points_after=np.zeros((4, 3), np.float32), points_before=np.zeros((5, 3), np.float32), min_views=3,
                               exposure=dict(rounds=2))
    assert [(n, g is not None) for n, g, _ in calls] == [(4, False), (4, True), (5, False), (5, True)]
    assert calls[1][1] is gains and calls[3][1] is gains and all(o == dict(min_views=3) for _, _, o in calls)
    assert len(est) == 1 and est[0][0] == 4 and est[0][1]["rounds"] == 2 and est[0][1]["min_views"] == 3
    assert out["exposure"]["gains"] is gains
    for name in ("after", "before"):
        assert out[name]["summary"]["mean_sigma"] == 1.0 and out[name]["summary_raw"]["mean_sigma"] == 9.0


def test_run_dataset_hands_the_keyword_on_and_writes_the_report(tmp_path, monkeypatch):
    pl = importlib.import_module("global-lvba_amd.pipeline")
    ds = importlib.import_module("global-lvba_amd.dataset")
    (tmp_path / "all_pcd_body").mkdir(); (tmp_path / "all_image").mkdir()
    rng = np.random.default_rng(0)
    for t in (0.5, 1.5):
        ds.save_pcd(str(tmp_path / "all_pcd_body" / f"{t}.pcd"), rng.normal(size=(10, 4)).astype(np.float32))
        (tmp_path / "all_image" / f"{t}.png").write_bytes(b"")
    (tmp_path / "all_pcd_body" / "lidar_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    (tmp_path / "all_image" / "image_poses.txt").write_text("0.5 0 0 0 0 0 0 1\n1.5 1 0 0 0 0 0 1\n")
    con = sqlite3.connect(str(tmp_path / "db.db"))
    con.execute("CREATE TABLE images (image_id INTEGER PRIMARY KEY, name TEXT)")
    con.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    con.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY, rows INTEGER, cols INTEGER, data BLOB)")
    kp = rng.uniform(0, 500, (6, 4)).astype(np.float32)
    for iid, name in ((1, "0.500000.png"), (2, "1.500000.png")):
        con.execute("INSERT INTO images VALUES (?, ?)", (iid, name))
        con.execute("INSERT INTO keypoints VALUES (?, ?, ?, ?)", (iid, 6, 4, kp.tobytes()))
    con.execute("INSERT INTO two_view_geometries VALUES (?, ?, ?, ?)",
                (ds.image_ids_to_pair_id(1, 2), 2, 2, np.array([[0, 1], [2, 3]], np.uint32).tobytes()))
    con.commit(); con.close()
    summary = dict(n_points=4, n_seen=3, n_valid=2, n_samples=7, mean_sigma=0.5, mean_views=7 / 3, ms=[0.1, 0.2, 0.3, 0.4])
    report = dict(gains=eo.identity(2), gains_float=np.zeros((2, 3, 2)), status=np.zeros(2, np.int32), status_names=["OK", "OK"],
                  mean_sigma=[3.0, 2.0, 1.5, 1.2], rounds=[dict(mean_sigma=3.0, rmse=np.zeros(2), n_used=np.zeros(2, np.int64),
                                                                max_gain_change=0.25, status=np.zeros(2, np.int32))],
                  sums=np.zeros((2, 20), np.uint64), options=dict(eo.DEFAULTS))
    calls = []

    def full_pipeline(*a, **k):
        calls.append(k)
        extra = {}
        if k.get("photo_consistency"):
            extra = dict(photo_consistency=dict(after=summary, before=dict(summary, mean_sigma=0.75)), photo_options=dict(po.DEFAULTS))
        if k.get("exposure"):
            extra.update(exposure=report, photo_consistency_raw=dict(after=dict(summary, mean_sigma=5.0), before=dict(summary, mean_sigma=6.0)))
        return dict(extra, poses=np.tile(np.r_[np.eye(3).reshape(9), 0, 0, 0], (2, 1)))

    monkeypatch.setattr(pl, "run_full_pipeline", full_pipeline)
    args = (str(tmp_path), "db.db", np.ones(8), 640, 512, np.eye(3), np.zeros(3))
    out_dir = tmp_path / "out"
    pl.run_dataset(*args, out_dir=str(out_dir), photo_consistency=True)
    assert "exposure" not in calls[0] and not (out_dir / "exposure.json").exists()
    assert sorted(json.load(open(out_dir / "photo_consistency.json"))) == ["after", "before", "options"]
    pl.run_dataset(*args, out_dir=str(out_dir), photo_consistency=True, exposure=dict(rounds=2))
    assert calls[1]["exposure"] == dict(rounds=2) and callable(calls[1]["images"])
    rep = json.load(open(out_dir / "exposure.json"))
    assert sorted(rep) == sorted(["gains", "gains_float", "status", "status_names", "mean_sigma", "rounds", "sums", "options"])
    assert rep["gains"] == eo.identity(2).tolist() and rep["mean_sigma"] == [3.0, 2.0, 1.5, 1.2] and rep["options"] == eo.DEFAULTS
    assert sorted(rep["rounds"][0]) == sorted(["mean_sigma", "rmse", "n_used", "max_gain_change", "status"])
    pcj = json.load(open(out_dir / "photo_consistency.json"))
    assert sorted(pcj) == ["after", "before", "options", "raw"] and pcj["raw"]["after"]["mean_sigma"] == 5.0 and pcj["after"]["mean_sigma"] == 0.5
