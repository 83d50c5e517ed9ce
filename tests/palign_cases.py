"""Fixture of the photometric-alignment tests (tests/test_palign_host.py on the CPU, tests/test_gpu_palign.py on the GPU): the room
of tests/photo_cases.py, both sizes, the reference = the planted colours, the cameras planted or turned about their centres
(photo_cases.turned, depth images re-rendered at the turned cameras).  Seeded; nothing is committed.

Fixture conditions (checked on the CPU, test_palign_host.py; conditions on inputs, not tolerances on the device): the colour
fusion's margins hold at every pose a GPU test linearises at -- the given poses of the parity tests and every pose the oracle's
iteration visits --, and every n_samples there is at least MIN_GAP away from min_samples."""
import functools

import numpy as np

import covis_cases as cc
import palign_oracle as pao
import photo_cases as pc

MIN_SAMPLES = 200                 # the default: the fixture's too
MIN_GAP = 10
TURN_SEED = 7
N = cc.N_CAMERAS
# the option sets of photo_cases.OPTION_SETS that apply (min_views belongs to the fusion's finish)
OPTION_SETS = tuple(kw for kw in pc.OPTION_SETS if "min_views" not in kw)
# the accepted cameras' worst error to the truth as the ORACLE leaves them (test_palign_host.py asserts them as upper bounds and
# prints the figures; DESIGN.md §10q quotes them); the issue's ceiling on them is BOUND_*
BOUND_ROT_DEG, BOUND_CENTRE_M = 0.1, 0.01
ORACLE_WORST = {   # (size, degrees, rounds): (rotation in degrees, centre in metres)
    (0, 0.5, 1): (0.034, 0.0027),
    (0, 2.0, 2): (0.035, 0.0028),
}


def reference(size):
    """(ref16 uint16 [4200, 3], valid uint8 [4200]): the planted colours in 1/256 grey level, rounded half up; every point valid"""
    s = pc.scene(size)
    return np.floor(s["colour"] * 256.0 + 0.5).astype(np.uint16), np.ones(len(s["points"]), np.uint8)


def poses(size, which):
    """(Rcw [18, 3, 3], tcw [18, 3], depth [18, H, W]) of "planted" or ("turned", degrees)"""
    s = pc.scene(size)
    if which == "planted":
        return np.ascontiguousarray(s["Rcw"][:N]), np.ascontiguousarray(s["tcw"][:N]), np.ascontiguousarray(s["depth"][:N])
    return pc.turned(size, which[1], TURN_SEED)


@functools.lru_cache(None)
def _linearized(size, which, key):
    s = pc.scene(size)
    with_depth, opts = pc.split(dict(key))
    ref16, valid = reference(size)
    R, t, depth = poses(size, which)
    return [pao.linearize(s["points"], ref16, valid, s["images"][j], depth[j] if with_depth else None, s["intr"], R[j], t[j], **opts)
            for j in range(N)]


def linearized(size, which, **kw):
    """the oracle's linearisation of the 18 cameras at the poses `which` under an option set: a list of dict(sums, abs_sums,
    n_samples, margins) (computed once; do not write into it)"""
    return _linearized(size, which, pc.key_of(kw))


def rerendered(size, Rcw, tcw):
    """the depth images at the cameras (Rcw, tcw), rendered analytically as photo_cases.turned renders them"""
    s = pc.scene(size)
    C = pc.centres(Rcw, tcw)
    return np.ascontiguousarray(np.stack([cc.analytic_depth(s["intr"], Rcw[k], C[k], s["W"], s["H"]) for k in range(len(Rcw))]))


@functools.lru_cache(None)
def _aligned(size, degrees, rounds, key):
    s = pc.scene(size)
    ref16, valid = reference(size)
    R, t, depth = pc.turned(size, degrees, TURN_SEED)
    out = []
    for _ in range(rounds):
        res = pao.align(s["points"], ref16, valid, s["images"][:N], depth, s["intr"], R, t, **dict(key))
        res["start"] = (R, t, depth)
        res["rot_err"], res["centre_err"] = pao.pose_errors(res["Rcw"], res["tcw"], s["Rcw"][:N], s["tcw"][:N])
        out.append(res)
        R, t = np.ascontiguousarray(res["Rcw"]), np.ascontiguousarray(res["tcw"])
        depth = rerendered(size, R, t)
    return out


def aligned(size, degrees, rounds=1, **kw):
    """the oracle's alignment of the 18 cameras turned by `degrees`, `rounds` rounds with the depth images re-rendered at the
    returned cameras in between: a list, per round, of palign_oracle.align's dict with start = (Rcw, tcw, depth) of the round and
    rot_err [18] (degrees), centre_err [18] (metres) to the planted cameras (computed once; do not write into it)"""
    return _aligned(size, degrees, rounds, pc.key_of(kw))


def spread(size, Rcw, tcw, depth):
    """the fusion's mean spread of the 18 cameras, on the oracle"""
    s = pc.scene(size)
    import photo_oracle as po
    return po.evaluate(s["points"], s["images"][:N], depth, s["intr"], Rcw, tcw)["summary"]["mean_sigma"]


def ramp_case():
    """photo_cases.pixel_edge_case's camera (R = I, t = 0, no distortion, fx = fy = 64, cx = cy = 32, a 65 x 65 image) with the ramp
    image b = x, g = y, r = x + y and points (X, Y, 1) whose pixels (u, v) = (64 X + 32, 64 Y + 32) are multiples of 1/2: every
    number below is dyadic with few bits, so the formulas hold in exact arithmetic and no sum rounds, in any order.
      c16 = 256 (u, v, u + v);  gu = (1, 0, 1), gv = (0, 1, 1);  Ju = (64, 0, -64 X), Jv = (0, 64, -64 Y)
      rows: b (-64 X Y, 64 + 64 X^2, -64 Y, 64, 0, -64 X);  g (-64 - 64 Y^2, 64 X Y, 64 X, 0, 64, -64 Y);  r = their sum
    The references are c16 + (128, 64, 256): residuals (-1/2, -1/4, -1).  dict(points, image [1, 65, 65, 3], intr, W, H, ref16,
    valid, inside bool [n], H [6, 6], g [6], cost, sum_sq, n_samples): the sums under the trivial loss."""
    W = H = 65
    intr = np.array([64.0, 64.0, 32.0, 32.0, 0, 0, 0, 0])
    axis = np.array([-0.5, 0.0, 0.5, 1.0, 7.5, 31.5, 32.0, 40.0, 63.0, 63.5, 64.0, 64.5])
    u, v = (q.ravel() for q in np.meshgrid(axis, axis))
    X, Y = (u - 32.0) / 64.0, (v - 32.0) / 64.0
    pts = np.stack([X, Y, np.ones_like(X)], 1).astype(np.float32)
    assert (pts[:, 0].astype(np.float64) == X).all() and (pts[:, 1].astype(np.float64) == Y).all()
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    image = np.stack([xx, yy, xx + yy], 2).astype(np.uint8)
    inside = (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
    c16 = 256.0 * np.stack([u, v, u + v], 1)
    ref16 = np.where(inside[:, None], c16 + np.array([128.0, 64.0, 256.0]), 0).astype(np.uint16)
    r = np.array([-0.5, -0.25, -1.0])
    Hm, g, n = np.zeros((6, 6)), np.zeros(6), 0
    for x, y in zip(X[inside], Y[inside]):
        Jb = np.array([-64 * x * y, 64 + 64 * x * x, -64 * y, 64, 0, -64 * x])
        Jg = np.array([-64 - 64 * y * y, 64 * x * y, 64 * x, 0, 64, -64 * y])
        for J, rk in zip((Jb, Jg, Jb + Jg), r):
            Hm += np.outer(J, J)
            g += J * rk
        n += 1
    return dict(points=np.ascontiguousarray(pts), image=np.ascontiguousarray(image[None]), intr=intr, W=W, H=H, ref16=ref16,
                valid=np.ones(len(pts), np.uint8), inside=inside, Hm=Hm, g=g, cost=0.5 * n * float((r * r).sum()),
                sum_sq=n * float((r * r).sum()), n_samples=n)
