"""Shared, seeded fixtures of the dynamic-point tests (tests/test_dynamic_host.py on the CPU, tests/test_gpu_dynamic.py and
tests/test_gpu_pipeline_dynamic.py on the GPU); the oracle's results are computed once per case and shared.

SCENE: a closed box room of 10 x 8 x 3 m; the sensor moves 0.5 m per frame along x at mid height, with yaw and roll; 8 frames;
one ray per cell of the frame's own 20 x 60 range image (6 degrees a cell), jittered inside the cell -- so every cell of every
dilated 3 x 3 neighbourhood holds a sample of the room, not only the centre; a cube 0.6 m wide moves 0.7 m per frame the other way,
2.5 m to the side of the path.  A point whose ray hits the cube first is "planted".

EDGE: frames of 63, 1, 64, 0, 65 and 257 points (the empty frame in the middle; workgroup chunks of 256 points end on and across
frame borders) under pure translations by dyadic numbers, so that a point can lie exactly on another frame's sensor axis; random
points from inside the minimum to beyond the maximum range and beyond the elevation range, plus points in column 0 and in column
n_cols - 1 (the halo wraps), in the bottom and top rows (the halo is clipped), 1e-6 inside and outside el_min / el_max, on the
sensor axis of frame 2 (rho = 0), below min_range, 1e-6 inside and outside max_range and far beyond it, and with NaN and inf
components.  (A point AT max_range to the bit would have margin 0 and break condition 1; 1e-6 either side is what the fixture has.
For the same reason the edge cases use free_ratio 0.45 and 0.3: with at most five voters n_free = ratio (n_free + n_support) has
no solution, whereas 0.5 ties whenever n_free = n_support -- an exact integer tie that no implementation can flip, but a margin
of 0.  The scene runs at the default 0.5; its planted points have n_free >= 5 against n_support <= 1.)

Conditions (asserted by tests/test_dynamic_host.py; a fixture that breaks one is re-seeded and the seed noted here):
  1. every margin of every case is >= 1e-9, so that the device's atan2 and sqrt cannot flip a decision and the GPU comparison
     leaves out no point;
  2. on the scene the oracle labels no wall, floor or ceiling point dynamic;
  3. on the scene the oracle labels at least nine of ten planted points dynamic, counting a planted point only if at least
     min_free other frames see through its position (their ray to it passes the cube of their own time by more than the tolerance).
Seeds: scene 11, edge 5 (the first tried; none failed).
Measured (oracle, scene, default tolerances, halo 1, min_free 3, free_ratio 0.5; printed by test_scene_meets_its_conditions and
written into DESIGN.md §10m): 34 planted points of 9 600, all 34 seen through by at least three other frames, all 34 labelled
dynamic (n_free 5 .. 7, n_support 0 or 1); of the 9 566 points of the room none is labelled, none has a single free vote; 6 415
points have at least one vote.  Smallest margin: 1.4e-7 on the scene, 6.8e-7 on the edge clouds."""
import functools

import numpy as np

import dynamic_oracle as do

PI = do.PI
SCENE_SEED, EDGE_SEED = 11, 5
ROOM = np.array([[-5.0, 5.0], [-4.0, 4.0], [0.0, 3.0]])
CUBE_HALF = 0.3
SCENE = dict(n_rows=20, n_cols=60)
EDGE = dict(n_rows=12, n_cols=16, max_range=8.0, window=0, free_ratio=0.45)
EDGE_SIZES = (63, 1, 64, 0, 65, 257)


def _rot(yaw, roll):
    cz, sz, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])


def _box_exit(o, d, lo, hi):
    """distance at which the ray o + t d leaves the box [lo, hi] it starts in"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
    return t.min(-1)


def _box_entry(o, d, lo, hi):
    """distance at which the ray enters the box from outside, inf when it misses"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    near, far = np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)
    return np.where((near <= far) & (far > 0) & (near > 0), near, np.inf)


def cube_center(k):
    return np.array([2.45 - 0.7 * k, 1.0, 1.5])


@functools.lru_cache(maxsize=None)
def scene(seed=SCENE_SEED, n_frames=8):
    """clouds (float32 [n, 3] per frame), poses [n_frames, 12], planted (bool per point, cloud order), the options"""
    rng = np.random.default_rng(seed)
    o = do.options(**SCENE)
    nr, nc = o["n_rows"], o["n_cols"]
    clouds, poses, planted = [], [], []
    for k in range(n_frames):
        R = _rot(0.12 * (k - 3.5) + 0.05 * rng.standard_normal(), 0.04 * np.sin(1.3 * k) + 0.01 * rng.standard_normal())
        t = np.array([-1.75 + 0.5 * k, -1.5 + 0.05 * rng.standard_normal(), 1.5 + 0.03 * rng.standard_normal()])
        i, j = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
        az = -PI + (j + 0.5 + 0.35 * rng.uniform(-1, 1, j.shape)) * (2.0 * PI / nc)
        el = o["el_min"] + (i + 0.5 + 0.35 * rng.uniform(-1, 1, i.shape)) * ((o["el_max"] - o["el_min"]) / nr)
        d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
        dw = d @ R.T
        t_room = _box_exit(t, dw, ROOM[:, 0], ROOM[:, 1])
        c = cube_center(k)
        t_cube = _box_entry(t, dw, c - CUBE_HALF, c + CUBE_HALF)
        hit = np.minimum(t_room, t_cube)
        clouds.append((d * hit[:, None]).astype(np.float32))
        poses.append(np.r_[R.reshape(-1), t])
        planted.append(t_cube < t_room)
    return dict(clouds=clouds, poses=np.array(poses), planted=np.concatenate(planted), opts=dict(SCENE))


def seen_through(sc, opts):
    """per point of the scene: the number of OTHER frames whose ray to the point's position passes their own cube by more than
    the tolerance, the position lying inside their elevation range"""
    o = do.options(**opts)
    n = len(sc["clouds"])
    out = []
    for f, c in enumerate(sc["clouds"]):
        w = do.world_points(c, sc["poses"][f])
        cnt = np.zeros(len(c), np.int64)
        for g in range(n):
            if g == f:
                continue
            og = sc["poses"][g][9:]
            v = w - og
            dist = np.linalg.norm(v, axis=1)
            q = do.to_body(w, sc["poses"][g])
            e = np.arctan2(q[:, 2], np.hypot(q[:, 0], q[:, 1]))
            cg = cube_center(g)
            t_cube = _box_entry(og, v / dist[:, None], cg - CUBE_HALF, cg + CUBE_HALF)
            cnt += (t_cube > dist + o["abs_tol"] + o["rel_tol"] * dist) & (e >= o["el_min"]) & (e < o["el_max"])
        out.append(cnt)
    return np.concatenate(out)


def edge_poses():
    return np.array([np.r_[np.eye(3).reshape(-1), 0.5 * k, 0.125 * k, 0.0] for k in range(len(EDGE_SIZES))])


@functools.lru_cache(maxsize=None)
def edge(seed=EDGE_SEED):
    rng = np.random.default_rng(seed)
    o = do.options(**EDGE)
    T = edge_poses()
    clouds = []
    for n in EDGE_SIZES:
        az, el, r = rng.uniform(-PI, PI, n), np.deg2rad(rng.uniform(-70, 70, n)), rng.uniform(0.3, 9.0, n)
        clouds.append(np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32))
    cw, ch = 2.0 * PI / o["n_cols"], (o["el_max"] - o["el_min"]) / o["n_rows"]

    def at(az, el, r):
        return [r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)]

    special = [at(-PI + 0.3 * cw, 0.1, 3.0), at(PI - 0.3 * cw, 0.1, 3.0), at(-PI + 0.4 * cw, -0.2, 2.0), at(PI - 0.4 * cw, -0.2, 5.0),
               at(0.2, o["el_min"] + 0.3 * ch, 3.0), at(0.2, o["el_max"] - 0.3 * ch, 3.0), at(-2.0, o["el_min"] + 0.4 * ch, 4.0),
               at(-2.0, o["el_max"] - 0.4 * ch, 2.5),
               at(1.0, o["el_min"] + 1e-6, 3.0), at(1.0, o["el_min"] - 1e-6, 3.0), at(1.0, o["el_max"] - 1e-6, 3.0),
               at(1.0, o["el_max"] + 1e-6, 3.0),
               list(T[2][9:] - T[5][9:] + np.array([0.0, 0.0, 2.0])), list(T[2][9:] - T[5][9:] + np.array([0.0, 0.0, -1.5])),
               at(0.7, 0.2, 0.3), at(0.7, 0.2, 8.0 * (1 + 1e-6)), at(0.7, 0.2, 8.0 * (1 - 1e-6)), at(0.7, 0.2, 20.0),
               [np.nan, 1.0, 0.5], [1.0, np.inf, 0.5], [1.0, 2.0, -np.inf], [np.nan, np.nan, np.nan]]
    clouds[5][:len(special)] = np.array(special, np.float32)
    clouds[4][:4] = np.array(special[:2] + special[4:6], np.float32)       # the wrap and the clipped rows in a second frame
    return dict(clouds=clouds, poses=T, opts=dict(EDGE), n_special=len(special))


# (name, fixture, frame_begin, n_frames, options on top of the fixture's)
CASES = (
    ("scene", "scene", 0, 8, {}),
    ("scene, window 2, halo 0", "scene", 0, 8, dict(window=2, halo=0)),
    ("edge, all frames (window 0)", "edge", 0, 6, {}),
    ("edge, window 1", "edge", 0, 6, dict(window=1, min_free=1)),
    ("edge, window 2 of 5 frames", "edge", 0, 5, dict(window=2, min_free=2)),
    ("edge, window 6 >= frames", "edge", 0, 6, dict(window=6)),
    ("edge, halo 0", "edge", 0, 6, dict(halo=0)),
    ("edge, halo 3", "edge", 0, 6, dict(halo=3)),
    ("edge, one frame", "edge", 5, 1, {}),
    ("edge, frame_begin 1", "edge", 1, 5, dict(window=2, min_free=2)),
    ("edge, min_free 1, ratio 0.3", "edge", 0, 6, dict(min_free=1, free_ratio=0.3)),
)


def fixture(name):
    return scene() if name == "scene" else edge()


@functools.lru_cache(maxsize=None)
def case(k):
    """clouds, poses (of the case's frames), frame_begin, n_frames, opts and ref = the oracle's result, computed once"""
    name, fx, fb, nf, extra = CASES[k]
    d = fixture(fx)
    opts = dict(d["opts"], **extra)
    poses = np.ascontiguousarray(d["poses"][fb:fb + nf])
    return dict(name=name, clouds=d["clouds"], poses=poses, frame_begin=fb, n_frames=nf, opts=opts,
                ref=do.labels(d["clouds"], poses, frame_begin=fb, n_frames=nf, **opts))
