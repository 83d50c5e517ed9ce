"""Times the LiDAR map colouriser (lvba_colorize_*) on tools/fusion_bench.py's scene: 64 frames x 100 k points, 1280 x 1024
images, one image per frame, thinning at 0.01 m.  Prints one JSON line: ms per image per cloud (wall, upload included) and
the device split among upload, projection, sort, walk, compaction and thinning.  With --ref, also the reference's own
VisualizeOptComparison (both clouds, one thread) where oracle/_ref is present.

    usage: colorize_bench.py [frames] [pts] [--reps N]"""
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("global-lvba_amd")
synth = importlib.import_module("global-lvba_amd.synth")
col = importlib.import_module("global-lvba_amd.colorize")

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
frames = int(argv[0]) if len(argv) > 0 else 64
ppf = int(argv[1]) if len(argv) > 1 else 100000
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
W, H = 1280, 1024
intr = np.array([646.78472, 646.65775, 313.456795 * 2, 261.399612 * 2, -0.076160, 0.123001, -0.00113, 0.000251])
RCB = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
s = synth.make_scans(frames, ppf, room=(30, 20, 6), n_panels=0, n_blobs=0, clutter_frac=0.0, rot_sigma_deg=0.0, trans_sigma=0.0)
poses = np.asarray(s["poses_gt"], np.float64).reshape(-1, 12)
times = 100.0 + 0.1 * np.arange(frames)
Rcw = np.array([RCB @ T[:9].reshape(3, 3).T for T in poses])
tcw = np.array([-R @ T[9:] for R, T in zip(Rcw, poses)])
images = np.random.default_rng(1).integers(0, 256, (frames, H, W, 3), dtype=np.uint8)
res = dict(frames=frames, pts_per_frame=ppf, images=frames, width=W, height=H, leaf=0.01)
with pkg.Scans(s["clouds"]) as scans:
    best = None
    for rep in range(reps + 1):                              # the first run warms the pool and the kernels up
        t0 = time.perf_counter()
        with col.ColorMap(scans, poses, times, intr, W, H) as cm:
            t1 = time.perf_counter()
            cm.add_images(times, Rcw, tcw, images)
            t2 = time.perf_counter()
            n = cm.count()
            prof = cm.profile()
        if rep and (best is None or t2 - t1 < best[1]):
            best = (t1 - t0, t2 - t1, prof, n)
    create_s, add_s, prof, n = best
    res.update(points=n, create_ms=1e3 * create_s, add_images_ms=1e3 * add_s, ms_per_image_per_cloud=1e3 * add_s / frames,
               device_ms_per_image={k: v / frames for k, v in prof.items()})
print(json.dumps(res))
