"""Host-side mirror of the reference's top-level flow over the C-ABI: everything between "a dataset in memory" and "refined
LiDAR poses, camera poses and landmarks", with every compute step in liblvba_hip.so on the GPU.

    LvbaSystem::runFullPipeline               src/lvba_system.cpp:136-142   initFromDatasetIO -> runLidarBA -> visual stage
    LvbaSystem::runVisualBAWithLidarAssist    src/lvba_system.cpp:144-154   grid map, camera poses from the refined LiDAR
                                                                            poses, depth images, (features), tracks + fusion,
                                                                            optimizeCameraPoses
    LvbaSystem::updateCameraPosesFromLidar    src/lvba_system.cpp:412-446   T_cam_new = (T_opt T_orig^-1) cam_orig of the
                                                                            nearest scan in time
    camera extrinsics                         src/lvba_system.cpp:860-869   Rcw = Rci Rwi^T, tcw = -Rcw Pwi + tci
    anchor clouds + plane map of the visual stage  src/lvba_system.cpp:1453-1507

    LvbaSystem::VisualizeOptComparison        src/lvba_system.cpp:1932-2144 the LiDAR map coloured from the images, after and
                                                                            before the refinement (colorize_maps)

Key points and matches are inputs of run_full_pipeline -- from a COLMAP database through dataset.load_colmap_db, the reference's own
alternative (`loadFromColmapDB`), or from the images themselves through extract_image_features and match_image_pairs, this
project's reading of `extractAndMatchFeaturesGPU` (features.py, match.py; not pinned against SiftGPU).  Out of scope, as in
DESIGN.md: writing a COLMAP database, ROS publishing and the OpenCV overlays.
"""
from __future__ import annotations

import numpy as np

from . import visual as V
from .voxel import Scans

DEFAULTS = dict(                                   # config/config.yaml of the reference
    window_enable=True, window_size=20, anchor_leaf=0.01, use_rel=True,
    stage1_enable=True, stage_voxel_size=(1.0, 0.5), stage_eigen_ratio=((0.2,) * 4, (0.08,) * 4),
    obser_thr=3, min_view_angle_deg=8.0, reproj_mean_thr_px=3.0, depth_half_window_s=0.5, depth_voxel=0.5,
    sigma_px=0.5, sigma_plane=0.01,
    # robust losses of the visual stage: None (the reference's nullptr at src/lvba_system.cpp:1630, :1639) or a pair
    # (reprojection, plane) of VisualProblem.set_loss arguments -- REFERENCE_HUBER is the pair the reference builds at :1585-1586
    visual_loss=None,
    colorize_half_window_s=0.5, colorize_leaf=0.01)       # VisualizeOptComparison: :1974, filter_size_points3D
REFERENCE_HUBER = (("huber", 1.0), ("huber", 0.1))


def _mat(T):
    T = np.asarray(T, np.float64).reshape(-1, 12)
    return T[:, :9].reshape(-1, 3, 3), T[:, 9:]


def update_camera_poses_from_lidar(x_opt, x_orig, scan_times, image_times, cam_orig):
    """src/lvba_system.cpp:412-446.  Poses are [n,12] (R row-major, p), T_world<-imu.  For every image the scan nearest in
    time (std::lower_bound, the previous one if it is strictly closer) gives T_delta = T_opt T_orig^-1; the image pose
    becomes T_delta o cam_orig."""
    Ro, po = _mat(x_opt)
    Rb, pb = _mat(x_orig)
    Rc, pc = _mat(cam_orig)
    ts = np.asarray(scan_times, np.float64)
    out = np.zeros((len(Rc), 12))
    for i, t in enumerate(np.asarray(image_times, np.float64)):
        it = int(np.searchsorted(ts, t, side="left"))
        idx = len(ts) - 1 if it == len(ts) else it
        if 0 < it < len(ts) and abs(ts[idx - 1] - t) < abs(ts[idx] - t):
            idx -= 1
        if idx >= len(Ro) or idx >= len(Rb):
            out[i, :9], out[i, 9:] = Rc[i].reshape(-1), pc[i]
            continue
        Rd = Ro[idx] @ Rb[idx].T                                            # T_opt * T_orig.inverse()
        pd = po[idx] - Rd @ pb[idx]
        out[i, :9] = (Rd @ Rc[i]).reshape(-1)
        out[i, 9:] = Rd @ pc[i] + pd
    return out


def camera_from_imu(T_wi, Rci, tci):
    """Rcw = Rci Rwi^T, tcw = -Rcw Pwi + tci (src/lvba_system.cpp:860-861)."""
    R, p = _mat(T_wi)
    Rci, tci = np.asarray(Rci, np.float64).reshape(3, 3), np.asarray(tci, np.float64).reshape(3)
    Rcw = np.einsum("ij,nkj->nik", Rci, R)
    tcw = -np.einsum("nij,nj->ni", Rcw, p) + tci
    return Rcw, tcw


def lidar_camera_priors(cam_poses, Rci, tci, sigma_rot, sigma_pos, relative=False):
    """Camera pose priors (VisualProblem.set_priors) that tie the visual stage to the LiDAR trajectory.  cam_poses [m,12]: the
    pose T_world<-imu the LiDAR trajectory gives every image (update_camera_poses_from_lidar).  relative=False: one POSE prior
    per camera; relative=True: one RELATIVE prior per pair of consecutive cameras (the trajectory's shape, free to move as a
    whole).  Every prior carries the extrinsic O = T_cam<-imu = (Rci, tci) as offset, so that what it constrains,
    T_world<-cam O, is the IMU pose and the measurement is the LiDAR pose itself (or the relative pose of two of them).
    sigma_rot [rad] / sigma_pos [m]: scalars or 3-vectors."""
    from .balm import Prior
    R, p = _mat(cam_poses)
    O = np.r_[np.asarray(Rci, np.float64).reshape(9), np.asarray(tci, np.float64).reshape(3)]
    if not relative:
        return [Prior.pose(k, np.r_[R[k].reshape(9), p[k]], sigma_rot, sigma_pos, offset=O) for k in range(len(R))]
    out = []
    for k in range(len(R) - 1):
        Rij = R[k].T @ R[k + 1]
        out.append(Prior.relative(k, k + 1, np.r_[Rij.reshape(9), R[k].T @ (p[k + 1] - p[k])], sigma_rot, sigma_pos, offset_i=O,
                                  offset_j=O))
    return out


def rot_to_quat_wxyz(R):
    """Eigen::Quaterniond(R).normalize() as [w, x, y, z] (src/lvba_system.cpp:1514-1517)."""
    from .dataset import rot_to_quat
    return np.array([rot_to_quat(r) for r in np.asarray(R).reshape(-1, 3, 3)])


def quat_wxyz_to_rot(q):
    from .dataset import quat_to_rot
    return np.array([quat_to_rot(*qq) for qq in np.asarray(q).reshape(-1, 4)])


def match_graph(n_keypoints, pairs, matches):
    """Adjacency of the key point match graph as BuildTracksAndFuse3D builds it (src/lvba_system.cpp:932-952): pairs visited in
    pairIndex order (i < j, i-major), every match appended to both ends' lists.  adj[i] = {key point: [(image, key point), ..]}."""
    N = len(n_keypoints)
    adj = [dict() for _ in range(N)]
    todo = []
    for (i, j), m in zip(pairs, matches):
        m = np.asarray(m, np.int64).reshape(-1, 2)
        if i > j:
            i, j, m = j, i, m[:, ::-1]
        todo.append((i, j, m))
    todo.sort(key=lambda q: (q[0], q[1]))
    for i, j, m in todo:
        for ki, kj in m:
            if ki < 0 or kj < 0 or ki >= n_keypoints[i] or kj >= n_keypoints[j]:
                continue
            adj[i].setdefault(int(ki), []).append((j, int(kj)))
            adj[j].setdefault(int(kj), []).append((i, int(ki)))
    return adj


def bfs_order(adj, start):
    """The BFS of :962-981 from `start` = (image, key point) over a whole connected component."""
    from collections import deque
    seen, comp, q = {start}, [], deque([start])
    while q:
        ci, ck = q.popleft()
        comp.append((ci, ck))
        for nb in adj[ci].get(ck, ()):
            if nb not in seen:
                seen.add(nb)
                q.append(nb)
    return comp


def match_components(n_keypoints, pairs, matches, obser_thr=3):
    """Connected components of the match graph that pass the two size checks (:983-1014: >= obser_thr observations from >=
    obser_thr images).  Returns (adj, comps); comps[c] = members sorted in scan order (image, key point): the reference starts
    its BFS at comps[c][0] and, if the fusion drops the component, again at comps[c][1], comps[c][2], ..."""
    adj = match_graph(n_keypoints, pairs, matches)
    seen = [set() for _ in adj]
    comps = []
    for i in range(len(adj)):
        for ki in sorted(adj[i]):
            if ki in seen[i]:
                continue
            comp = bfs_order(adj, (i, ki))
            for ci, ck in comp:
                seen[ci].add(ck)
            if len(comp) >= obser_thr and len({c for c, _ in comp}) >= obser_thr:
                comps.append(sorted(comp))
    return adj, comps


def build_components(n_keypoints, pairs, matches, obser_thr=3):
    """First-attempt BFS order of every component of match_components as CSR arrays (obs_off, obs_img, obs_kp)."""
    adj, comps = match_components(n_keypoints, pairs, matches, obser_thr)
    off, img, kp = [0], [], []
    for members in comps:
        for ci, ck in bfs_order(adj, members[0]):
            img.append(ci); kp.append(ck)
        off.append(len(img))
    return np.asarray(off, np.int64), np.asarray(img, np.int32), np.asarray(kp, np.int32)


def build_components_device(n_keypoints, pairs, matches, obser_thr=3, device=0):
    """build_components with the graph, its components and the BFS orders made on the GPU (trackgraph.TrackGraph; DESIGN.md
    §10j): the same three arrays."""
    from . import trackgraph as TG
    with TG.TrackGraph([int(n) for n in n_keypoints], pairs, matches, obser_thr, device=device) as g:
        return g.orders()


def _csr_take(off, which):
    """positions of the entries of the CSR rows `which`, row after row, and the rows' lengths"""
    lens = (off[1:] - off[:-1])[which]
    first = np.repeat(off[:-1][which] - (np.cumsum(lens) - lens), lens)
    return first + np.arange(int(lens.sum()), dtype=np.int64), lens


def _tracks_on_device(keypoints, pairs, matches, fuse_fn, obser_thr, device=0):
    """build_tracks_and_fuse(device_tracks=True): the graph is built once on the device, every round's orders come from
    TrackGraph.orders(pending, attempt, uv=True); the bookkeeping is numpy on whole arrays."""
    from . import trackgraph as TG
    rounds = []                                     # per round, of its accepted components: dict of arrays
    with TG.TrackGraph(keypoints, pairs, matches, obser_thr, device=device) as g:
        sizes = np.diff(g.components()[0])
        comp_status = np.zeros(len(sizes), np.uint8)
        pending, attempt = np.arange(len(sizes), dtype=np.int64), 0
        while len(pending):
            off, img, kp, uv = g.orders(pending, attempt, uv=True)
            status, X, err, kept = fuse_fn(off, img, uv)
            status = np.asarray(status)
            ok = status != 0
            comp_status[pending[ok]] = status[ok]
            if ok.any():
                won = np.flatnonzero(ok)
                obs, lens = _csr_take(off, won)
                rounds.append(dict(start_img=img[off[:-1][won]], start_kp=kp[off[:-1][won]], lens=lens, img=img[obs], kp=kp[obs], uv=uv[obs],
                                   kept=np.asarray(kept)[obs], X=np.asarray(X, np.float64).reshape(-1, 3)[won], err=np.asarray(err, np.float64)[won],
                                   status=status[won], attempts=np.full(len(won), attempt, np.int32)))
            pending = pending[~ok & (attempt + 1 < sizes[pending])]
            attempt += 1

    def cat(key, empty):
        return np.concatenate([r[key] for r in rounds]) if rounds else empty
    lens = cat("lens", np.zeros(0, np.int64))
    by_start = np.lexsort((cat("start_kp", np.zeros(0, np.int32)), cat("start_img", np.zeros(0, np.int32))))   # the reference's order
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    obs, lens = _csr_take(off, by_start)
    return dict(obs_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), obs_img=cat("img", np.zeros(0, np.int32))[obs],
                obs_kp=cat("kp", np.zeros(0, np.int32))[obs], obs_uv=cat("uv", np.zeros((0, 2), np.float32))[obs],
                kept=cat("kept", np.zeros(0, np.uint8))[obs].astype(np.uint8), X=cat("X", np.zeros((0, 3)))[by_start],
                err=cat("err", np.zeros(0))[by_start], status=cat("status", np.zeros(0, np.uint8))[by_start].astype(np.uint8),
                attempts=cat("attempts", np.zeros(0, np.int32))[by_start], component_status=comp_status)


def build_tracks_and_fuse(keypoints, pairs, matches, fuse_fn, obser_thr=3, device_tracks=False):
    """The track loop of BuildTracksAndFuse3D (src/lvba_system.cpp:954-1246) with the per-component fusion batched:
    fuse_fn(obs_off, obs_img, obs_uv) -> (status, X, err, kept) is lvba_fuse_tracks on the GPU.  A component the fusion drops is
    released by the reference (:1197, :1203) and met again at its next member in scan order, i.e. fused again in another BFS
    order; round r of the loop below fuses, in one batch, the r-th attempt of every component that is still dropped.  Tracks
    come out in the reference's order (by the key point their successful BFS started from).
    Returns dict(obs_off, obs_img, obs_kp, obs_uv, kept: CSR arrays of the tracks; X, err, status: per track; component_status:
    per component (0 = dropped after all attempts), attempts: per track, 0-based).
    device_tracks=True: the match graph, its components and every round's BFS orders are made on the GPU instead
    of by the Python mirror below; the returned dict is the same, key for key."""
    if device_tracks:
        return _tracks_on_device(keypoints, pairs, matches, fuse_fn, obser_thr)
    nk = [len(k) for k in keypoints]
    adj, comps = match_components(nk, pairs, matches, obser_thr)
    comp_status = np.zeros(len(comps), np.uint8)
    done = []                                                               # (start, order, X, err, status, kept, attempt)
    pending, attempt = list(range(len(comps))), 0
    while pending:
        orders = [bfs_order(adj, comps[c][attempt]) for c in pending]
        off = np.concatenate([[0], np.cumsum([len(o) for o in orders])]).astype(np.int64)
        flat = [ob for o in orders for ob in o]
        img = np.array([i for i, _ in flat], np.int32)
        uv = np.array([keypoints[i][k][:2] for i, k in flat], np.float32).reshape(-1, 2)
        status, X, err, kept = fuse_fn(off, img, uv)
        nxt = []
        for n, c in enumerate(pending):
            if status[n]:
                comp_status[c] = status[n]
                done.append((comps[c][attempt], orders[n], X[n].copy(), float(err[n]), int(status[n]),
                             np.asarray(kept[off[n]:off[n + 1]]).copy(), attempt))
            elif attempt + 1 < len(comps[c]):
                nxt.append(c)
        pending, attempt = nxt, attempt + 1
    done.sort(key=lambda d: d[0])
    off = np.concatenate([[0], np.cumsum([len(d[1]) for d in done])]).astype(np.int64)
    flat = [ob for d in done for ob in d[1]]
    img = np.array([i for i, _ in flat], np.int32)
    kp = np.array([k for _, k in flat], np.int32)
    uv = np.array([keypoints[i][k][:2] for i, k in flat], np.float32).reshape(-1, 2)
    return dict(obs_off=off, obs_img=img, obs_kp=kp, obs_uv=uv,
                kept=np.concatenate([d[5] for d in done]).astype(np.uint8) if done else np.zeros(0, np.uint8),
                X=np.array([d[2] for d in done]).reshape(-1, 3), err=np.array([d[3] for d in done]),
                status=np.array([d[4] for d in done], np.uint8), attempts=np.array([d[6] for d in done], np.int32),
                component_status=comp_status)


def run_visual_ba_with_lidar_assist(scans, x_opt, x_orig, scan_times, image_times, image_poses, Rci, tci, intr, width, height,
                                    keypoints, pairs, matches, camera_priors=None, depth=None, device_tracks=False, **cfg):
    """LvbaSystem::runVisualBAWithLidarAssist (src/lvba_system.cpp:144-154) from the refined LiDAR poses to the refined
    cameras.  scans: a voxel.Scans holding the raw clouds; keypoints[i] = [n_i, 2] float pixel coordinates; pairs / matches as
    build_tracks takes them.  cfg["visual_loss"]: see DEFAULTS.  camera_priors: None (the reference's problem), a list of
    balm.Prior objects on cameras, or a callable cam_poses -> list, called with the LiDAR-derived image poses [m,12]
    (T_world<-imu) that only exist inside this call (e.g. lambda cams: lidar_camera_priors(cams, Rci, tci, 1e-3, 0.02)).
    depth: None (the depth images are rendered here), or a visual.DepthImages already rendered with these arguments
    (as run_full_pipeline does under match_depth): it is used as it is and stays the caller's to close.
    device_tracks: build_tracks_and_fuse's (the track graph on the GPU; off by default).
    Returns a dict (cameras before / after, tracks, landmarks, planes, traces)."""
    c = dict(DEFAULTS); c.update(cfg)
    cam_new = update_camera_poses_from_lidar(x_opt, x_orig, scan_times, image_times, image_poses)      # poses_
    Rcw, tcw = camera_from_imu(cam_new, Rci, tci)                                                      # Rcw_all_optimized_
    Rcw0, tcw0 = camera_from_imu(image_poses, Rci, tci)                                                # Rcw_all_ (before)
    # generateDepthWithVoxel (+ buildGridMapFromOptimized)
    own_depth = depth is None
    if own_depth:
        depth = V.DepthImages.render(scans, x_opt, scan_times, image_times, Rcw, tcw, intr, width, height,
                                     half_window_s=c["depth_half_window_s"], voxel_size=c["depth_voxel"])
    try:
        # BuildTracksAndFuse3D
        T = build_tracks_and_fuse(keypoints, pairs, matches,
                                  lambda o, i, u: V.fuse_tracks(o, i, u, Rcw, tcw, intr, depth=depth, obser_thr=c["obser_thr"],
                                                                min_view_angle_deg=c["min_view_angle_deg"],
                                                                reproj_mean_thr_px=c["reproj_mean_thr_px"]), c["obser_thr"],
                                  device_tracks=device_tracks)
    finally:
        if own_depth:
            depth.close()
    off, img, uv, kept, X, err = T["obs_off"], T["obs_img"], T["obs_uv"], T["kept"], T["X"], T["err"]
    status = T["component_status"]
    tr = np.arange(len(X))                                                   # tracks_: every one is usable (:1436-1441)
    out = dict(cam_poses=cam_new, Rcw_before=Rcw0, tcw_before=tcw0, Rcw_lidar=Rcw, tcw_lidar=tcw, track_status=status,
               n_components=len(status), tracks=T)
    if len(tr) == 0:
        out.update(Rcw=Rcw, tcw=tcw, landmarks=np.zeros((0, 3)), landmark_valid=np.zeros(0, np.uint8), trace=[], termination="NO_TRACKS")
        return out
    # anchor clouds from the refined poses and the plane map of the visual stage (:1453-1507)
    m = scans.window_ba(x_opt, window_size=c["window_size"], anchor_leaf=c["anchor_leaf"], merge_only=True)
    try:
        with m["anchor_scans"].voxel_map(m["anchor_poses"], c["stage_voxel_size"][1], np.float32(c["stage_eigen_ratio"][1])) as vmap:
            plane, pvalid = vmap.find_planes(X[tr])
    finally:
        m["anchor_scans"].close()
    # inlier observations of the usable tracks, one residual per distinct observation (:1612-1634)
    o_off, o_cam, o_uv = [0], [], []
    for t in tr:
        a, b = int(off[t]), int(off[t + 1])
        sel = np.nonzero(kept[a:b])[0] + a
        o_cam.extend(img[sel].tolist()); o_uv.extend(uv[sel].astype(np.float64).tolist())
        o_off.append(len(o_cam))
    q0 = rot_to_quat_wxyz(Rcw)
    loss_r, loss_p = c["visual_loss"] if c["visual_loss"] is not None else (None, None)
    priors = camera_priors(cam_new) if callable(camera_priors) else camera_priors
    (q, t, Xn), trace, term, rc, valid = V.optimize_camera_poses(
        q0, tcw, X[tr], np.asarray(o_off, np.int64), np.asarray(o_cam, np.int32), np.asarray(o_uv, np.float64).reshape(-1, 2),
        plane[:, :3], plane[:, 3], intr, c["sigma_px"], c["sigma_plane"], loss_reproj=loss_r, loss_plane=loss_p,
        priors=priors)
    out.update(Rcw=quat_wxyz_to_rot(q), tcw=np.asarray(t), q=q, landmarks=np.asarray(Xn), landmarks_before=X[tr],
               landmark_valid=valid, track_ids=tr, plane=plane, plane_valid=pvalid, obs_off=np.asarray(o_off), obs_cam=np.asarray(o_cam),
               obs_uv=np.asarray(o_uv).reshape(-1, 2), trace=trace, termination=term, status=rc, mean_reproj=err[tr])
    return out


def colorize_maps(scans, image_times, images, intr, width, height, after, before=None, scan_times=None, half_window_s=0.5,
                  leaf_size=0.01, max_batch_images=0, chunk=16):
    """LvbaSystem::VisualizeOptComparison (src/lvba_system.cpp:1932-2144): the LiDAR map coloured from the images, thinned
    by down_sampling_voxel2(leaf_size).  scans: a voxel.Scans; images: [m,H,W,3] BGR uint8 or a callable k -> [H,W,3] (read in
    chunks of `chunk` images, each fed to both clouds); after / before = (scan_poses [n,12], Rcw [m,3,3], tcw [m,3]): the
    refined scan poses and cameras, and the original ones (x_buf_before_, Rcw_all_); before may be None.
    Returns {"after": (xyz, rgb), "before": (xyz, rgb)} (float32 [k,3], uint8 [k,3]), sorted by leaf key when thinned."""
    from .colorize import ColorMap
    if scan_times is None:
        raise ValueError("scan_times are required")
    sets = {"after": after} if before is None else {"after": after, "before": before}
    maps = {}
    try:
        for name, (x, _, _) in sets.items():
            maps[name] = ColorMap(scans, x, scan_times, intr, width, height, half_window_s=half_window_s, leaf_size=leaf_size,
                                  max_batch_images=max_batch_images)
        t = np.asarray(image_times, np.float64).reshape(-1)
        for a in range(0, len(t), max(1, int(chunk))):
            ks = range(a, min(len(t), a + max(1, int(chunk))))
            bgr = np.stack([np.asarray(images(k) if callable(images) else images[k], np.uint8) for k in ks])
            for name, (_, Rcw, tcw) in sets.items():
                Rcw, tcw = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
                maps[name].add_images(t[a:a + len(ks)], Rcw[a:a + len(ks)], tcw[a:a + len(ks)], bgr)
        return {name: m.download() for name, m in maps.items()}
    finally:
        for m in maps.values():
            m.close()


def map_quality(scans, after, before=None, **kw):
    """Mean map entropy / mean plane variance (mapq.map_quality_scans) of the scans at the refined poses `after` [n,12] and, when
    given, at the original ones `before`: {"after": summary, "before": summary or None}.  kw: radius, min_neighbors,
    query_stride, per_point.  A sharper map has the lower mme."""
    from .mapq import map_quality_scans
    return {"after": map_quality_scans(scans, after, **kw),
            "before": None if before is None else map_quality_scans(scans, before, **kw)}


def photo_consistency(scans, scan_times, image_times, images, intr, width, height, after, before=None, points_after=None,
                      points_before=None, exposure=None, **opts):
    """Multi-view colour fusion and photometric consistency (photo.photo_consistency) of the points points_after
    under the pose set after = (scan_poses [n,12], Rcw [m,3,3], tcw [m,3]), as for colorize_maps, and of points_before under
    `before` when both are given.  For each set the depth images are rendered at that set's scan poses and cameras
    (DepthImages.render: the occlusion test), that set's points are evaluated against all images (an array or a callable k ->
    [H,W,3], read in chunks), and what was opened is closed.  opts: photo.photo_opts' options, and depth_half_window_s, depth_voxel
    and chunk (DEFAULTS' values and 16).  Returns {"after": dict(summary, n_views, rgb, sigma, options), "before": ... or None}.
    The spread summary["mean_sigma"] drops when cameras, extrinsic and trajectory agree with the images.
    exposure: None (off: nothing of the stage is launched, its module is not imported and no entry point of it is called), True,
    or a dict of expo.estimate_exposure's keywords (rounds, expo.expo_opts' options): per-image exposure gains
    are estimated on the `after` set and applied to the `after` and the `before` evaluation alike -- a different compensation
    must not fake a change of spread.  Each set's dict then is the compensated evaluation and also holds "summary_raw", the
    summary without compensation, and the result holds "exposure", estimate_exposure's report."""
    from .photo import photo_consistency as evaluate
    half, voxel = opts.pop("depth_half_window_s", DEFAULTS["depth_half_window_s"]), opts.pop("depth_voxel", DEFAULTS["depth_voxel"])
    chunk = opts.pop("chunk", 16)
    out = {"after": None, "before": None}
    gains = None
    for name, poses, points in (("after", after, points_after), ("before", before, points_before)):
        if poses is None or points is None:
            continue
        x, Rcw, tcw = poses
        with V.DepthImages.render(scans, x, scan_times, image_times, Rcw, tcw, intr, width, height, half_window_s=half,
                                  voxel_size=voxel) as depth:
            out[name] = evaluate(points, images, Rcw, tcw, intr, width, height, depth=depth, chunk=chunk, device=scans.device, **opts)
            if not exposure:
                continue
            if name == "after":
                from .expo import estimate_exposure
                kw = dict(exposure) if isinstance(exposure, dict) else {}
                for k in ("occlusion_rel", "occlusion_abs", "max_depth", "holes", "min_views"):      # the evaluation's own
                    if k in opts:
                        kw.setdefault(k, opts[k])
                out["exposure"] = estimate_exposure(points, images, Rcw, tcw, intr, width, height, depth=depth, chunk=chunk,
                                                    device=scans.device, **kw)
                gains = out["exposure"]["gains"]
            if gains is not None:
                raw = out[name]["summary"]
                out[name] = evaluate(points, images, Rcw, tcw, intr, width, height, depth=depth, chunk=chunk, device=scans.device,
                                     gains=gains, **opts)
                out[name]["summary_raw"] = raw
    return out


def align_cameras_photometric(points, images, cameras, depth, intr, width, height, rounds=1, min_views=2, render=None, chunk=16,
                              device=0, **opts):
    """Photometric camera alignment against the coloured map (palign.PhotoAligner): the colour-map optimisation of
    Zhou & Koltun in `rounds` rounds.  points [n,3]: the map's points; images: an array [m,H,W,3] or a callable k -> [H,W,3], read
    `chunk` at a time; cameras = (Rcw [m,3,3], tcw [m,3]); depth: a visual.DepthImages at those cameras (the caller's, left open)
    or None (no occlusion test).  Per round: (1) the colour fusion at the current cameras gives the integer sums and the spread;
    (2) the reference colours are the fused ones, points below min_views invalid; (3) every image is aligned against them;
    (4) the depth images are rendered again at the returned cameras by render(Rcw, tcw) -> DepthImages (None: the depth images
    stay as they came), closed here.  opts: palign.palign_opts' options.  Returns dict(Rcw, tcw, status [m] and status_names,
    iterations, accepted, n_samples, rmse_initial (at the cameras given, first round) and rmse (at the cameras returned, last
    round) [m] in grey levels, mean_sigma: the spread at the start of every round and at the cameras returned [rounds + 1],
    rounds: per round dict(status, rmse_initial, rmse, n_valid), options).  The reference of a round holds every image's own
    earlier sample, so a round's step falls short by about 1 / n_views: the rounds make up for it."""
    from .palign import STATUS, PhotoAligner, reference_from_sums
    from .photo import PhotoMap
    R = np.ascontiguousarray(cameras[0], np.float64).reshape(-1, 3, 3).copy()
    t = np.ascontiguousarray(cameras[1], np.float64).reshape(-1, 3).copy()
    M, step = len(R), max(int(chunk), 1)
    read = (lambda a, b: np.stack([np.asarray(images(k), np.uint8) for k in range(a, b)])) if callable(images) else (lambda a, b: images[a:b])
    occl = {k: opts[k] for k in ("occlusion_rel", "occlusion_abs", "max_depth", "holes") if k in opts}

    def fuse(d):
        """the fusion at the current cameras: (mean spread, (n_views, s1, s2))"""
        with PhotoMap(points, M, intr, width, height, depth=d, device=device, min_views=max(int(min_views), 2), **occl) as pm:
            for k0 in range(0, M, step):
                k1 = min(M, k0 + step)
                pm.add_images(k0, R[k0:k1], t[k0:k1], read(k0, k1))
            return pm.finish()["summary"]["mean_sigma"], pm.sums()

    out = dict(mean_sigma=[], rounds=[])
    own = None                                   # the depth images rendered here
    try:
        for rnd in range(max(int(rounds), 1)):
            d = own if own is not None else depth
            spread, sums = fuse(d)
            out["mean_sigma"].append(spread)
            ref16, valid = reference_from_sums(sums[0], sums[1], min_views)
            parts = []
            with PhotoAligner(points, ref16, valid, M, width, height, intr, depth=d, device=device, **opts) as pa:
                for k0 in range(0, M, step):
                    k1 = min(M, k0 + step)
                    parts.append(pa.align(k0, R[k0:k1], t[k0:k1], read(k0, k1)))
                out["options"] = dict(pa.options)
            res = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
            if rnd == 0:
                out["rmse_initial"] = res["rmse_initial"]
            R, t = np.ascontiguousarray(res["Rcw"]), np.ascontiguousarray(res["tcw"])
            out["rounds"].append(dict(status=res["status"], rmse_initial=res["rmse_initial"], rmse=res["rmse"], n_valid=int(valid.sum())))
            for k in ("status", "iterations", "accepted", "n_samples", "rmse", "cost", "information"):
                out[k] = res[k]
            if render is not None:
                if own is not None:
                    own.close()
                own = render(R, t)
        out["mean_sigma"].append(fuse(own if own is not None else depth)[0])
    finally:
        if own is not None:
            own.close()
    out["Rcw"], out["tcw"] = R, t
    out["status_names"] = [STATUS[int(v)] for v in out["status"]]
    return out


def remove_dynamic(scans, poses, **opts):
    """The scans without their moving objects: the points that other frames saw through at `poses` [n,12] are labelled
    (dynamic.dynamic_labels, opts its options) and dropped.  Returns (static Scans -- the caller closes it --, report): the report
    holds the summary (n_points, n_judged, n_dynamic, ms), per_frame = the dynamic points of every frame, and label, n_free,
    n_support per point in cloud order."""
    from .dynamic import dynamic_labels, static_scans
    report = dynamic_labels(scans, poses, **opts)
    frame = np.repeat(np.arange(scans.n_frames), np.asarray(scans.counts, np.int64))
    report["per_frame"] = np.bincount(frame[report["label"] != 0], minlength=scans.n_frames).astype(np.int64)
    return static_scans(scans, report["label"]), report


def registration_prior(i, j, pose_i, pose_j, information, rmse, status, sigma=None):
    """The balm.Prior.relative(i, j) a registration of frame j gives against reference frame i (loop_closure_prior has the
    derivation): measurement T_i^-1 T_j(registered), sqrt_info the upper Cholesky factor of M H M^T / sigma^2 with
    M = diag(I, R_i^T) and sigma = rmse unless given; a registration that ended neither converged nor at max_iterations, or whose
    information is not positive definite, constrains nothing (sqrt_info = 0)."""
    from .balm import Prior
    pose_i, Tj = np.asarray(pose_i, np.float64).reshape(12), np.asarray(pose_j, np.float64).reshape(12)
    Ri, pi = pose_i[:9].reshape(3, 3), pose_i[9:]
    meas = np.r_[(Ri.T @ Tj[:9].reshape(3, 3)).reshape(9), Ri.T @ (Tj[9:] - pi)]
    s2 = float(rmse) ** 2 if sigma is None else float(sigma) ** 2
    M = np.zeros((6, 6))
    M[:3, :3], M[3:, 3:] = np.eye(3), Ri.T
    info = M @ np.asarray(information, np.float64).reshape(6, 6) @ M.T / s2 if s2 > 0 and status in (0, 1) else np.zeros((6, 6))
    try:
        sqrt_info = np.linalg.cholesky(info).T
    except np.linalg.LinAlgError:
        sqrt_info = np.zeros((6, 6))   # a failed registration constrains nothing
    return Prior.relative(int(i), int(j), meas, sqrt_info=sqrt_info)


def loop_closure_prior(scans, poses, map_frames, query_frame, ref_frame=None, voxel_size=1.0, eigen_ratio_array=None, sigma=None,
                       **opts):
    """A relative pose constraint from a revisit: the map of the frames `map_frames` (a contiguous ascending run of frame
    indices) of `scans` at their current `poses` [n,12] is built, frame `query_frame` is registered against it from its current
    pose (VoxelMap.register, opts: its options) and the result becomes a balm.Prior.relative between `ref_frame` (a map frame;
    default the first) and the query frame.  Returns (prior, registration dict); the caller decides on status / rmse / inliers
    whether to use it.
    The measurement is T_ref^-1 T_query(registered).  The registration's information H is in the tangent (theta, t) of
    R <- R Exp(theta), t <- t + delta, which is the LiDAR BA's own retraction (prior_device.h:3); the prior's residual is
    r = [Log(Rm^T R_i^T R_j); R_i^T (p_j - p_i) - pm] (prior_device.h:7) and at r = 0, with identity offsets, its Jacobian to the
    query pose is dr / dd_j = M = diag(I, R_i^T) (prior_device.h:230-245), so the information of r is M H M^T.  It is divided by
    sigma^2, the variance of a point-to-plane distance in m^2 (default: the registration's rmse^2), to make 1/2 |L r|^2 the
    negative log-likelihood; sqrt_info is the upper Cholesky factor L, L^T L = M H M^T / sigma^2.
    eigen_ratio_array: default register.STRICT_RATIO (the reason is DESIGN.md §10c)."""
    from .register import STRICT_RATIO
    mf = [int(f) for f in map_frames]
    if not mf or mf != list(range(mf[0], mf[0] + len(mf))):
        raise ValueError("map_frames must be a contiguous ascending run of frame indices")
    i, j = (mf[0] if ref_frame is None else int(ref_frame)), int(query_frame)
    if i not in mf or j == i:
        raise ValueError("ref_frame must be one of map_frames and differ from query_frame")
    x = np.asarray(poses, np.float64).reshape(-1, 12)
    with scans.voxel_map(x[mf[0]:mf[0] + len(mf)], voxel_size, STRICT_RATIO if eigen_ratio_array is None else eigen_ratio_array,
                         frame_begin=mf[0], n_frames=len(mf)) as m:
        reg = m.register(scans, [j], x[j:j + 1], **opts)
    return registration_prior(i, j, x[i], reg["poses"][0], reg["information"][0], reg["rmse"][0], reg["status"][0], sigma), reg


def pose_correction(T0, T):
    """(rotation angle of R0^T R [rad], |t - t0| [m]) between a start pose and a registered one."""
    T0, T = np.asarray(T0, np.float64).reshape(12), np.asarray(T, np.float64).reshape(12)
    dR = T0[:9].reshape(3, 3).T @ T[:9].reshape(3, 3)
    return float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(T[9:] - T0[9:]))


def loop_acceptance(status, inliers, points, rmse, rot, trans, min_inlier_frac=0.3, max_rmse=None, max_rot=None, max_trans=None):
    """The acceptance rule of find_loop_closures on one registered candidate: (accepted, reason).  Accepted iff the registration
    converged, inliers >= min_inlier_frac * points, rmse <= max_rmse, and the correction from the start to the registered pose is
    within max_rot [rad] / max_trans [m] (each bound only when given).  reason: None, or the first clause that failed --
    "status", "inliers", "rmse", "correction"."""
    if int(status) != 0:
        return False, "status"
    if not inliers >= min_inlier_frac * points:
        return False, "inliers"
    if max_rmse is not None and not rmse <= max_rmse:
        return False, "rmse"
    if (max_rot is not None and not rot <= max_rot) or (max_trans is not None and not trans <= max_trans):
        return False, "correction"
    return True, None


def find_loop_closures(scans, poses, submap_size=10, voxel_size=1.0, eigen_ratio_array=None, radius=5.0, min_gap=50, max_per_frame=2,
                       query_stride=1, min_inlier_frac=0.3, max_rmse=None, max_rot=None, max_trans=None, sigma=None, method="pose",
                       place=None, consistency=None, **register_opts):
    """Loop closures of a trajectory, found and verified on the GPU: the submap set of all frames of `scans` at their current
    `poses` [n,12] is built in one pass (Scans.submaps, eigen ratios register.STRICT_RATIO by default: DESIGN.md §10c), the
    candidates (query frame, submap, reference frame ref) are found, and ALL candidates are registered in one call, each query
    frame from its start pose against its submap (SubmapSet.register, register_opts: its options).  A candidate is accepted by
    loop_acceptance.
    method: where the candidates and their start poses come from.
      "pose"        from the poses alone (register.loop_candidates: radius, min_gap, max_per_frame, query_stride); ref is the
                    submap's nearest frame and the start is the query's current pose.  Finds a revisit only while the drift is
                    below radius.
      "descriptor"  from the clouds alone (register.place_candidates: Scan Context descriptors; `place` is a dict
                    of its options, submap_size / min_gap / max_per_frame / query_stride are this function's own); ref is the
                    submap's most similar frame and the start is poses[ref] o (Rz(yaw), 0), the reference pose turned by the
                    yaw the descriptors give.  It does not depend on the query's current pose, however far that has drifted.
      "both"        the union; a (query, submap) found by both is kept once, with the pose-based ref and start.
    rot / trans, and hence the max_rot / max_trans bounds, are measured from the START pose to the registered one: for a
    descriptor candidate the jump from the query's drifted pose to the registered pose is the finding, not an error, while a
    large correction of the start says the registration wandered off.
    Returns (priors, report): priors = a balm.Prior.relative(ref, query) per accepted candidate, measurement and sqrt_info as
    loop_closure_prior builds them (registration_prior; sigma as there) -- a relative constraint from ref to the REGISTERED pose
    of the query, valid whatever the query's current pose; report = one dict per candidate, by (query, submap): query, submap,
    ref, method ("pose", "descriptor", or "both" for a pair that both found), distance and distance_kind ("metres" between the
    positions for a pose candidate, "descriptor" for the shift distance in [0, 1]), shift and yaw (None for a pose candidate),
    start, the registration's fields (pose, information, status, status_name, iterations, inliers, points, cost_first,
    cost_last, rmse, min_eigenvalue), rot / trans (the correction), accepted and reason (None when accepted).
    consistency: None (default: off, nothing more is launched and the report is as above), True, or a dict of
    register.closure_consistency's options: the candidates that loop_acceptance accepted are tested pairwise against the relative
    motion of `poses` between them and only the largest mutually consistent set found yields priors (consistent_closures,
    DESIGN.md §10f).  A candidate outside it gets accepted=False, reason="consistency"; every report entry gains `consistent`:
    True, False, or None for a candidate that was not accepted in the first place."""
    from .register import STRICT_RATIO, loop_candidates, place_candidates
    if method not in ("pose", "descriptor", "both"):
        raise ValueError(f"method {method!r}: one of 'pose', 'descriptor', 'both'")
    if place is not None and method == "pose":
        raise TypeError("place options are for method='descriptor' or 'both'")
    x = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    shared = dict(submap_size=submap_size, min_gap=min_gap, max_per_frame=max_per_frame, query_stride=query_stride)
    found = {}
    if method in ("descriptor", "both"):
        clash = set(place or {}) & set(shared)
        if clash:
            raise TypeError(f"place options {sorted(clash)} are arguments of find_loop_closures itself")
        if scans.n_frames != len(x):
            raise ValueError(f"{len(x)} poses for {scans.n_frames} frames")
        cand = place_candidates(scans, **shared, **(place or {}))
        for k in range(len(cand["query"])):
            ref, yaw = int(cand["ref"][k]), float(cand["yaw"][k])
            c, s = np.cos(yaw), np.sin(yaw)
            start = np.r_[(x[ref, :9].reshape(3, 3) @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])).reshape(9), x[ref, 9:]]
            found[(int(cand["query"][k]), int(cand["submap"][k]))] = dict(
                ref=ref, method="descriptor", distance=float(cand["distance"][k]), distance_kind="descriptor", shift=int(cand["shift"][k]),
                yaw=yaw, start=start)
    if method in ("pose", "both"):
        cand = loop_candidates(x, radius=radius, **shared)
        for k in range(len(cand["query"])):
            key = (int(cand["query"][k]), int(cand["submap"][k]))
            found[key] = dict(ref=int(cand["ref"][k]), method="both" if key in found else "pose", distance=float(cand["distance"][k]),
                              distance_kind="metres", shift=None, yaw=None, start=x[key[0]].copy())
    if consistency is not None and consistency is not True and not isinstance(consistency, dict):
        raise TypeError("consistency: None, True or a dict of closure_consistency's options")
    priors, report = [], []
    if not found:
        return priors, report
    keys = sorted(found)
    q, w = np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32)
    starts = np.stack([found[k]["start"] for k in keys])
    with scans.submaps(x, submap_size, voxel_size, STRICT_RATIO if eigen_ratio_array is None else eigen_ratio_array) as sm:
        reg = sm.register(scans, q, w, starts, **register_opts)
    for k, key in enumerate(keys):
        rot, trans = pose_correction(starts[k], reg["poses"][k])
        ok, why = loop_acceptance(reg["status"][k], reg["inliers"][k], reg["points"][k], reg["rmse"][k], rot, trans, min_inlier_frac,
                                  max_rmse, max_rot, max_trans)
        r = dict(query=key[0], submap=key[1], **found[key], pose=reg["poses"][k].copy(), information=reg["information"][k].copy(),
                 status_name=reg["status_name"][k], rot=rot, trans=trans, accepted=ok, reason=why)
        for f in ("status", "iterations", "inliers", "points"):
            r[f] = int(reg[f][k])
        for f in ("cost_first", "cost_last", "rmse", "min_eigenvalue"):
            r[f] = float(reg[f][k])
        report.append(r)
        if ok:
            priors.append(registration_prior(r["ref"], r["query"], x[r["ref"]], r["pose"], r["information"], r["rmse"], r["status"], sigma))
    if consistency is not None:
        priors, keep = consistent_closures(x, priors, device=getattr(scans, "device", 0), **(consistency if isinstance(consistency, dict) else {}))
        verdict = iter(keep)
        for r in report:
            r["consistent"] = bool(next(verdict)) if r["accepted"] else None
            if r["consistent"] is False:
                r["accepted"], r["reason"] = False, "consistency"
    return priors, report


def consistent_closures(poses, priors, device=0, **opts):
    """The loop closures among `priors` that agree with one another over the relative motion of the current `poses` [n,12]
    between them (register.closure_consistency; opts: its options): (kept priors, keep mask [len(priors)] of
    bool).  priors: balm.Prior.relative objects with identity offsets, as find_loop_closures returns them -- ValueError for any
    other.  A closure is tested with its earlier frame as ref, whichever way the prior names the two.  A per-candidate check
    (loop_acceptance) cannot tell a registration that converged well on the wrong place; a closure
    that contradicts the largest mutually consistent set can, and is voted out here."""
    from . import _lib as L
    from .register import closure_consistency
    identity = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    priors = list(priors)
    for k, p in enumerate(priors):
        if getattr(p, "kind", None) != L.PRIOR_KINDS["relative"]:
            raise ValueError(f"prior {k} is not a relative prior")
        for off in (p.offset_i, p.offset_j):
            if any(v != 0.0 for v in off) and list(off) != identity:
                raise ValueError(f"prior {k} has a body-frame offset: the cycle is between the frames themselves")
    # The cycle of two closures runs over the odometry from ref to ref and from query to query, so two closures that say the same
    # must name their frames in the same order: every closure goes in with its earlier frame as ref, (j, i, Z^-1) for (i, j, Z).
    ref, query, meas = [], [], np.zeros((len(priors), 12))
    for k, p in enumerate(priors):
        z = np.array(list(p.meas), np.float64)
        if p.i > p.j:
            R = z[:9].reshape(3, 3)
            z = np.r_[R.T.reshape(9), -(R.T @ z[9:])]
        ref.append(min(p.i, p.j)); query.append(max(p.i, p.j))
        meas[k] = z
    got = closure_consistency(poses, ref, query, meas, device=device, **opts)
    return [p for p, k in zip(priors, got["keep"]) if k], got["keep"]


def relax_trajectory(poses, priors, device=0, **opts):
    """Pose-graph relaxation of the trajectory `poses` [n,12] over its own odometry and the loop closures `priors`
    (posegraph.relax_pose_graph; opts: its options -- odom_sigma_rot / odom_sigma_pos per frame step, anchor,
    closure_loss, max_iter, rel_tol, ...).  The closures go in as they are: nothing is re-oriented, and nothing is refused that
    the library call accepts.  Returns relax_pose_graph's dict plus max_pose_change = (largest rotation [rad], largest position
    change [m]) of a pose.  A closure whose query has drifted by more than the voxel size couples no planes in the bundle
    adjustment; relaxed first, the two passes share voxels again and the same closures then serve as its priors."""
    from .posegraph import relax_pose_graph
    x = np.asarray(poses, np.float64).reshape(-1, 12)
    got = relax_pose_graph(x, priors, device=device, **opts)
    change = [pose_correction(a, b) for a, b in zip(x, got["poses"])]
    got["max_pose_change"] = (max(c[0] for c in change), max(c[1] for c in change))
    return got


def _relax_over(poses, closures, relax, device=0):
    """run_lidar_ba / run_full_pipeline: relax=True or a dict of relax_trajectory's options -> (poses, summary dict)"""
    got = relax_trajectory(poses, closures, device=device, **(dict(relax) if isinstance(relax, dict) else {}))
    return got["poses"], dict(report=got["report"], weights=[float(w) for w in got["weights"]],
                              max_pose_change=[float(v) for v in got["max_pose_change"]])


_map_quality = map_quality   # run_full_pipeline / run_dataset have a keyword of that name
_photo_consistency = photo_consistency
_align_cameras_photometric = align_cameras_photometric
_remove_dynamic = remove_dynamic


def _lidar_cfg(cfg):
    c = dict(DEFAULTS); c.update(cfg)
    return dict(window_enable=c["window_enable"], window_size=c["window_size"], anchor_leaf=c["anchor_leaf"], use_rel=c["use_rel"],
                stage1_enable=c["stage1_enable"], stage_voxel_size=c["stage_voxel_size"], stage_eigen_ratio=c["stage_eigen_ratio"])


def run_lidar_ba(scans, poses, priors=None, window_loss=None, stage_loss=None, host_driven=False, relax=None, **cfg):
    """LvbaSystem::runLidarBA (src/lvba_system.cpp:312-410) on resident scans: (poses [n,12], report dict).  cfg: the LiDAR keys of
    DEFAULTS.  window_loss / stage_loss: robust losses (BalmProblem.set_loss arguments) of every window problem / of both global
    stages; None: the plain sum of lambda_min.
    host_driven=False: the library's whole-stage entry (Scans.lidar_ba -> lvba_lidar_ba / _priors / _robust).
    host_driven=True: the same flow driven from here, stage by stage -- window BA, then per global stage a voxel map of the anchor
    clouds at the current anchor poses, its problem (tras_opt), set_loss, refine -- and the composition anchor o rel.  It takes a
    stage loss only (the window stage is one library call) and no priors.
    relax: None (default: nothing more is launched), True, or a dict of relax_trajectory's options: the trajectory is first relaxed
    over the relative priors among `priors` (the loop closures), the stages start from the relaxed poses with the same priors, and
    the report gains pose_graph.  Without a relative prior it does nothing."""
    k = _lidar_cfg(cfg)
    closures = [p for p in (priors or []) if getattr(p, "kind", None) == 2] if relax else []
    if closures:
        poses, summary = _relax_over(poses, closures, relax, device=getattr(scans, "device", 0))
        out, report = run_lidar_ba(scans, poses, priors=priors, window_loss=window_loss, stage_loss=stage_loss, host_driven=host_driven, **cfg)
        report = dict(report)
        report["pose_graph"] = summary
        return out, report
    if not host_driven:
        return scans.lidar_ba(poses, priors=priors, window_loss=window_loss, stage_loss=stage_loss, **k)
    if priors or window_loss is not None or not k["window_enable"]:
        raise ValueError("the host-driven flow takes a stage loss only, and needs the window stage")
    x = np.asarray(poses, np.float64).reshape(-1, 12)
    w = scans.window_ba(x, window_size=k["window_size"], voxel_size=k["stage_voxel_size"][0], anchor_leaf=k["anchor_leaf"],
                        use_rel=k["use_rel"])
    anchors, ax = w["anchor_scans"], w["anchor_poses"].copy()
    report = dict(n_anchors=len(ax), stage_ran=[0, 0], stage_iters=[0, 0])
    try:
        for s in range(0 if k["stage1_enable"] else 1, 2):
            if not len(ax):
                break
            with anchors.voxel_map(ax, k["stage_voxel_size"][s], k["stage_eigen_ratio"][s]) as m:
                if m.info["n_voxels"] == 0:
                    continue
                with m.tras_opt() as prob:
                    prob.set_loss(stage_loss)
                    ax, trace, _ = prob.refine(ax)
                    report["stage_ran"][s], report["stage_iters"][s] = 1, len(trace)
    finally:
        anchors.close()
    out = x.copy()
    for i, a in enumerate(w["anchor_index"]):
        if a < 0:
            continue
        A, Lr = ax[a], w["rel_poses"][i]
        R = A[:9].reshape(3, 3)
        out[i, :9] = (R @ Lr[:9].reshape(3, 3)).reshape(9)
        out[i, 9:] = R @ Lr[9:] + A[9:]
    return out, report


def match_image_pairs(descriptors, pairs, keypoints=None, Rcw=None, tcw=None, intr=None, device=0, depth=None, **opts):
    """Feature matches of image pairs from their descriptors (match.Matcher), in the form build_tracks and
    run_full_pipeline take: one int32 [m, 2] array per pair, in the order of `pairs`; a pair without matches gives an empty
    array, it is not dropped.  descriptors[i] = uint8 [n_i, 128].  Without geometry the matching is unguided (the reference's
    fallback, src/lvba_system.cpp:697-833: distance bound, ratio test, mutual best match); with keypoints, Rcw, tcw
    (T_cam<-world) and intr a candidate must also lie within max_epipolar_px of the epipolar line the poses give.  With depth (a
    visual.DepthImages rendered at those poses, one image per image) on top, the gate is a point instead of a line (guided=2): a
    keypoint with a depth return is a 3-D point, and a candidate must lie within max_reproj_px of its image in the other view
    -- which separates copies of a texture that lie along the epipolar line.  opts: max_distance, max_ratio, mutual, guided,
    max_epipolar_px, max_reproj_px."""
    from . import match as M
    return M.match_pairs(descriptors, pairs, keypoints=keypoints, intr=intr, Rcw=Rcw, tcw=tcw, device=device, depth=depth, **opts)


def extract_image_features(read_image, n_images, device=0, batch=32, **opts):
    """SIFT features of images 0 .. n_images - 1 on the GPU (features.extract; the rule is in include/lvba_hip.h):
    read_image(k) -> uint8 [h, w, 3] in B, G, R order or [h, w] grey, all of one size; `batch` images are read and handed to the
    device at a time.  Returns (keypoints, descriptors): per image float32 [n_i, 4] = (x, y, sigma, theta) and uint8 [n_i, 128],
    the form match_image_pairs takes.  opts: features.sift_opts' keywords."""
    from . import features as F
    kps, descs = [], []
    for k0 in range(0, int(n_images), max(1, int(batch))):
        imgs = [read_image(k) for k in range(k0, min(int(n_images), k0 + max(1, int(batch))))]
        kp, ds, _ = F.extract(imgs, device=device, **opts)
        kps += kp
        descs += ds
    return kps, descs


def verify_image_pairs(keypoints, pairs, matches, intr, Rcw=None, device=0, **opts):
    """Geometric verification of putative matches (verify.Verifier): per image pair an essential matrix by RANSAC
    on the GPU, all pairs in one grid, and the matches that agree with it.  matches: one [m, 2] array per pair, as
    match_image_pairs returns them.  Without Rcw the pose-free eight-point method (method=0; degenerate where the scene is one
    plane); with Rcw [M, 3, 3] (T_cam<-world rotations) and method=1 the rotation-aided two-point method, which trusts the relative
    rotation and nothing else.  opts: method, hypotheses, refine_rounds, min_inliers, max_error_px, seed, and model =
    "essential" (the default: the call as it was) | "homography" (four-point homography with a symmetric transfer test, the model
    of a scene that is one plane) | "auto" (both, per pair the homography where its count reaches planar_ratio, default 0.8, of
    the essential matrix's).  Returns (inlier_matches, report): one int32 [m, 2] array per pair in the order of `pairs` -- empty
    for a pair that fails, which is not dropped -- and a dict of arrays E, status, n_inliers, n_matches, best_h, and with a model
    other than "essential" kind, n_inliers_E, n_inliers_H."""
    from . import verify as VF
    return VF.verify_pairs(keypoints, pairs, matches, intr, Rcw=Rcw, device=device, **opts)


def correspondences_from_matches(pairs, matches, points):
    """The 2-D to 3-D correspondences the matches hold: for every image the (own keypoint, partner's lifted point) of every match
    whose partner has a point.  points: one [n_i, 3] array per image, NaN rows where a keypoint has no point (Matcher.points,
    resect.lift_keypoints).  Both directions of a pair are used; the order is the order of `pairs` -- within a pair its first
    image's side, then its second's -- then match order.  Returns (keypoint, world): per image an int32 [c_i] and a float64
    [c_i, 3] array."""
    M = len(points)
    kp, X = [[] for _ in range(M)], [[] for _ in range(M)]
    for (a, b), m in zip(pairs, matches):
        m = np.asarray(m, np.int64).reshape(-1, 2)
        for own, other, co, cp in ((int(a), int(b), 0, 1), (int(b), int(a), 1, 0)):
            P = np.asarray(points[other], np.float64).reshape(-1, 3)[m[:, cp]]
            has = ~np.isnan(P[:, 0])
            kp[own].append(m[has, co])
            X[own].append(P[has])
    return ([np.concatenate(k).astype(np.int32) if k else np.zeros(0, np.int32) for k in kp],
            [np.concatenate(x).reshape(-1, 3) if x else np.zeros((0, 3)) for x in X])


def check_cameras(keypoints, pairs, matches, depth, Rcw, tcw, intr, device=0, **opts):
    """Where the images say the cameras are (resect.resect_images): every keypoint with a depth return is lifted
    through its image's depth image (depth: a visual.DepthImages at the poses Rcw, tcw = T_cam<-world), the matches turn the
    lifted points of an image's partners into its 2-D to 3-D correspondences, and every image is resected from them alone, all
    in one grid.  Returns the report as plain Python: per image the status, the counts, the rmse and -- for an image that comes
    back OK -- the rotation angle (degrees) and the distance of the camera centres between the resected and the given pose; the
    medians of both; and poses = the resected [M, 12] (R row-major, t), zeros where not OK.  opts: resect.resect_opts'."""
    from . import resect as RS
    uv = [np.asarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    points = RS.lift_keypoints(depth, uv, intr, Rcw, tcw)
    kp, world = correspondences_from_matches(pairs, matches, points)
    _, report = RS.resect_images([u[k] for u, k in zip(uv, kp)], world, intr, device=device, **opts)
    out = RS.summary(report, Rcw, tcw)
    out["poses"] = np.concatenate([report["Rcw"].reshape(-1, 9), report["tcw"]], 1).tolist()
    return out


_check_cameras = check_cameras    # run_full_pipeline's keyword of the same name shadows the function there


def calibration_records_from_points(keypoints, pairs, matches, points, Rcw, tcw):
    """The records of calib.refine_extrinsic that the matches hold, from lifted points (one [n_i, 3] array per image, NaN rows
    where a keypoint has none, lifted at the poses Rcw, tcw = T_cam<-world): every match whose partner keypoint has a point is a
    record (own pixel, the partner's point in the partner's camera frame).  Both directions of a pair are used, in the order of
    correspondences_from_matches: the order of `pairs`, within a pair its first image's side, then its second's, then match order;
    every direction is a row of the directed pair table.  Returns (records, (img_a, img_b)): records = dict(pair int32 [n], uv
    float32 [n, 2], Xb float64 [n, 3]), img_a the image the pixel is in, img_b the image the point was lifted in."""
    Rcw, tcw = np.asarray(Rcw, np.float64).reshape(-1, 3, 3), np.asarray(tcw, np.float64).reshape(-1, 3)
    pr, uv, Xb, ia, ib = [], [], [], [], []
    for (a, b), m in zip(pairs, matches):
        m = np.asarray(m, np.int64).reshape(-1, 2)
        for own, other, co, cp in ((int(a), int(b), 0, 1), (int(b), int(a), 1, 0)):
            P = np.asarray(points[other], np.float64).reshape(-1, 3)[m[:, cp]]
            has = ~np.isnan(P[:, 0])
            pr.append(np.full(int(has.sum()), len(ia), np.int32))
            uv.append(np.asarray(keypoints[own], np.float32).reshape(-1, 2)[m[has, co]])
            Xb.append(P[has] @ Rcw[other].T + tcw[other])      # back into its source camera, with the pose it was lifted with
            ia.append(own); ib.append(other)
    records = dict(pair=np.concatenate(pr) if pr else np.zeros(0, np.int32),
                   uv=np.concatenate(uv).reshape(-1, 2) if uv else np.zeros((0, 2), np.float32),
                   Xb=np.concatenate(Xb).reshape(-1, 3) if Xb else np.zeros((0, 3)))
    return records, (np.asarray(ia, np.int32), np.asarray(ib, np.int32))


def calibration_records(keypoints, pairs, matches, depth, Rcw, tcw, intr):
    """calibration_records_from_points of the keypoints lifted through their images' depth images (resect.lift_keypoints; depth: a
    visual.DepthImages at the poses Rcw, tcw = T_cam<-world)."""
    from . import resect as RS
    uv = [np.asarray(k, np.float32).reshape(-1, 2) for k in keypoints]
    points = RS.lift_keypoints(depth, uv, intr, Rcw, tcw)
    return calibration_records_from_points(uv, pairs, matches, points, Rcw, tcw)


def body_twists(scan_poses, scan_times, image_times):
    """The twist of the body at every image time, for calib.refine_extrinsic_td: [M, 6] rows (om, v), om the body-frame angular
    velocity (rad/s), v the world-frame linear velocity (m/s), from the scan segment [k, k + 1] that brackets the image (the first
    or the last segment for an image outside the scans): om = log(R_k^T R_k+1) / dt, v = (P_k+1 - P_k) / dt.  scan_poses [n, 12]
    = T_world<-imu at scan_times (ascending)."""
    R, p = _mat(scan_poses)
    ts = np.asarray(scan_times, np.float64).reshape(-1)
    if len(ts) < 2 or len(ts) != len(R):
        raise ValueError("body_twists needs at least two scan poses and one time per pose")
    out = np.zeros((len(np.atleast_1d(image_times)), 6))
    for i, t in enumerate(np.asarray(image_times, np.float64).reshape(-1)):
        k = min(max(int(np.searchsorted(ts, t, side="right")) - 1, 0), len(ts) - 2)
        dt = ts[k + 1] - ts[k]
        if not dt > 0.0:
            raise ValueError(f"scan times {k} and {k + 1} do not ascend")
        E = R[k].T @ R[k + 1]
        th = np.arccos(np.clip(0.5 * (np.trace(E) - 1.0), -1.0, 1.0))
        w = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
        out[i, :3] = (w if th < 1e-9 else w * th / np.sin(th)) / dt
        out[i, 3:] = (p[k + 1] - p[k]) / dt
    return out


def calibrate_extrinsic(keypoints, pairs, matches, body_poses, Rci, tci, intr, depth=None, render=None, rounds=1, starts=None, device=0,
                        time_offset=False, twists=None, **opts):
    """What the extrinsic T_cam<-imu should be instead of (Rci, tci), from the matches and the LiDAR depths (calib.refine_extrinsic;
    DESIGN.md §10o).  body_poses [M, 12]: T_world<-imu at the image times (the LiDAR-derived image poses).  depth: a
    visual.DepthImages rendered at camera_from_imu(body_poses, Rci, tci), used by the first round and left to the caller; render:
    a callable (Rcw, tcw) -> visual.DepthImages, called where a round has no depth images (every round after the first: the depth
    under a keypoint was read through the old extrinsic, and that error is why rounds exist); what it returns is closed here.
    rounds: how many times records are built and the extrinsic solved, each from the last result; a round that does not come back
    converged or at its iteration limit ends the loop and its extrinsic is not taken.  starts, opts: calib.refine_extrinsic's.
    Returns calib.summary of the last round against the given extrinsic (Rci, tci there are the refined ones; rotation_deg and
    translation_m the total change) plus n_records and rounds = the summary of every round against its own start.
    time_offset=True (needs twists [M, 6], body_twists): the camera-LiDAR time offset td is refined with the extrinsic
    (calib.refine_extrinsic_td).  Every round lifts its records at camera_from_imu(calib.shift_poses(body_poses, twists, td), R, t)
    and calls the solver with the ORIGINAL poses and td0 = td, so the offset accumulates across rounds; the report's time_offset_s
    and std_td_s are then numbers, and time_offset_rounds lists td after every round.  Off (the default), no _td entry point is
    looked up and the report is what it always was, with time_offset_s = std_td_s = None."""
    from . import calib as CB
    if time_offset and twists is None:
        raise ValueError("calibrate_extrinsic(time_offset=True) needs twists (pipeline.body_twists)")
    R0, t0 = np.asarray(Rci, np.float64).reshape(3, 3), np.asarray(tci, np.float64).reshape(3)
    R, t, td = R0, t0, 0.0
    per, last, tds = [], None, []
    for k in range(max(1, int(rounds))):
        Rcw, tcw = camera_from_imu(CB.shift_poses(body_poses, twists, td) if time_offset else body_poses, R, t)
        dk = depth if k == 0 and depth is not None else None
        own = dk is None
        if own:
            if render is None:
                raise ValueError("calibrate_extrinsic needs depth images: depth for the first round, render for every other")
            dk = render(Rcw, tcw)
        try:
            records, table = calibration_records(keypoints, pairs, matches, dk, Rcw, tcw, intr)
        finally:
            if own:
                dk.close()
        if time_offset:
            Rn, tn, tdn, rep = CB.refine_extrinsic_td(records, table, body_poses, twists, intr, R, t, td, starts=starts if k == 0 else None,
                                                      device=device, **opts)
        else:
            Rn, tn, rep = CB.refine_extrinsic(records, table, body_poses, intr, R, t, starts=starts if k == 0 else None, device=device, **opts)
        per.append(dict(CB.summary(rep, R, t), n_records=int(len(records["pair"]))))
        if int(rep["status"]) not in (CB.CONVERGED, CB.MAX_ITERATIONS):
            if last is None:
                last = rep
            break
        R, t, last = Rn, tn, rep
        if time_offset:
            td = float(tdn)
            tds.append(td)
    out = CB.summary(dict(last, Rci=R, tci=t, **({"td": td} if time_offset else {})), R0, t0)
    out.update(n_records=per[-1]["n_records"], rounds=per)
    if time_offset:
        out["time_offset_rounds"] = tds
    return out


_calibrate_extrinsic = calibrate_extrinsic    # run_full_pipeline's keyword of the same name shadows the function there


def localize_images(query_keypoints, query_descriptors, map_keypoints, map_descriptors, map_points, intr, candidates=None, device=0,
                    match_opts=None, **opts):
    """Places images that were not part of the run into the map: each query image is matched unguided against its candidate map
    images (match.Matcher), a match whose map keypoint has a point (map_points: per map image [n_i, 3], NaN rows without one) is a
    2-D to 3-D correspondence, and every query image is resected from its correspondences (resect.resect_images).  candidates:
    per query image the map images to match against (None: all).  Returns (Rcw [Q, 3, 3], tcw [Q, 3], report): T_cam<-world of
    every query image (zeros where the status is not OK), and the report of resect.summary with, under "correspondences", per
    query image a dict of arrays keypoint, map_image, map_keypoint and inlier."""
    from . import match as M
    from . import resect as RS
    Q, n_map = len(query_descriptors), len(map_descriptors)
    cand = [list(range(n_map)) if candidates is None else [int(c) for c in candidates[q]] for q in range(Q)]
    pairs = [(n_map + q, c) for q in range(Q) for c in cand[q]]
    with M.Matcher(list(map_descriptors) + list(query_descriptors), device=device) as matcher:
        matches = matcher.match_pairs(pairs, **dict(match_opts or {}, guided=0)) if pairs else []
    uv, world, corr = [], [], []
    k = 0
    for q in range(Q):
        kq = np.asarray(query_keypoints[q], np.float32).reshape(-1, 2)
        rows = dict(keypoint=[], map_image=[], map_keypoint=[], world=[])
        for c in cand[q]:
            m = np.asarray(matches[k], np.int64).reshape(-1, 2)
            k += 1
            P = np.asarray(map_points[c], np.float64).reshape(-1, 3)[m[:, 1]]
            has = ~np.isnan(P[:, 0])
            rows["keypoint"].append(m[has, 0]); rows["map_keypoint"].append(m[has, 1]); rows["world"].append(P[has])
            rows["map_image"].append(np.full(int(has.sum()), c, np.int64))
        cat = {a: (np.concatenate(b) if b else np.zeros((0, 3) if a == "world" else 0, np.float64 if a == "world" else np.int64))
               for a, b in rows.items()}
        uv.append(kq[cat["keypoint"]]); world.append(cat["world"].reshape(-1, 3)); corr.append(cat)
    inliers, rep = RS.resect_images(uv, world, intr, device=device, **opts)
    report = RS.summary(rep)
    for q in range(Q):
        mask = np.zeros(len(uv[q]), bool)
        mask[inliers[q]] = True
        corr[q]["inlier"] = mask
    report["correspondences"] = corr
    return rep["Rcw"], rep["tcw"], report


def select_image_pairs(depth, Rcw, tcw, intr, sequential=0, **opts):
    """Which image pairs to match (covis.select_pairs) instead of all M (M - 1) / 2: the pairs in which one image
    sees enough of what the other sees, judged on a grid of samples lifted through the LiDAR depth images (a visual.DepthImages
    rendered at the poses Rcw, tcw = T_cam<-world), occlusion by the other view's depth image included.  sequential = k > 0 adds,
    on the host, every pair with |i - j| <= k: the neighbours in time of an image whose depth image is empty have no other way
    in.  opts: covis.covis_opts' (grid_x, grid_y, search_radius, occlusion, both_ways, max_per_image, min_shared, min_overlap,
    occlusion_rel, occlusion_abs).  Returns (pairs: a list of (i, j) with i < j, sorted; report: n_images, all_pairs, selected,
    covisible -- the selection before the sequential pairs --, and empty_images, those without a single sample)."""
    from . import covis as CV
    M = depth.n_images
    pairs, _, _ = CV.select_pairs(depth, Rcw, tcw, intr, **opts)
    # the images without a sample, from the lifted table alone: the lift kernel and M G 24 bytes back, a third of what a second
    # pass of the count kernel for n_points would take
    no_sample = np.isnan(CV.samples(depth, Rcw, tcw, intr, **opts)[:, :, 0]).all(axis=1)
    chosen = {(int(i), int(j)) for i, j in pairs}
    chosen |= {(i, j) for i in range(M) for j in range(i + 1, min(M, i + int(sequential) + 1))}
    report = dict(n_images=M, all_pairs=M * (M - 1) // 2, selected=len(chosen), covisible=len(pairs),
                  empty_images=[int(i) for i in np.flatnonzero(no_sample)])
    return sorted(chosen), report


def run_full_pipeline(clouds, poses, scan_times, image_times, image_poses, Rci, tci, intr, width, height, keypoints, pairs,
                      matches, enable_lidar_ba=True, enable_visual_ba=True, device=0, images=None, lidar_priors=None,
                      window_loss=None, stage_loss=None, camera_priors=None, map_quality=False, loop_closures=None, relax=None,
                      match_fn=None, match_depth=False, match_select=None, device_tracks=False, verify_matches=None,
                      remove_dynamic=None, check_cameras=None, calibrate_extrinsic=False, photo_consistency=None, photo_align=None,
                      exposure=None, **cfg):
    """LvbaSystem::runFullPipeline (src/lvba_system.cpp:136-142) on in-memory data: clouds = body-frame [n_i, >=3] float32
    arrays, poses [n,12] = x_buf_ (T_world<-imu), image_poses [m,12] the image poses from the odometry.  cfg: DEFAULTS' keys
    (visual_loss, colorize_leaf among them).  images: None, or the images ([m,H,W,3] BGR uint8 or a callable k -> [H,W,3]):
    then the output also holds colored_after / colored_before = (xyz, rgb), the LiDAR map coloured from them
    (colorize_maps) with the refined poses and cameras and with the original ones; this needs the visual stage.
    lidar_priors: balm.Prior objects on frames (GNSS fixes, loop closures, ...) for the global stages of the LiDAR BA
    (Scans.lidar_ba(priors=...)).  window_loss / stage_loss: robust losses of the LiDAR BA (run_lidar_ba).  camera_priors:
    priors on the cameras of the visual stage (run_visual_ba_with_lidar_assist; None: none).  map_quality: True, or a dict of
    mapq.map_quality_scans' keywords: the output also holds map_quality = {"after": ..., "before": ...}, the mean map entropy and
    mean plane variance of the scans at the refined and at the original poses (off by default: nothing is launched).
    loop_closures: None (off: nothing is launched), True, or a dict of find_loop_closures' keywords: loop closures are detected on
    the input poses before the LiDAR stage, the accepted priors are appended to lidar_priors and the output holds
    loop_closures = the report.  With consistency=True (or a dict of options) among the keywords the accepted closures are vetted
    against one another first (consistent_closures) and only the mutually consistent ones become priors.
    relax: None (off), True, or a dict of relax_trajectory's options; honoured only together with loop_closures: after the closures
    are found (and vetted), the trajectory is relaxed over them, the LiDAR stage starts from the relaxed poses with the same
    closures as priors, and the output holds pose_graph = dict(report, weights, max_pose_change).  poses_before stays the input.
    match_fn: None (pairs and matches are the caller's), or a callable cam_poses -> (pairs, matches), called after the LiDAR stage
    with the LiDAR-derived image poses [m,12] (T_world<-imu): the matches are then made against the refined poses (guided
    matching, match_image_pairs) and replace the arguments; the output holds pairs / matches as used.
    match_depth: False, or True (only with match_fn): the depth images of the visual stage are rendered once, at the LiDAR-refined
    poses, before the matching; match_fn is called as match_fn(cam_poses, depth=depth) (depth-guided matching: hand it on to
    match_image_pairs) and the visual stage uses the same images, which are closed here.
    match_select: None (off), True, or a dict of select_image_pairs' keywords (only with match_fn): the depth images are rendered
    once as under match_depth, the image pairs to match are selected from them (select_image_pairs), match_fn is called with
    pairs=selected (and depth=depth when match_depth is set), and the output holds pair_selection, the report.
    device_tracks: False, or True: the visual stage builds its tracks on the GPU (run_visual_ba_with_lidar_assist's device_tracks).
    verify_matches: None (off: nothing is launched), True, or a dict of verify_image_pairs' options: the matches actually used --
    the caller's or match_fn's -- are verified geometrically immediately before the visual stage and only the inliers go on (a
    pair that fails keeps its place with no matches).  Here the method defaults to 1, the rotation-aided one: the rotations are
    those of camera_from_imu of the camera poses in force at that point (the LiDAR-derived ones), and the scenes a LiDAR sees are
    mostly walls and floors, where the pose-free eight-point method (method=0, which uses no pose at all) is degenerate.  The output holds pairs / matches as used and match_verification: per pair
    the status and the counts, plus the totals.  dict(model="auto") or dict(model="homography") (verify_image_pairs) adds each
    pair's model and the two models' counts to it, and n_pairs_planar; without `model` none of these fields appear.
    remove_dynamic: None (off: nothing is launched), True, or a dict of dynamic.dynamic_labels' options: after the LiDAR stage the
    points that other frames saw through at the refined poses -- whatever moved while the data was recorded -- are labelled
    (pipeline.remove_dynamic) and the coloured maps and the map quality are made from the static scans, `before` as well as `after`,
    so that the two compare the same points; the output holds dynamic = the report.  The LiDAR stage, the depth images and the
    visual stage keep using the full scans.
    check_cameras: None (off: nothing is launched and no entry point of the stage is called), True, or a dict of resect.resect_opts' options: once
    the matches in force are final -- after the verification where that is on -- every image is resected from the LiDAR points its
    matches reach (pipeline.check_cameras) at the LiDAR-derived camera poses, through the depth images of match_depth /
    match_select or images rendered the same way; the output holds camera_check, per image how far the pose the images ask for
    lies from the one the trajectory and the extrinsic give.  Nothing downstream reads it.
    calibrate_extrinsic: False (off: nothing is launched and no entry point of the stage is called), True, "apply", or a dict of
    pipeline.calibrate_extrinsic's keywords (rounds, starts, calib.calib_opts' options; time_offset=True refines the camera-LiDAR
    time offset too, with the twists of the refined LiDAR trajectory (body_twists) unless twists are given, and with apply and a
    converged result the visual stage gets the image poses shifted by it: poses_shifted in the report) with an optional apply=True: once the
    matches in force are final, the extrinsic is refined from them and the LiDAR depths (pipeline.calibrate_extrinsic) at the
    LiDAR-derived image poses, and the output holds extrinsic, the report.  True reports only: nothing downstream reads it.
    "apply": the visual stage -- camera poses, depth images, track fusion, the start of the BA, the colours -- runs with the
    refined extrinsic instead of (Rci, tci), when the refinement converged; it needs depth images from the matching stage
    (match_depth or match_select), which are closed before the visual stage renders its own at the new extrinsic.
    photo_consistency: None (off: nothing is launched and no entry point of the stage is called), True, or a dict of
    pipeline.photo_consistency's options; it needs `images` (ValueError without them).  The points of colored_after are projected
    into every image that sees them at the refined scan poses and cameras, those of colored_before at the original ones, each set
    with the occlusion test against depth images rendered for it; the output holds photo_consistency = {"after": summary,
    "before": summary} -- mean_sigma is the spread of the colours across the views, lower where cameras, extrinsic and trajectory
    agree with the images -- and fused_after / fused_before = (xyz, rgb, n_views, sigma) on the points of colored_after /
    colored_before.  With remove_dynamic these are the static scans' coloured maps, as for the other map products.  The images
    are read a second time, after the colouring: the points do not exist before the colouring is done.
    photo_align: None (off: nothing is launched, no entry point of the stage is called and its module is not imported), True,
    "apply", or a dict of pipeline.align_cameras_photometric's keywords (rounds, min_views, palign.palign_opts' options) with an
    optional apply=True; it needs `images`.  The refined cameras are aligned photometrically against the points of colored_after
    (depth images rendered at the refined scan poses and cameras, and again after every round), and the output holds photo_align,
    the report (without the per-image information matrices), and photo_align_cameras = (Rcw, tcw).  True reports only.  "apply":
    the `after` set of photo_consistency -- fused_after and its summary -- is evaluated at the aligned cameras; everything else
    stays as it is (the coloured maps keep the colours of the refined cameras: their points are what the alignment is made
    against).
    exposure: None (off: nothing is launched, the stage's module is not imported and no lvba_expo_* entry point is called), True,
    or a dict of expo.estimate_exposure's keywords; only together with photo_consistency (ValueError without it).  Per-image
    exposure gains are estimated on the `after` set and applied to both evaluations (pipeline.photo_consistency's exposure); the
    output's photo_consistency and fused_after / fused_before are then the compensated ones, photo_consistency_raw =
    {"after": summary, "before": summary} are the summaries without compensation, and exposure is the report."""
    if exposure and not photo_consistency:
        raise ValueError("exposure compensates the photometric consistency: it needs photo_consistency=...")
    if photo_consistency and images is None:
        raise ValueError("photo_consistency samples the images: it needs images=...")
    if photo_align and images is None:
        raise ValueError("photo_align samples the images: it needs images=...")
    if verify_matches and not enable_visual_ba:
        raise ValueError("verify_matches verifies the matches of the visual stage (enable_visual_ba=True)")
    if images is not None and not enable_visual_ba:
        raise ValueError("colouring the map needs the cameras of the visual stage (enable_visual_ba=True)")
    if match_select and (match_fn is None or not enable_visual_ba):
        raise ValueError("match_select selects the pairs that match_fn is handed before the visual stage: it needs match_fn and "
                         "enable_visual_ba=True")
    c = dict(DEFAULTS); c.update(cfg)
    x_orig = np.asarray(poses, np.float64).reshape(-1, 12).copy()
    out = dict(poses_before=x_orig)
    with Scans(clouds, device=device) as scans:
        x_opt = x_orig
        if loop_closures:
            found, out["loop_closures"] = find_loop_closures(scans, x_orig, **(dict(loop_closures) if isinstance(loop_closures, dict) else {}))
            lidar_priors = list(lidar_priors or []) + found if found or lidar_priors is not None else None
            if relax and found:
                x_opt, out["pose_graph"] = _relax_over(x_orig, found, relax, device=device)
        if enable_lidar_ba:
            x_opt, report = run_lidar_ba(scans, x_opt, priors=lidar_priors, window_loss=window_loss, stage_loss=stage_loss, **c)
            out["lidar_report"] = report
        out["poses"] = np.asarray(x_opt).reshape(-1, 12)
        depth = None
        try:
            if enable_visual_ba and match_fn is not None:
                cam_poses = update_camera_poses_from_lidar(out["poses"], x_orig, scan_times, image_times, image_poses)
                kw = {}
                if match_depth or match_select:
                    Rcw, tcw = camera_from_imu(cam_poses, Rci, tci)
                    depth = V.DepthImages.render(scans, out["poses"], scan_times, image_times, Rcw, tcw, intr, width, height,
                                                 half_window_s=c["depth_half_window_s"], voxel_size=c["depth_voxel"])
                    if match_select:
                        kw["pairs"], out["pair_selection"] = select_image_pairs(
                            depth, Rcw, tcw, intr, **(dict(match_select) if isinstance(match_select, dict) else {}))
                    if match_depth:
                        kw["depth"] = depth
                pairs, matches = match_fn(cam_poses, **kw)
                out["pairs"], out["matches"] = pairs, matches
            if enable_visual_ba and verify_matches:
                from . import verify as VF
                vo = dict(verify_matches) if isinstance(verify_matches, dict) else {}
                vo.setdefault("method", VF.KNOWN_ROTATION)   # here the rotations exist, and LiDAR scenes are walls and floors
                Rv = None
                if int(vo["method"]) == VF.KNOWN_ROTATION:
                    Rv, _ = camera_from_imu(update_camera_poses_from_lidar(out["poses"], x_orig, scan_times, image_times, image_poses),
                                            Rci, tci)
                matches, vrep = verify_image_pairs(keypoints, pairs, matches, intr, Rcw=Rv, device=device, **vo)
                out["pairs"], out["matches"] = pairs, matches
                out["match_verification"] = VF.summary(pairs, vrep)
            if check_cameras:
                Rk, tk = camera_from_imu(update_camera_poses_from_lidar(out["poses"], x_orig, scan_times, image_times, image_poses), Rci, tci)
                dk = depth if depth is not None else V.DepthImages.render(scans, out["poses"], scan_times, image_times, Rk, tk, intr, width,
                                                                          height, half_window_s=c["depth_half_window_s"],
                                                                          voxel_size=c["depth_voxel"])
                try:
                    out["camera_check"] = _check_cameras(keypoints, pairs, matches, dk, Rk, tk, intr, device=device,
                                                         **(dict(check_cameras) if isinstance(check_cameras, dict) else {}))
                finally:
                    if dk is not depth:
                        dk.close()
            x_orig_v, image_poses_v = x_orig, image_poses    # what the visual stage derives its image poses from
            if calibrate_extrinsic:
                ce = dict(calibrate_extrinsic) if isinstance(calibrate_extrinsic, dict) else {}
                apply = bool(ce.pop("apply", False)) or calibrate_extrinsic == "apply"
                if apply and depth is None:
                    raise ValueError("calibrate_extrinsic='apply' needs the matches and depth images of match_depth or match_select")
                cam_k = update_camera_poses_from_lidar(out["poses"], x_orig, scan_times, image_times, image_poses)
                if ce.get("time_offset") and ce.get("twists") is None:
                    ce["twists"] = body_twists(out["poses"], scan_times, image_times)   # of the refined LiDAR trajectory
                out["extrinsic"] = _calibrate_extrinsic(
                    keypoints, pairs, matches, cam_k, Rci, tci, intr, depth=depth, device=device,
                    render=lambda Rk, tk: V.DepthImages.render(scans, out["poses"], scan_times, image_times, Rk, tk, intr, width, height,
                                                               half_window_s=c["depth_half_window_s"], voxel_size=c["depth_voxel"]), **ce)
                out["extrinsic"]["applied"] = bool(apply and out["extrinsic"]["status"] == "converged")
                if out["extrinsic"]["applied"]:
                    Rci, tci = np.array(out["extrinsic"]["Rci"]), np.array(out["extrinsic"]["tci"])
                    depth.close()            # rendered at the old extrinsic: the visual stage renders its own
                    depth = None
                if ce.get("time_offset"):
                    out["extrinsic"]["poses_shifted"] = out["extrinsic"]["applied"]
                    if out["extrinsic"]["applied"]:
                        # the image poses the later stages get are the ones at t + td, handed on as they are: x_orig = the refined
                        # scans makes update_camera_poses_from_lidar the identity
                        from . import calib as CB
                        image_poses_v = CB.shift_poses(cam_k, ce["twists"], out["extrinsic"]["time_offset_s"])
                        x_orig_v = out["poses"]
            if enable_visual_ba:
                out["visual"] = run_visual_ba_with_lidar_assist(scans, out["poses"], x_orig_v, scan_times, image_times, image_poses_v, Rci,
                                                                tci, intr, width, height, keypoints, pairs, matches,
                                                                camera_priors=camera_priors, **({"depth": depth} if depth is not None else {}),
                                                                **({"device_tracks": True} if device_tracks else {}), **c)
        finally:
            if depth is not None:
                depth.close()
        static = None
        if remove_dynamic:
            static, out["dynamic"] = _remove_dynamic(scans, out["poses"], **(dict(remove_dynamic) if isinstance(remove_dynamic, dict) else {}))
        try:
            _map_products(static if static is not None else scans, out, x_orig, scan_times, image_times, images, intr, width, height,
                          map_quality, c, photo_consistency, photo_align, exposure)
        finally:
            if static is not None:
                static.close()
    return out


def _photo_align(scans, out, scan_times, image_times, images, intr, width, height, c, photo_align):
    """run_full_pipeline's photo_align: the report into out, and the cameras the `after` set of the photometric consistency uses"""
    kw = dict(photo_align) if isinstance(photo_align, dict) else {}
    apply = bool(kw.pop("apply", False)) or photo_align == "apply"
    v = out["visual"]
    render = lambda Rk, tk: V.DepthImages.render(scans, out["poses"], scan_times, image_times, Rk, tk, intr, width, height,
                                                 half_window_s=c["depth_half_window_s"], voxel_size=c["depth_voxel"])
    with render(v["Rcw"], v["tcw"]) as depth:
        rep = _align_cameras_photometric(out["colored_after"][0], images, (v["Rcw"], v["tcw"]), depth, intr, width, height, render=render,
                                         device=scans.device, **kw)
    out["photo_align_cameras"] = (rep.pop("Rcw"), rep.pop("tcw"))
    rep.pop("information")
    rep["applied"] = apply
    out["photo_align"] = rep
    return out["photo_align_cameras"] if apply else (v["Rcw"], v["tcw"])


def _map_products(scans, out, x_orig, scan_times, image_times, images, intr, width, height, map_quality, c, photo=None, photo_align=None,
                  exposure=None):
    """run_full_pipeline's products made from every point of `scans`: the coloured maps, the photometric alignment, the photometric
    consistency and the map quality"""
    if images is not None:
        v = out["visual"]
        col = colorize_maps(scans, image_times, images, intr, width, height, after=(out["poses"], v["Rcw"], v["tcw"]),
                            before=(x_orig, v["Rcw_before"], v["tcw_before"]), scan_times=scan_times,
                            half_window_s=c["colorize_half_window_s"], leaf_size=c["colorize_leaf"])
        out["colored_after"], out["colored_before"] = col["after"], col["before"]
    if photo_align:
        Rcw_after, tcw_after = _photo_align(scans, out, scan_times, image_times, images, intr, width, height, c, photo_align)
    elif images is not None:
        Rcw_after, tcw_after = v["Rcw"], v["tcw"]
    if photo:
        kw = dict(photo) if isinstance(photo, dict) else {}
        kw.setdefault("depth_half_window_s", c["depth_half_window_s"])
        kw.setdefault("depth_voxel", c["depth_voxel"])
        pc = _photo_consistency(scans, scan_times, image_times, images, intr, width, height,
                                after=(out["poses"], Rcw_after, tcw_after), before=(x_orig, v["Rcw_before"], v["tcw_before"]),
                                points_after=out["colored_after"][0], points_before=out["colored_before"][0],
                                **({"exposure": exposure} if exposure else {}), **kw)
        if exposure:
            out["exposure"] = pc.pop("exposure")
            out["photo_consistency_raw"] = {k: dict(q["summary_raw"]) for k, q in pc.items()}
        out["photo_consistency"] = {k: dict(q["summary"]) for k, q in pc.items()}
        out["photo_options"] = dict(pc["after"]["options"])
        for k, q in pc.items():
            out["fused_" + k] = (out["colored_" + k][0], q["rgb"], q["n_views"], q["sigma"])
    if map_quality:
        kw = dict(map_quality) if isinstance(map_quality, dict) else {}
        out["map_quality"] = _map_quality(scans, out["poses"], x_orig, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# The same flow from a dataset directory in the reference's on-disk layout (README.md "Dataset", src/dataset_io.cpp):
#     <data_path>/all_pcd_body/lidar_poses.txt + <timestamp>.pcd      TUM poses (T_world<-imu) + body-frame scans
#     <data_path>/all_image/image_poses.txt + <timestamp>.png         TUM poses of the images + the images (only their names are read)
#     <data_path>/<colmap_db_path>                                    keypoints + inlier matches (loadFromColmapDB)
# ---------------------------------------------------------------------------------------------------------------------
UNDISTORT_FORMATS = ("jpg", "png")


def export_undistorted(out_dir, images, n, intr, width, height, gains=None, format="jpg", quality=95, chunk=16, device=0, **opts):
    """The images the rows of images.txt name (the reference's Colmap/images/k.jpg, src/lvba_system.cpp:2029), undistorted on the
    GPU (undistort.undistort_images): out_dir/images/<k>.<format> for k < n, out_dir/images_mask.png (255 where a
    pixel has a source, 0 where it is border) and out_dir/cameras.txt, the pinhole camera those images and the poses of images.txt
    belong to.  images: an array [n, height, width, 3] BGR uint8 or a callable k -> [height, width, 3].  gains: None, or the
    exposure gains int64 [n, 3, 2] (§10r), applied on the way out.  format: "jpg" (the reference's) or "png" (lossless).  opts:
    undistort.undistort_opts' options.  Returns dict(size (w', h'), pinhole, n_valid, profile: the three device times, n_files,
    format, options)."""
    import os
    if format not in UNDISTORT_FORMATS:
        raise ValueError(f"format={format!r}: one of {UNDISTORT_FORMATS}")
    from . import dataset as D
    from .undistort import undistort_images
    img_dir = os.path.join(out_dir, "images")
    os.makedirs(img_dir, exist_ok=True)
    rep, n_files = {}, 0
    for k, bgr in undistort_images(images, intr, width, height, gains=gains, chunk=chunk, device=device, n=n, report=rep, **opts):
        D.write_image_bgr(os.path.join(img_dir, f"{k}.{format}"), bgr, quality=quality)
        n_files += 1
    D.write_image_bgr(os.path.join(out_dir, "images_mask.png"), rep.pop("mask"))
    D.write_cameras_txt(os.path.join(out_dir, "cameras.txt"), rep["size"][0], rep["size"][1], rep["pinhole"])
    return dict(size=list(rep["size"]), pinhole=list(rep["pinhole"]), n_valid=rep["n_valid"], profile=rep["profile"], n_files=n_files,
                format=format, options=rep["options"])


def _undistort_request(undistorted_images, exposure):
    """run_dataset's undistorted_images as (format, apply_exposure, undistort options), checked without touching a device"""
    kw = dict(undistorted_images) if isinstance(undistorted_images, dict) else {}
    fmt, apply_exposure = kw.pop("format", "jpg"), bool(kw.pop("apply_exposure", False))
    from . import _lib as L
    names = L.option_names(L.UndistortOpts)              # the struct's mirror: the library is not loaded
    unknown = sorted(k for k in kw if k not in names + ("quality", "chunk"))
    if unknown:
        raise ValueError(f"undistorted_images: unknown keys {unknown}; one of {('format', 'apply_exposure', 'quality', 'chunk') + names}")
    if fmt not in UNDISTORT_FORMATS:
        raise ValueError(f"undistorted_images: format={fmt!r}: one of {UNDISTORT_FORMATS}")
    if apply_exposure and not exposure:
        raise ValueError("undistorted_images: apply_exposure=True applies the gains of the exposure stage: it needs exposure=...")
    return fmt, apply_exposure, kw


def list_image_ids(image_dir, stride=1):
    """DatasetIO::handleImages (src/dataset_io.cpp:77-131): numeric ids of *.png/.jpg/.jpeg/.bmp, sorted, every stride-th."""
    import os
    from .dataset import parse_timestamp_from_name
    ids = []
    for name in os.listdir(image_dir):
        if os.path.splitext(name)[1] not in (".png", ".jpg", ".jpeg", ".bmp"):
            continue
        t = parse_timestamp_from_name(name)
        if t is not None:
            ids.append(t)
    ids.sort()
    return np.asarray(ids[::max(1, int(stride))], np.float64)


def extrinsics_from_config(Rcl, Pcl, extrinsic_R, extrinsic_T):
    """Rci = Rcl Rli, tci = Rcl tli + tcl with (Rli, tli) the inverse of the lidar->imu extrinsic (src/lvba_system.cpp:484-504)."""
    Rcl, tcl = np.asarray(Rcl, np.float64).reshape(3, 3), np.asarray(Pcl, np.float64).reshape(3)
    Ril, til = np.asarray(extrinsic_R, np.float64).reshape(3, 3), np.asarray(extrinsic_T, np.float64).reshape(3)
    Rli = Ril.T
    tli = -Rli @ til
    return Rcl @ Rli, Rcl @ tli + tcl


def run_dataset(data_path, colmap_db_path, intr, width, height, Rcl, Pcl, extrinsic_R=np.eye(3), extrinsic_T=np.zeros(3),
                image_sample_step=1, out_dir=None, device=0, colorize=False, map_quality=False, loop_closures=None, relax=None,
                matching="db", match_opts=None, pair_selection=None, device_tracks=False, verify=None, features="db",
                feature_opts=None, remove_dynamic=None, check_cameras=None, calibrate_extrinsic=False, photo_consistency=None,
                photo_align=None, exposure=None, undistorted_images=None, **cfg):
    """initFromDatasetIO + runFullPipeline on a dataset directory; with out_dir, the refined LiDAR poses (TUM) and the COLMAP
    text files images.txt / points3D.txt the reference writes (src/lvba_system.cpp:2018-2137) are saved there.  images.txt is
    the reference's, character for character (tests/test_ref_system.py).
    colorize=False (default): points3D.txt has the reference's format but holds the refined visual landmarks in white.
    colorize=True: the LiDAR map is coloured from the images as VisualizeOptComparison does (colorize_maps): all_image/<t>.png
    are decoded with Pillow into BGR as cv::imread(IMREAD_COLOR) would (8-bit RGB, RGBA and grey); an image whose size is not
    the camera's is resized with Pillow's bilinear filter, which is not OpenCV's INTER_LINEAR bit for bit.  The output gains
    colored_after / colored_before, and out_dir gets colored_merged_after.pcd / colored_merged_before.pcd (binary PCD, PCL's
    XYZRGB layout) and a points3D.txt holding the coloured after-cloud, as the reference writes them.
    map_quality (True or a dict of keywords, as for run_full_pipeline): the output gains map_quality and out_dir gets
    map_quality.json, the two summaries.
    loop_closures (True or a dict of keywords, as for run_full_pipeline): the output gains loop_closures and out_dir gets
    loop_closures.json, the report without its arrays; dict(consistency=True, ...) vets the closures against one another.
    relax (True or a dict, as for run_full_pipeline; only with loop_closures): the output gains pose_graph and out_dir gets
    pose_graph.json (the report, the closures' weights, the largest pose change).
    matching: where the feature matches come from.  "db" (default): two_view_geometries of the database (loadFromColmapDB).
    "descriptors": every image pair is matched from the database's descriptors table, unguided, as the reference's fallback does
    when the database holds no verified matches (src/lvba_system.cpp:697-833; match_image_pairs).  "guided": the same, but after
    the LiDAR stage and against the refined, LiDAR-derived camera poses, a candidate having to lie near its epipolar line -- the
    one place where the order differs from the reference's.  "depth": as "guided", but the gate is the point the LiDAR depth image
    of the keypoint's own view predicts in the other view (match_image_pairs' depth; run_full_pipeline's match_depth): it also
    separates copies of a texture along the epipolar line.  match_opts: match_image_pairs' options for the last three.
    pair_selection: None (all pairs, as the reference), True, or a dict of select_image_pairs' keywords; only with "guided" or
    "depth", where refined poses and depth images exist before the matching (run_full_pipeline's match_select): only the pairs
    selected from LiDAR co-visibility are matched; the output gains pair_selection and out_dir gets pair_selection.json.
    device_tracks: False, or True: the feature tracks are built on the GPU (run_full_pipeline's device_tracks) -- worth it where
    the matcher delivers matches by the million.
    verify: None (off), True, or a dict of verify_image_pairs' options, with every `matching` value: the matches are verified
    geometrically before the visual stage (run_full_pipeline's verify_matches); the output gains match_verification and out_dir
    gets match_verification.json.
    features: where the key points and descriptors come from.  "db" (default): the database.  "images": every all_image/<t>.png
    is read (dataset.read_image_bgr at the camera's width and height) and its SIFT features are extracted on the GPU
    (extract_image_features, feature_opts its options) -- the reference's path without a database
    (extractAndMatchFeaturesGPU, src/lvba_system.cpp:687-778); the database file is not opened.  Then `matching` must be
    "descriptors", "guided" or "depth": the database's matches index the database's key points.
    remove_dynamic (True or a dict of options, as for run_full_pipeline): the coloured maps and the map quality are made without
    the points of moving objects; the output gains dynamic and out_dir gets dynamic.json, the summary and the per-frame counts.
    check_cameras (True or a dict of options, as for run_full_pipeline): every image is resected from the LiDAR points its matches
    reach; the output gains camera_check and out_dir gets camera_check.json.
    calibrate_extrinsic (True, "apply" or a dict, as for run_full_pipeline): the extrinsic is refined from the matches and the LiDAR
    depths; the output gains extrinsic and out_dir gets extrinsic.json.
    photo_consistency (True or a dict of options, as for run_full_pipeline): the images are read as for colorize=True, whether or
    not that is set; the output gains photo_consistency, fused_after and fused_before, and out_dir gets photo_consistency.json:
    the two summaries and the options.
    photo_align (True, "apply" or a dict, as for run_full_pipeline): the images are read as for colorize=True; the output gains
    photo_align and photo_align_cameras, and out_dir gets photo_align.json: the report with its per-image arrays as lists.
    exposure (True or a dict, as for run_full_pipeline; only with photo_consistency): the output gains exposure and
    photo_consistency_raw, photo_consistency.json also holds "raw", the two summaries without compensation, and out_dir gets
    exposure.json: the report with its per-image arrays as lists.
    undistorted_images: None (off: nothing of the stage is launched and its module is not imported), True, or a dict with the keys
    format ("jpg", the reference's, or "png"), apply_exposure, quality, chunk and undistort.undistort_opts' options; needs out_dir.
    The images are read as for colorize=True and, after the run, written undistorted (export_undistorted):
    out_dir/images/<k>.<format>, one per image and per row of images.txt, images_mask.png and cameras.txt, the pinhole camera
    they belong to.  The output gains undistorted, the exporter's report, and out_dir gets undistorted.json.  With format="png"
    images.txt names k.png.  apply_exposure=True applies out["exposure"]'s gains on the way out and needs exposure (ValueError
    without it); unknown keys raise ValueError before any device is touched.
    cfg as for run_full_pipeline, e.g. visual_loss=REFERENCE_HUBER, window_loss=("cauchy", 0.1), stage_loss=("huber", 0.05),
    camera_priors=lambda cams: lidar_camera_priors(cams, Rci, tci, 1e-3, 0.02)."""
    import os
    from . import dataset as D
    if features not in ("db", "images"):
        raise ValueError(f"features={features!r}: one of 'db', 'images'")
    if features == "images" and matching not in ("descriptors", "guided", "depth"):
        raise ValueError(f"features='images' needs matching='descriptors', 'guided' or 'depth', not {matching!r}: the database's matches "
                         "index the database's key points")
    if undistorted_images:
        und_format, und_exposure, und_opts = _undistort_request(undistorted_images, exposure)
        if out_dir is None:
            raise ValueError("undistorted_images writes files: it needs out_dir")
    if pair_selection and matching not in ("guided", "depth"):
        raise ValueError(f"pair_selection needs matching='guided' or 'depth' (refined poses and depth images before the matching), not {matching!r}")
    ds = D.load_dataset(data_path)
    img_dir = os.path.join(data_path, "all_image")
    image_ids = list_image_ids(img_dir, image_sample_step)
    _, image_poses = D.load_poses_tum(os.path.join(img_dir, "image_poses.txt"), image_sample_step)
    if len(image_poses) != len(image_ids):
        raise ValueError(f"{len(image_ids)} images but {len(image_poses)} image poses")          # :457-460
    names = [f"{t:.6f}.png" for t in image_ids]                                                   # getImagePath: std::to_string
    pairs = [(i, j) for i in range(len(image_ids)) for j in range(i + 1, len(image_ids))]        # image_pairs_, :462-466
    if features == "images":
        kps, descs = extract_image_features(lambda k: D.read_image_bgr(os.path.join(img_dir, names[k]), width, height), len(names),
                                            device=device, **(feature_opts or {}))
        matches = [np.zeros((0, 2), np.int64) for _ in pairs]
    else:
        kps, matches = D.load_colmap_db(colmap_db_path if os.path.isabs(colmap_db_path) else os.path.join(data_path, colmap_db_path),
                                        names, pairs)
    if matching not in ("db", "descriptors", "guided", "depth"):
        raise ValueError(f"matching={matching!r}: one of 'db', 'descriptors', 'guided', 'depth'")
    Rci, tci = extrinsics_from_config(Rcl, Pcl, extrinsic_R, extrinsic_T)
    match_fn, all_pairs = None, pairs
    if matching != "db":
        if features == "db":
            descs = D.load_colmap_descriptors(colmap_db_path if os.path.isabs(colmap_db_path) else os.path.join(data_path, colmap_db_path),
                                              names)
            descs = [d if len(d) == len(k) else np.zeros((0, 128), np.uint8) for d, k in zip(descs, kps)]   # rows are key points
            kps = [k if len(d) else k[:0] for d, k in zip(descs, kps)]
        if matching == "descriptors":
            matches = match_image_pairs(descs, pairs, device=device, **(match_opts or {}))
        else:
            def match_fn(cam_poses, depth=None, pairs=None):
                use = all_pairs if pairs is None else pairs
                Rcw, tcw = camera_from_imu(cam_poses, Rci, tci)
                m = match_image_pairs(descs, use, keypoints=[k[:, :2] for k in kps], Rcw=Rcw, tcw=tcw, intr=intr, device=device,
                                      depth=depth, **(match_opts or {}))
                kept = [k for k, mm in enumerate(m) if len(mm)]
                return [use[k] for k in kept], [m[k] for k in kept]
    keep = [k for k, m in enumerate(matches) if len(m)]
    out = run_full_pipeline([c[:, :3] for c in ds["clouds"]], ds["poses"], ds["timestamps"], image_ids, image_poses, Rci, tci, intr,
                            width, height, [k[:, :2] for k in kps], [pairs[k] for k in keep], [matches[k] for k in keep],
                            device=device, **({"match_fn": match_fn} if match_fn is not None else {}),
                            **({"match_depth": True} if matching == "depth" else {}),
                            **({"match_select": pair_selection} if pair_selection else {}),
                            **({"device_tracks": True} if device_tracks else {}), **({"verify_matches": verify} if verify else {}),
                            images=(lambda k: D.read_image_bgr(os.path.join(img_dir, names[k]), width, height))
                            if colorize or photo_consistency or photo_align else None, **({"map_quality": map_quality} if map_quality else {}),
                            **({"photo_consistency": photo_consistency} if photo_consistency else {}),
                            **({"photo_align": photo_align} if photo_align else {}),
                            **({"exposure": exposure} if exposure else {}),
                            **({"loop_closures": loop_closures} if loop_closures else {}),
                            **({"relax": relax} if relax and loop_closures else {}),
                            **({"remove_dynamic": remove_dynamic} if remove_dynamic else {}),
                            **({"check_cameras": check_cameras} if check_cameras else {}),
                            **({"calibrate_extrinsic": calibrate_extrinsic} if calibrate_extrinsic else {}), **cfg)
    out.update(image_ids=image_ids, scan_times=ds["timestamps"])
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        D.write_poses_tum(os.path.join(out_dir, "lidar_poses_refined.txt"), ds["timestamps"], out["poses"])
        v = out.get("visual")
        if v is not None and len(v.get("landmarks", [])):
            D.write_images_txt(os.path.join(out_dir, "images.txt"), rot_to_quat_wxyz(v["Rcw"]), v["tcw"],
                               **({"ext": und_format} if undistorted_images and und_format != "jpg" else {}))
            if not colorize:
                ok = v["landmark_valid"] > 0
                D.write_points3d_txt(os.path.join(out_dir, "points3D.txt"), v["landmarks"][ok], np.full((int(ok.sum()), 3), 255))
        if colorize:
            D.save_pcd_xyzrgb(os.path.join(out_dir, "colored_merged_after.pcd"), *out["colored_after"])
            D.save_pcd_xyzrgb(os.path.join(out_dir, "colored_merged_before.pcd"), *out["colored_before"])
            D.write_points3d_txt(os.path.join(out_dir, "points3D.txt"), *out["colored_after"])
        if map_quality:
            import json
            with open(os.path.join(out_dir, "map_quality.json"), "w") as f:
                json.dump({k: None if q is None else {a: b for a, b in q.items() if not isinstance(b, np.ndarray)}
                           for k, q in out["map_quality"].items()}, f, indent=1)
        if "photo_consistency" in out:
            import json
            with open(os.path.join(out_dir, "photo_consistency.json"), "w") as f:
                json.dump({"after": out["photo_consistency"]["after"], "before": out["photo_consistency"]["before"],
                           "options": out.get("photo_options"),
                           **({"raw": out["photo_consistency_raw"]} if "photo_consistency_raw" in out else {})}, f, indent=1)
        plain = lambda q: q.tolist() if isinstance(q, np.ndarray) else [plain(e) for e in q] if isinstance(q, list) else \
            {a: plain(b) for a, b in q.items()} if isinstance(q, dict) else q
        if "exposure" in out:
            import json
            with open(os.path.join(out_dir, "exposure.json"), "w") as f:
                json.dump(plain(out["exposure"]), f, indent=1)
        if undistorted_images:
            import json
            out["undistorted"] = export_undistorted(
                out_dir, lambda k: D.read_image_bgr(os.path.join(img_dir, names[k]), width, height), len(names), intr, width, height,
                gains=out["exposure"]["gains"] if und_exposure else None, format=und_format, device=device, **und_opts)
            with open(os.path.join(out_dir, "undistorted.json"), "w") as f:
                json.dump(plain(out["undistorted"]), f, indent=1)
        if "photo_align" in out:
            import json
            with open(os.path.join(out_dir, "photo_align.json"), "w") as f:
                json.dump(plain(out["photo_align"]), f, indent=1)
        if "dynamic" in out:
            import json
            with open(os.path.join(out_dir, "dynamic.json"), "w") as f:
                json.dump({a: b.tolist() if a == "per_frame" else b for a, b in out["dynamic"].items()
                           if a == "per_frame" or not isinstance(b, np.ndarray)}, f, indent=1)
        if loop_closures:
            import json
            with open(os.path.join(out_dir, "loop_closures.json"), "w") as f:
                json.dump([{a: b for a, b in r.items() if not isinstance(b, np.ndarray)} for r in out["loop_closures"]], f, indent=1)
        if "pair_selection" in out:
            import json
            with open(os.path.join(out_dir, "pair_selection.json"), "w") as f:
                json.dump(out["pair_selection"], f, indent=1)
        if "match_verification" in out:
            import json
            with open(os.path.join(out_dir, "match_verification.json"), "w") as f:
                json.dump(out["match_verification"], f, indent=1)
        if "camera_check" in out:
            import json
            with open(os.path.join(out_dir, "camera_check.json"), "w") as f:
                json.dump(out["camera_check"], f, indent=1)
        if "extrinsic" in out:
            import json
            with open(os.path.join(out_dir, "extrinsic.json"), "w") as f:
                json.dump(out["extrinsic"], f, indent=1)
        if "pose_graph" in out:
            import json
            with open(os.path.join(out_dir, "pose_graph.json"), "w") as f:
                json.dump(out["pose_graph"], f, indent=1)
    return out
