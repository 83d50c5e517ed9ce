"""Host-side mirror of the reference's BALM interface over the C-ABI.

`BalmProblem` is the thin object wrapper of an `lvba_balm_t` handle.  `VOX_HESS` / `BALM2` mirror the
reference classes of the same names (include/BALM/bavoxel.hpp:32-269, 587-767) -- same method names,
argument meaning and return values -- so the parity tests read like calls into the reference:

    voxhess = VOX_HESS(win_size); voxhess.push_voxel(sig_orig)            # bavoxel.hpp:45-54
    opt = BALM2(win_size); opt.damping_iter(x_stats, voxhess)              # bavoxel.hpp:662

All arithmetic runs in liblvba_hip.so on the GPU; this file only packs arrays and forwards calls.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def shard_range(n_voxels, rank, n_ranks):
    """[floor(V*r/G), floor(V*(r+1)/G)) -- bavoxel.hpp:621-624 with thread -> GPU."""
    a, b = C.c_int64(), C.c_int64()
    L.load().lvba_shard_range(int(n_voxels), int(rank), int(n_ranks), C.byref(a), C.byref(b))
    return a.value, b.value


def _pose12(T):
    """a pose as 12 doubles R row-major | p, from 12 numbers, a 4 x 4 / 3 x 4 matrix or an (R, p) pair"""
    if isinstance(T, (tuple, list)) and len(T) == 2:
        return np.r_[np.asarray(T[0], np.float64).reshape(9), np.asarray(T[1], np.float64).reshape(3)]
    a = np.asarray(T, np.float64)
    if a.shape in ((4, 4), (3, 4)):
        return np.r_[a[:3, :3].reshape(9), a[:3, 3]]
    return a.reshape(12)


def _sqrt_info(sqrt_info, sigma_rot, sigma_pos):
    if sqrt_info is not None:
        return np.asarray(sqrt_info, np.float64).reshape(6, 6)
    if sigma_rot is None or sigma_pos is None:
        raise ValueError("give sigma_rot and sigma_pos, or sqrt_info")
    sr = np.broadcast_to(np.asarray(sigma_rot, np.float64), (3,))
    sp = np.broadcast_to(np.asarray(sigma_pos, np.float64), (3,))
    return np.diag(1.0 / np.r_[sr, sp])


class Prior:
    """Pose priors of the LiDAR bundle adjustment (lvba_balm_set_priors; model in include/lvba_hip.h).  Poses and offsets are 12
    numbers (R row-major | p), a 4 x 4 matrix or an (R, p) pair; sigma_rot [rad] / sigma_pos [m] are scalars or 3-vectors and make a
    diagonal square-root information diag(1 / sigma), or sqrt_info gives the 6 x 6 matrix itself (row-major).  Offsets are body-frame
    transforms O: the prior constrains T_i O (identity by default)."""

    @staticmethod
    def _make(kind, i, j, meas, L6, oi, oj):
        p = L.Prior()
        p.kind, p.i, p.j, p.reserved = L.PRIOR_KINDS[kind], int(i), int(j), 0
        p.meas[:] = [float(v) for v in meas]
        p.offset_i[:] = [float(v) for v in (np.zeros(12) if oi is None else _pose12(oi))]
        p.offset_j[:] = [float(v) for v in (np.zeros(12) if oj is None else _pose12(oj))]
        p.sqrt_info[:] = [float(v) for v in np.asarray(L6, np.float64).reshape(36)]
        return p

    @staticmethod
    def pose(i, T, sigma_rot=None, sigma_pos=None, sqrt_info=None, offset=None):
        """r = [Log(R^T R_A); p_A - p] with A = T_i offset"""
        return Prior._make("pose", i, 0, _pose12(T), _sqrt_info(sqrt_info, sigma_rot, sigma_pos), offset, None)

    @staticmethod
    def position(i, z, sigma=None, sqrt_info=None, lever_arm=None):
        """r = R_i lever_arm + p_i - z (a GNSS fix of the antenna at `lever_arm` in the body frame); sqrt_info: 3 x 3 (or 6 x 6,
        of which the top-left 3 x 3 is read)"""
        L6 = np.zeros((6, 6))
        if sqrt_info is not None:
            a = np.asarray(sqrt_info, np.float64)
            L6[:3, :3] = a[:3, :3] if a.shape == (6, 6) else a.reshape(3, 3)
        elif sigma is not None:
            L6[:3, :3] = np.diag(1.0 / np.broadcast_to(np.asarray(sigma, np.float64), (3,)))
        else:
            raise ValueError("give sigma or sqrt_info")
        meas = np.r_[np.eye(3).reshape(9), np.asarray(z, np.float64).reshape(3)]
        off = None if lever_arm is None else np.r_[np.eye(3).reshape(9), np.asarray(lever_arm, np.float64).reshape(3)]
        return Prior._make("position", i, 0, meas, L6, off, None)

    @staticmethod
    def relative(i, j, T_ij, sigma_rot=None, sigma_pos=None, sqrt_info=None, offset_i=None, offset_j=None):
        """r = [Log(R_ij^T R_A^T R_B); R_A^T (p_B - p_A) - p_ij] with A = T_i offset_i, B = T_j offset_j"""
        return Prior._make("relative", i, j, _pose12(T_ij), _sqrt_info(sqrt_info, sigma_rot, sigma_pos), offset_i, offset_j)


class BalmProblem(L.Handle):
    """One packed LiDAR-BA problem (or one rank's voxel shard) resident on a GPU."""
    _destroy = "lvba_balm_destroy"

    def __init__(self, n_poses, voxel_off, pose_idx, clusters, device=0, ordering=None, band_frac=None):
        self.lib = L.load()
        voxel_off = np.ascontiguousarray(voxel_off, np.int64)
        pose_idx = np.ascontiguousarray(pose_idx, np.int32)
        clusters = np.ascontiguousarray(clusters, np.float64).reshape(-1, 10)
        self.n_poses = int(n_poses)
        self.n_voxels = len(voxel_off) - 1
        self._h = C.c_void_p()
        # pose_idx / clusters are indexed relative to voxel_off[0]
        L.check(self.lib.lvba_balm_create(self.n_poses, self.n_voxels, voxel_off, pose_idx, clusters.reshape(-1),
                                          int(device), C.byref(self._h)))
        if ordering is not None or band_frac is not None:
            L.check(self.lib.lvba_balm_configure(self._h, 1 if ordering is None else int(ordering),
                                                 0.6 if band_frac is None else float(band_frac)))

    @classmethod
    def _from_handle(cls, handle, n_poses, n_voxels, ordering=None, band_frac=None):
        """Wrap an lvba_balm_t made by another entry point (lvba_voxmap_to_balm)."""
        self = cls.__new__(cls)
        self.lib = L.load()
        self.n_poses, self.n_voxels, self._h = int(n_poses), int(n_voxels), handle
        if ordering is not None or band_frac is not None:
            L.check(self.lib.lvba_balm_configure(self._h, 1 if ordering is None else int(ordering),
                                                 0.6 if band_frac is None else float(band_frac)))
        return self

    def _poses(self, poses):
        x = np.ascontiguousarray(poses, np.float64).reshape(-1)
        if x.size != 12 * self.n_poses:
            raise ValueError(f"poses must hold {self.n_poses} x 12 doubles")
        return x

    # -- multi-GPU ----------------------------------------------------------------------------------
    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        L.check(L.load().lvba_dist_unique_id(buf))
        return buf.raw

    def dist_init(self, n_ranks, rank, uid):
        L.check(self.lib.lvba_balm_dist_init(self._h, int(n_ranks), int(rank), bytes(uid)))

    def dist_init_external(self, n_ranks, rank, fn, ctx):
        """The caller's all-reduce instead of RCCL (lvba_balm_dist_init_external): fn = address of an lvba_allreduce_fn,
        ctx = its context pointer."""
        L.check(self.lib.lvba_balm_dist_init_external(self._h, int(n_ranks), int(rank), C.c_void_p(fn), C.c_void_p(ctx)))

    # -- queries ------------------------------------------------------------------------------------
    def info(self):
        i = L.BalmInfo()
        L.check(self.lib.lvba_balm_info(self._h, C.byref(i)))
        return i.as_dict()

    def pair_layout(self):
        """how the pair pass was laid out (lvba_balm_pair_layout): form, cut, n_items, n_multi, n_partial, window_voxels,
        longest_item, longest_multi, and per item item_len / item_slot (-1 - k: partial block k)"""
        return L.pair_layout(self.lib.lvba_balm_pair_layout, self._h)

    def eval_layout(self):
        """how the factor pass is launched (lvba_balm_eval_layout): slices per pose, units = unit_grid = its (pose, slice)
        workgroups, n_groups = voxels, n_factors, n_chunks of the voxel pass"""
        return L.eval_layout(self.lib.lvba_balm_eval_layout, self._h)

    def nd_model(self, n_ranks):
        """the nested-dissection plan of this problem's graph on n_ranks ranks and its cost model (lvba_balm_nd_model)"""
        m = L.NdModel()
        L.check(self.lib.lvba_balm_nd_model(self._h, int(n_ranks), C.byref(m)))
        return m.as_dict()

    def ordering(self):
        perm = np.empty(self.n_poses, np.int32)
        L.check(self.lib.lvba_balm_get_ordering(self._h, perm))
        return perm

    def set_profiling(self, on=True):
        L.check(self.lib.lvba_balm_set_profiling(self._h, 1 if on else 0))

    def profile(self, reset=False):
        p = L.Prof()
        L.check(self.lib.lvba_balm_get_profile(self._h, C.byref(p), 1 if reset else 0))
        return p.as_dict()

    # -- the hot path ---------------------------------------------------------------------------------
    def cost(self, poses, is_avg=False):
        out = C.c_double()
        L.check(self.lib.lvba_balm_cost(self._h, self._poses(poses), 1 if is_avg else 0, C.byref(out)))
        return out.value

    def eval(self, poses, want_H=True, want_g=True):
        n = 6 * self.n_poses
        H = np.empty((n, n)) if want_H else None
        g = np.empty(n) if want_g else None
        c = C.c_double()
        L.check(self.lib.lvba_balm_eval(self._h, self._poses(poses), H.ctypes.data if want_H else None,
                                        g.ctypes.data if want_g else None, C.byref(c)))
        return H, g, c.value

    def eval_blocks(self, poses):
        """H in sparse form (lvba_balm_eval_blocks): (bi, bj, blocks [nb, 6, 6], g, cost) with bi >= bj in the caller's pose
        order, every unordered pair once, blocks[k, r, c] = H[6 bi + r, 6 bj + c]."""
        x = self._poses(poses)
        nb = C.c_int64()
        c = C.c_double()
        L.check(self.lib.lvba_balm_eval_blocks(self._h, x, 0, None, None, None, C.byref(nb), None, None))
        cap = int(nb.value)
        bi, bj = np.empty(cap, np.int32), np.empty(cap, np.int32)
        blocks = np.empty((cap, 6, 6))
        g = np.empty(6 * self.n_poses)
        L.check(self.lib.lvba_balm_eval_blocks(self._h, x, cap, bi.ctypes.data, bj.ctypes.data, blocks.ctypes.data, C.byref(nb),
                                               g.ctypes.data, C.byref(c)))
        return bi, bj, blocks, g, c.value

    def solve(self, u):
        dx = np.empty(6 * self.n_poses)
        L.check(self.lib.lvba_balm_solve(self._h, float(u), dx))
        return dx

    @staticmethod
    def default_opts(**kw):
        return L.make_opts(L.BalmOpts, "LM", **kw)

    def refine(self, poses, **opts):
        o = self.default_opts(**opts)
        x = self._poses(poses).copy()
        trace = (L.LmTrace * max(1, o.max_iter))()
        nt = C.c_int32()
        rc = L.check(self.lib.lvba_balm_refine(self._h, x, C.byref(o), trace, C.byref(nt)), allow_numeric=True)
        return x.reshape(-1, 12), [trace[i].as_dict() for i in range(nt.value)], rc

    def set_priors(self, priors):
        """Pose priors (lvba_balm_set_priors): a sequence of Prior.pose / .position / .relative; empty or None clears them.
        Relative priors that join new pairs of poses must come before the first cost / eval / refine call."""
        priors = list(priors or [])
        arr = (L.Prior * max(1, len(priors)))(*priors)
        L.check(self.lib.lvba_balm_set_priors(self._h, len(priors), C.cast(arr, C.c_void_p) if priors else None))
        self.n_priors = len(priors)

    def prior_residuals(self, poses):
        """(e [n, 6] whitened residuals L r in the order given to set_priors -- position priors fill e[k, :3] --, their cost
        sum 1/2 |e|^2)"""
        n = getattr(self, "n_priors", 0)
        e = np.zeros((max(n, 1), 6))
        c = C.c_double()
        L.check(self.lib.lvba_balm_prior_residuals(self._h, self._poses(poses), e.ctypes.data, C.byref(c)))
        return e[:n], c.value

    def set_loss(self, loss=None):
        """Robust loss on the voxel costs (lvba_balm_set_loss): None (the default, plain sum of lambda_min) or (kind, scale) with
        kind one of "trivial", "huber", "softlone", "cauchy", "arctan", "tukey" (or an LVBA_LOSS_* integer) and the scale a in
        metres -- a voxel is down-weighted when its RMS plane distance exceeds a (not "arctan": see include/lvba_hip.h).  Not between lm_begin and lm_end."""
        L.check(self.lib.lvba_balm_set_loss(self._h, L.loss_struct(loss)))

    def voxel_residuals(self, poses):
        """(lambda_min [n_voxels], weight [n_voxels] = rho'(lambda_min)) at `poses`, in the order the voxels were given to the
        constructor (lvba_balm_voxel_residuals); every weight is 1 without a loss."""
        lam, w = np.empty(self.n_voxels), np.empty(self.n_voxels)
        L.check(self.lib.lvba_balm_voxel_residuals(self._h, self._poses(poses), lam.ctypes.data, w.ctypes.data))
        return lam, w

    def covariance(self, poses, anchor=None, pairs=None, min_pivot_ratio=1e-10, scale=1.0):
        """Marginal pose covariance Sigma = H(poses)^-1 (lvba_balm_covariance): the inverse Hessian of the cost the LM minimises,
        in the tangent [dphi; dp] of each pose, caller order.  anchor: a pose held fixed (its blocks come back as zeros), or None
        when priors fix the frame.  pairs: (K, 2) caller indices i != j.  scale multiplies every block (Sigma is in the cost's
        units; a noise variance turns it into a metric covariance).  Returns (diag [N, 6, 6], pair_blocks [K, 6, 6], avail [K]):
        avail[k] is False for a pair outside the solver's band, whose block is NaN."""
        x = self._poses(poses)
        o = L.make_opts(L.CovOpts, "covariance", anchor=-1 if anchor is None else anchor, min_pivot_ratio=min_pivot_ratio)
        pr = np.ascontiguousarray(np.zeros((0, 2)) if pairs is None else pairs, np.int32).reshape(-1, 2)
        K = pr.shape[0]
        pi, pj = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        diag = np.empty((self.n_poses, 6, 6))
        blocks = np.empty((K, 6, 6))
        avail = np.zeros(K, np.uint8)
        L.check(self.lib.lvba_balm_covariance(self._h, x, C.byref(o), diag.ctypes.data, K, pi.ctypes.data if K else None,
                                              pj.ctypes.data if K else None, blocks.ctypes.data if K else None,
                                              avail.ctypes.data if K else None))
        if scale != 1.0:
            diag *= scale
            blocks *= scale
        return diag, blocks, avail.astype(bool)

    def set_groups(self, pose_off, voxel_off):
        """Independent groups of poses / voxels (lvba_balm_set_groups); before the first cost / eval / refine call."""
        po = np.ascontiguousarray(pose_off, dtype=np.int32)
        vo = np.ascontiguousarray(voxel_off, dtype=np.int64)
        if len(po) != len(vo) or len(po) < 2:
            raise ValueError("pose_off and voxel_off need n_groups + 1 entries each")
        L.check(self.lib.lvba_balm_set_groups(self._h, len(po) - 1, po, vo))
        self.n_groups = len(po) - 1

    def refine_groups(self, poses, **opts):
        """All groups through one LM loop in lock-step; returns (poses, per-group dict of arrays, rc)."""
        o = self.default_opts(**opts)
        x = self._poses(poses).copy()
        G = self.n_groups
        n_iter, status = np.zeros(G, np.int32), np.zeros(G, np.int32)
        first, last = np.zeros(G), np.zeros(G)
        rc = L.check(self.lib.lvba_balm_refine_groups(self._h, x, C.byref(o), n_iter, status, first, last), allow_numeric=True)
        return x.reshape(-1, 12), dict(n_iter=n_iter, status=status, cost_first=first, cost_last=last), rc

    def lm_begin(self, poses, **opts):
        o = self.default_opts(**opts)
        L.check(self.lib.lvba_balm_lm_begin(self._h, self._poses(poses), C.byref(o)))

    def lm_step(self):
        row, done = L.LmTrace(), C.c_int32()
        rc = L.check(self.lib.lvba_balm_lm_step(self._h, C.byref(row), C.byref(done)), allow_numeric=True)
        return row.as_dict(), bool(done.value), rc

    def lm_end(self, want_poses=True):
        out = np.empty((self.n_poses, 12)) if want_poses else None
        L.check(self.lib.lvba_balm_lm_end(self._h, out.ctypes.data if want_poses else None))
        return out


# =====================================================================================================
# Mirror of the reference classes (same names / call shapes as include/BALM/bavoxel.hpp)
# =====================================================================================================
class IMUST:
    """Pose state; only R, p (and t) are live on this path (tools.hpp:147-207)."""

    def __init__(self, R=None, p=None, t=0.0):
        self.R = np.eye(3) if R is None else np.array(R, dtype=np.float64).reshape(3, 3)
        self.p = np.zeros(3) if p is None else np.array(p, dtype=np.float64).reshape(3)
        self.t = t


def pack_x_stats(x_stats):
    return np.stack([np.concatenate([x.R.reshape(9), x.p]) for x in x_stats])


def unpack_x_stats(poses, x_stats):
    for x, row in zip(x_stats, np.asarray(poses).reshape(-1, 12)):
        x.R = row[:9].reshape(3, 3).copy()
        x.p = row[9:12].copy()


class VOX_HESS:
    """bavoxel.hpp:32-54.  `sig_orig` is one voxel's win_size PointCluster slots as an array
    [win_size, 10] (Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N); empty slots have N == 0."""

    def __init__(self, win_size=10):
        self.win_size = int(win_size)
        self.plvec_voxels = []

    def push_voxel(self, sig_orig, vec_orig=None):
        sig = np.asarray(sig_orig, dtype=np.float64).reshape(self.win_size, 10)
        if np.count_nonzero(sig[:, 9] != 0) < 2:      # bavoxel.hpp:47-52
            return
        self.plvec_voxels.append(sig)

    def pack(self):
        """CSR arrays of lvba_balm_create: the non-empty slots of every admitted voxel, ascending pose."""
        offs, idx, clu = [0], [], []
        for sig in self.plvec_voxels:
            nz = np.nonzero(sig[:, 9] != 0)[0]
            idx.append(nz.astype(np.int32))
            clu.append(sig[nz])
            offs.append(offs[-1] + len(nz))
        return (np.asarray(offs, np.int64), np.concatenate(idx) if idx else np.zeros(0, np.int32),
                np.concatenate(clu) if clu else np.zeros((0, 10)))


class BALM2:
    """bavoxel.hpp:587-767 on the GPU.  The packed device problem is cached per VOX_HESS instance."""

    def __init__(self, win_size=10, device=0):
        self.win_size = int(win_size)
        self.jac_leng = 6 * self.win_size
        self.device = device
        self._cache = (None, None)
        self.last_trace = []

    def _problem(self, voxhess):
        if self._cache[0] is not voxhess or self._cache[1] is None:
            off, idx, clu = voxhess.pack()
            if self._cache[1] is not None:
                self._cache[1].close()
            self._cache = (voxhess, BalmProblem(self.win_size, off, idx, clu, device=self.device))
        return self._cache[1]

    def divide_thread(self, x_stats, voxhess, x_ab=None):
        """-> (residual averaged over voxels, Hess [6N,6N], JacT [6N])   bavoxel.hpp:597-639"""
        H, g, c = self._problem(voxhess).eval(pack_x_stats(x_stats))
        return c, H, g

    def only_residual(self, x_stats, voxhess, x_ab=None, is_avg=False):
        """bavoxel.hpp:641-648"""
        return self._problem(voxhess).cost(pack_x_stats(x_stats), is_avg)

    def damping_iter(self, x_stats, voxhess):
        """Refines x_stats in place (bavoxel.hpp:662-767); the LM trace is kept in self.last_trace."""
        x, trace, rc = self._problem(voxhess).refine(pack_x_stats(x_stats))
        self.last_trace = trace
        unpack_x_stats(x, x_stats)
        return rc
