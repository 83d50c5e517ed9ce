"""The LiDAR map coloured from the camera images (lvba_colorize_t), LvbaSystem::VisualizeOptComparison of the reference
(src/lvba_system.cpp:1932-2144) for one pose set:

    with ColorMap(scans, scan_poses, scan_times, intr, width, height) as cm:
        cm.add_images(image_times, Rcw, tcw, bgr)         # any number of calls, in image order
        xyz, rgb = cm.download()

Every point of the scans within +-half_window_s of an image is projected into it, a pixel keeps the point the reference's
depth buffer keeps and takes its colour; the merged cloud is thinned as down_sampling_voxel2 does (leaf_size, 0.01 m;
below 1 mm: no thinning).  Everything runs in liblvba_hip.so on the GPU; this file packs arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def default_opts():
    return L.make_opts(L.ColorizeOpts, "colourisation")


class ColorMap(L.Handle):
    """One coloured cloud: scans (a voxel.Scans) seen from their poses scan_poses [n,12] (R row-major | t, T_world<-body),
    scan_times ascending; images of width x height through intr = fx fy cx cy k1 k2 p1 p2."""
    _destroy = "lvba_colorize_destroy"

    def __init__(self, scans, scan_poses, scan_times, intr, width, height, half_window_s=0.5, leaf_size=0.01, max_batch_images=0):
        self.lib = L.load()
        self.width, self.height = int(width), int(height)
        o = L.make_opts(L.ColorizeOpts, "colourisation", half_window_s=half_window_s, leaf_size=leaf_size, max_batch_images=max_batch_images)
        self._h = C.c_void_p()
        L.check(self.lib.lvba_colorize_create(scans._h, np.ascontiguousarray(scan_poses, np.float64).reshape(-1),
                                              np.ascontiguousarray(scan_times, np.float64).reshape(-1),
                                              np.ascontiguousarray(intr, np.float64).reshape(-1), self.width, self.height,
                                              C.byref(o), C.byref(self._h)))

    def add_images(self, image_times, Rcw, tcw, bgr):
        """image_times [m]; Rcw [m,3,3], tcw [m,3] (T_cam<-world); bgr [m,height,width,3] uint8 (cv::imread's channel order)."""
        t = np.ascontiguousarray(image_times, np.float64).reshape(-1)
        m = len(t)
        R = np.ascontiguousarray(Rcw, np.float64).reshape(-1)
        tc = np.ascontiguousarray(tcw, np.float64).reshape(-1)
        img = np.ascontiguousarray(bgr, np.uint8)
        if R.size != 9 * m or tc.size != 3 * m or img.shape != (m, self.height, self.width, 3):
            raise ValueError(f"{m} images: Rcw {R.size // 9}, tcw {tc.size // 3}, bgr {img.shape} "
                             f"(want [{m},{self.height},{self.width},3])")
        L.check(self.lib.lvba_colorize_add_images(self._h, m, t.ctypes.data, R.ctypes.data, tc.ctypes.data, img.ctypes.data))

    def count(self):
        n = C.c_int64()
        L.check(self.lib.lvba_colorize_count(self._h, C.byref(n)))
        return n.value

    def download(self):
        """(xyz [n,3] float32, rgb [n,3] uint8): sorted by leaf key when thinned, else in merge order."""
        n = self.count()
        xyz, rgb = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8)
        L.check(self.lib.lvba_colorize_download(self._h, xyz.ctypes.data, rgb.ctypes.data))
        return xyz, rgb

    def profile(self):
        """Accumulated device time (ms) of the stages."""
        ms = np.zeros(6)
        L.check(self.lib.lvba_colorize_profile(self._h, ms.ctypes.data))
        return dict(zip(("upload", "project", "sort", "walk", "compact", "thin"), ms.tolist()))
