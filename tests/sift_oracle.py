"""numpy restatement of the SIFT extractor's rule (include/lvba_hip.h, "SIFT key points and descriptors"), written
from the rule and not from the kernels.  The blur taps are an input: the tests hand in the library's, so that a last-bit difference
between two `exp`s cannot reach the pyramid (test_sift_host.py pins the library's taps against numpy's).

Every transcendental of the orientation and the descriptor goes through a `Libm`; `Libm(perturb=True)` scales each result by
1 +- 1e-12 with the sign from a counter hash -- the second evaluation of the fragility test."""
import math

import numpy as np

F = np.float32
TWO_PI = 6.283185307179586
LN2 = 0.6931471805599453
DEFAULTS = dict(first_octave=-1, n_intervals=3, sigma0=1.6, dog_threshold=0.01, edge_threshold=12.0, orientation_window=3.0,
                max_orientations=2, max_features=8192)


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    o.pop("chunk_images", None)
    return o


class Libm:
    def __init__(self, perturb=False):
        self.perturb, self.n = perturb, 0

    def _p(self, v):
        if not self.perturb:
            return v
        v = np.asarray(v, np.float64)
        k = (self.n + np.arange(v.size, dtype=np.uint64)).reshape(v.shape)
        self.n += v.size
        sign = np.where(((k * np.uint64(2654435761)) >> np.uint64(15)) & np.uint64(1), 1.0, -1.0)
        out = v * (1.0 + sign * 1e-12)
        return out if out.ndim else float(out)

    def exp(self, v): return self._p(np.exp(v))
    def sqrt(self, v): return self._p(np.sqrt(v))
    def atan2(self, a, b): return self._p(np.arctan2(a, b))
    def cos(self, v): return self._p(np.cos(v))
    def sin(self, v): return self._p(np.sin(v))


# ---------------------------------------------------------------------------------------------------------------- taps
def level_sigma(o, level):
    if level == 0:
        assumed = 1.0 if o["first_octave"] < 0 else 0.5
        return math.sqrt(o["sigma0"] * o["sigma0"] - assumed * assumed)
    S = float(o["n_intervals"])
    return o["sigma0"] * 2.0 ** ((level - 1) / S) * math.sqrt(2.0 ** (2.0 / S) - 1.0)


def numpy_taps(o, level):
    """fp64: exp(-k^2 / (2 sigma^2)) over their sum, k = -r .. r, r = ceil(4 sigma)"""
    sigma = level_sigma(o, level)
    r = int(math.ceil(4.0 * sigma))
    k = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return g / g.sum(), r


# ------------------------------------------------------------------------------------------------------------- pyramid
def grey(img):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.astype(F) / F(255.0)
    b, g, r = (img[:, :, k].astype(F) for k in range(3))
    return ((F(0.299) * r + F(0.587) * g) + F(0.114) * b) / F(255.0)


def base_image(img, o):
    g = grey(img)
    if o["first_octave"] >= 0:
        return g
    h, w = g.shape
    H = np.zeros((h, 2 * w), F)
    H[:, 0::2] = g
    H[:, 1::2] = F(0.5) * (g + g[:, np.minimum(np.arange(w) + 1, w - 1)])
    B = np.zeros((2 * h, 2 * w), F)
    B[0::2] = H
    B[1::2] = F(0.5) * (H + H[np.minimum(np.arange(h) + 1, h - 1)])
    return B


def blur(a, taps):
    """rows, then columns; fp32 products and sums, taps ascending, indices clamped"""
    taps = np.asarray(taps, F)
    r = (len(taps) - 1) // 2

    def rows(a):
        w = a.shape[1]
        acc = taps[0] * a[:, np.clip(np.arange(w) - r, 0, w - 1)]
        for k in range(1, 2 * r + 1):
            acc = acc + taps[k] * a[:, np.clip(np.arange(w) + k - r, 0, w - 1)]
        return acc
    return np.ascontiguousarray(rows(rows(a).T).T)


def octave_sizes(w, h, o):
    if o["first_octave"] < 0:
        w, h = 2 * w, 2 * h
    out = []
    while True:
        out.append((w, h))
        w, h = w // 2, h // 2
        if min(w, h) < 8:
            return out


def pyramid(img, o, taps):
    """[(gauss [S + 3, h, w], dog [S + 2, h, w])] per octave; taps[level] fp32, level 0 .. S + 2"""
    S = o["n_intervals"]
    h, w = np.asarray(img).shape[:2]
    level0 = blur(base_image(img, o), taps[0])
    out = []
    for k, (ow, oh) in enumerate(octave_sizes(w, h, o)):
        assert level0.shape == (oh, ow)
        G = [level0]
        for l in range(1, S + 3):
            G.append(blur(G[-1], taps[l]))
        G = np.stack(G)
        out.append((G, G[1:] - G[:-1]))
        level0 = np.ascontiguousarray(G[S][0:2 * (oh // 2):2, 0:2 * (ow // 2):2])
    return out


# ---------------------------------------------------------------------------------------------------------- key points
def pow2(z):
    n = int(z)
    if float(n) > z:
        n -= 1
    u = (z - float(n)) * LN2
    r = 1.0
    for k in range(20, 0, -1):
        r = 1.0 + (u / float(k)) * r
    for _ in range(abs(n)):
        r = r * 2.0 if n > 0 else r * 0.5
    return r


def extrema(D, o):
    """(l, y, x) of the candidates of one octave, in (l, y, x) order"""
    S = o["n_intervals"]
    nl, h, w = D.shape
    thr = (0.5 * o["dog_threshold"]) / float(S)
    c = D[1:S + 1, 1:h - 1, 1:w - 1]
    gt = np.ones(c.shape, bool)
    lt = np.ones(c.shape, bool)
    for dl in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dl == dy == dx == 0:
                    continue
                nb = D[1 + dl:S + 1 + dl, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                gt &= c > nb
                lt &= c < nb
    hit = (np.abs(c).astype(np.float64) > thr) & (gt | lt)
    l, y, x = np.nonzero(hit)
    return np.stack([l + 1, y + 1, x + 1], 1)


def refine(D, o, x, y, l):
    """None, or (x, y, l, ox, oy, ol)"""
    S = o["n_intervals"]
    nl, h, w = D.shape

    def d(L, Y, X):
        return float(D[L, Y, X])
    moves = 0
    while True:
        v = d(l, y, x)
        gx = 0.5 * (d(l, y, x + 1) - d(l, y, x - 1))
        gy = 0.5 * (d(l, y + 1, x) - d(l, y - 1, x))
        gs = 0.5 * (d(l + 1, y, x) - d(l - 1, y, x))
        dxx = (d(l, y, x + 1) + d(l, y, x - 1)) - 2.0 * v
        dyy = (d(l, y + 1, x) + d(l, y - 1, x)) - 2.0 * v
        dss = (d(l + 1, y, x) + d(l - 1, y, x)) - 2.0 * v
        dxy = 0.25 * ((d(l, y + 1, x + 1) - d(l, y + 1, x - 1)) - (d(l, y - 1, x + 1) - d(l, y - 1, x - 1)))
        dxs = 0.25 * ((d(l + 1, y, x + 1) - d(l + 1, y, x - 1)) - (d(l - 1, y, x + 1) - d(l - 1, y, x - 1)))
        dys = 0.25 * ((d(l + 1, y + 1, x) - d(l + 1, y - 1, x)) - (d(l - 1, y + 1, x) - d(l - 1, y - 1, x)))
        c00, c01, c02 = dyy * dss - dys * dys, dxs * dys - dxy * dss, dxy * dys - dxs * dyy
        c11, c12, c22 = dxx * dss - dxs * dxs, dxy * dxs - dxx * dys, dxx * dyy - dxy * dxy
        det = (dxx * c00 + dxy * c01) + dxs * c02
        if det == 0.0:
            return None
        ox = -(((c00 * gx + c01 * gy) + c02 * gs) / det)
        oy = -(((c01 * gx + c11 * gy) + c12 * gs) / det)
        ol = -(((c02 * gx + c12 * gy) + c22 * gs) / det)
        sx, sy, sl = abs(ox) <= 0.5, abs(oy) <= 0.5, abs(ol) <= 0.5
        if sx and sy and sl:
            break
        if moves == 5:
            return None
        moves += 1
        if not sx:
            x += 1 if ox > 0.0 else -1
        if not sy:
            y += 1 if oy > 0.0 else -1
        if not sl:
            l += 1 if ol > 0.0 else -1
        if x < 1 or x > w - 2 or y < 1 or y > h - 2 or l < 1 or l > S:
            return None
    contrast = v + 0.5 * ((gx * ox + gy * oy) + gs * ol)
    if abs(contrast) < o["dog_threshold"] / float(S):
        return None
    tr, det2 = dxx + dyy, dxx * dyy - dxy * dxy
    if det2 <= 0.0:
        return None
    e = o["edge_threshold"]
    if (tr * tr) / det2 >= ((e + 1.0) * (e + 1.0)) / e:
        return None
    return x, y, l, ox, oy, ol


def candidates(pyr, o):
    """The refined key points in canonical order: dicts with octave, the sample (x, y, l), the offset, sig (the scale inside the
    octave) and the float x, y, sigma."""
    S = o["n_intervals"]
    out = []
    for k, (G, D) in enumerate(pyr):
        oc = o["first_octave"] + k
        scale = 2.0 ** oc
        for l, y, x in extrema(D, o):
            r = refine(D, o, int(x), int(y), int(l))
            if r is None:
                continue
            x1, y1, l1, ox, oy, ol = r
            sig = o["sigma0"] * pow2((float(l1) + ol) / float(S))
            out.append(dict(k=k, octave=oc, x=x1, y=y1, l=l1, ox=ox, oy=oy, ol=ol, sig=sig,
                            xys=np.array([(float(x1) + ox) * scale, (float(y1) + oy) * scale, sig * scale]).astype(F)))
    return out


def _window(L, x, y, R):
    """the samples j = -R .. R, inside i = -R .. R, with a gradient: i, j, gx, gy (fp64), in that order"""
    h, w = L.shape
    jj, ii = np.mgrid[-R:R + 1, -R:R + 1]
    ii, jj = ii.ravel(), jj.ravel()
    px, py = x + ii, y + jj
    ok = (px >= 1) & (px <= w - 2) & (py >= 1) & (py <= h - 2)
    ii, jj, px, py = ii[ok], jj[ok], px[ok], py[ok]
    gx = L[py, px + 1].astype(np.float64) - L[py, px - 1].astype(np.float64)
    gy = L[py + 1, px].astype(np.float64) - L[py - 1, px].astype(np.float64)
    return ii, jj, gx, gy


def orientation_histogram(L, c, o, m):
    sig = c["sig"]
    R = int(math.floor(o["orientation_window"] * (1.5 * sig) + 0.5))
    ii, jj, gx, gy = _window(L, c["x"], c["y"], R)
    ok = ii * ii + jj * jj <= R * R
    ii, jj, gx, gy = ii[ok], jj[ok], gx[ok], gy[ok]
    ddx, ddy, s = ii - c["ox"], jj - c["oy"], 1.5 * sig
    wgt = m.exp(-((ddx * ddx + ddy * ddy) / (2.0 * (s * s))))
    mag = m.sqrt(gx * gx + gy * gy)
    a = m.atan2(gy, gx)
    a = np.where(a < 0.0, a + TWO_PI, a)
    b = np.minimum((a * (36.0 / TWO_PI)).astype(np.int64), 35)
    hist = np.zeros(36)
    np.add.at(hist, b, mag * wgt)              # unbuffered: every bin in sample order
    return hist


def orientation_peaks(hist, max_ori):
    h = [float(v) for v in hist]
    for _ in range(2):
        h = [((h[(k + 35) % 36] + h[k]) + h[(k + 1) % 36]) / 3.0 for k in range(36)]
    top = max(h)
    if not top > 0.0:
        return []
    peaks = [k for k in range(36) if h[k] > h[(k + 35) % 36] and h[k] > h[(k + 1) % 36] and h[k] >= 0.8 * top]
    peaks.sort(key=lambda k: (-h[k], k))
    out = []
    for k in peaks[:max_ori]:
        a, b, c = h[(k + 35) % 36], h[k], h[(k + 1) % 36]
        t = ((float(k) + 0.5) + (0.5 * (a - c)) / ((a - 2.0 * b) + c)) * (TWO_PI / 36.0)
        if t < 0.0:
            t = t + TWO_PI
        if t >= TWO_PI:
            t = t - TWO_PI
        out.append(t)
    return out


def descriptor_bins(L, c, theta, m):
    """the 128 sums before the normalisation; theta: the float orientation"""
    sig = c["sig"]
    theta = float(F(theta))
    ct, st = float(m.cos(theta)), float(m.sin(theta))
    hw = 3.0 * sig
    R = int(math.floor(hw * 1.4142135623730951 * 2.5 + 0.5))
    ii, jj, gx, gy = _window(L, c["x"], c["y"], R)
    ddx, ddy = ii - c["ox"], jj - c["oy"]
    rx, ry = (ct * ddx + st * ddy) / hw, (ct * ddy - st * ddx) / hw
    cb, rb = rx + 1.5, ry + 1.5
    ok = (rb > -1.0) & (rb < 4.0) & (cb > -1.0) & (cb < 4.0)
    gx, gy, rx, ry, cb, rb = gx[ok], gy[ok], rx[ok], ry[ok], cb[ok], rb[ok]
    mag = m.sqrt(gx * gx + gy * gy)
    a = m.atan2(gy, gx) - theta
    a = np.where(a < 0.0, a + TWO_PI, a)
    a = np.where(a < 0.0, a + TWO_PI, a)
    a = np.where(a >= TWO_PI, a - TWO_PI, a)
    ob = a * (8.0 / TWO_PI)
    wgt = m.exp(-((rx * rx + ry * ry) / 8.0))
    v = mag * wgt
    r0, c0, o0 = np.floor(rb), np.floor(cb), np.floor(ob)
    fr, fc, fo = rb - r0, cb - c0, ob - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64) & 7
    idx, val, use = [], [], []
    for dr in (0, 1):
        for dc in (0, 1):
            for do in (0, 1):
                r, cc, oo = r0 + dr, c0 + dc, (o0 + do) & 7
                idx.append((4 * r + cc) * 8 + oo)
                val.append(((v * (fr if dr else 1.0 - fr)) * (fc if dc else 1.0 - fc)) * (fo if do else 1.0 - fo))
                use.append((r >= 0) & (r <= 3) & (cc >= 0) & (cc <= 3))
    idx, val, use = np.stack(idx, 1), np.stack(val, 1), np.stack(use, 1)     # [samples, 8]: flattened sample by sample
    acc = np.zeros(128)
    np.add.at(acc, idx[use], val[use])
    return acc


def descriptor_bytes(acc, m):
    n2 = float(np.cumsum(acc * acc)[-1])                                     # left to right
    if not n2 > 0.0:
        return np.zeros(128, np.uint8)
    v = np.minimum(acc / float(m.sqrt(n2)), 0.2)
    v = v / float(m.sqrt(float(np.cumsum(v * v)[-1])))
    return np.minimum(np.floor(512.0 * v + 0.5), 255.0).astype(np.uint8)


def describe(pyr, cands, o, m=None):
    """per candidate: [(theta float32, bytes uint8 [128])], the larger peak first"""
    m = m or Libm()
    out = []
    for c in cands:
        L = pyr[c["k"]][0][c["l"]]
        thetas = orientation_peaks(orientation_histogram(L, c, o, m), o["max_orientations"])
        out.append([(F(t), descriptor_bytes(descriptor_bins(L, c, F(t), m), m)) for t in thetas])
    return out


def assemble(cands, feats, o):
    """(keypoints [n, 4] float32, descriptors [n, 128] uint8, count before the cap, candidate of each row)"""
    kp, ds, src = [], [], []
    for n, (c, f) in enumerate(zip(cands, feats)):
        for t, b in f:
            kp.append(np.array([c["xys"][0], c["xys"][1], c["xys"][2], t], F))
            ds.append(b)
            src.append(n)
    count = len(kp)
    kp = np.array(kp, F).reshape(-1, 4)
    ds = np.array(ds, np.uint8).reshape(-1, 128)
    src = np.array(src, np.int64)
    if count > o["max_features"]:
        keep = np.sort(np.argsort(-kp[:, 2].astype(np.float64), kind="stable")[:o["max_features"]])
        kp, ds, src = kp[keep], ds[keep], src[keep]
    return kp, ds, count, src


def extract(img, o, taps, with_fragile=False):
    """The features of one image.  with_fragile: also the fragile mask per candidate and the largest orientation difference
    between the two evaluations over the others."""
    pyr = pyramid(img, o, taps)
    cands = candidates(pyr, o)
    feats = describe(pyr, cands, o)
    kp, ds, count, src = assemble(cands, feats, o)
    if not with_fragile:
        return kp, ds, count
    other = describe(pyr, cands, o, Libm(perturb=True))
    fragile = np.zeros(len(cands), bool)
    dtheta = 0.0
    for n, (a, b) in enumerate(zip(feats, other)):
        fragile[n] = len(a) != len(b) or any((x[1] != y[1]).any() for x, y in zip(a, b))
        if not fragile[n]:
            for x, y in zip(a, b):
                d = abs(float(x[0]) - float(y[0]))
                dtheta = max(dtheta, min(d, TWO_PI - d))
    return dict(keypoints=kp, descriptors=ds, count=count, source=src, candidates=cands, features=feats, fragile=fragile,
                dtheta=dtheta, pyramid=pyr)
