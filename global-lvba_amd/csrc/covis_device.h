// covis_device.h -- scalar pieces of the co-visibility pair selection (covis.hip; the rule is in include/lvba_hip.h, DESIGN.md
// §10i): the sample of a grid cell through the image's own depth image, "seen in j" with the occlusion test against j's depth
// image, the score of a pair and the order of the cap.  Host/device-neutral, like match_device.h and fusion_device.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include "tracks_device.h"
#include "fusion_device.h"

namespace lvba {

constexpr int COVIS_MAX_GRID = 64;        // cells per axis
constexpr int COVIS_MAX_RADIUS = 16;      // Chebyshev rings of the search for a pixel with a depth return
constexpr int COVIS_MAX_PER_IMAGE = 1024; // the cap
constexpr int COVIS_MAX_IMAGES = 8192;    // the count matrix is [M][M] int32: 256 MB here

struct CovisRule {
    int32_t occlusion, both_ways, max_per_image, min_shared;
    double min_overlap, occlusion_rel, occlusion_abs;
};

// centre pixel of cell g of `cells` along an axis of `size` pixels: 0 <= centre <= size - 2
LVBA_TRK_FN int covis_centre(int g, int cells, int size) { return ((2 * g + 1) * (size - 1)) / (2 * cells); }

// one candidate pixel of a cell: its world point through the image's own depth image; false (X untouched) outside
// [0, w - 2] x [0, h - 2], where the undistortion fails, without a depth return, or for a point that is not finite
LVBA_TRK_FN bool covis_candidate(const float *__restrict__ depth, int w, int h, const TrkIntr &cam, int u, int v,
                                 const double *__restrict__ R, const double *__restrict__ t, double *__restrict__ X)
{
    if (u < 0 || v < 0 || u > w - 2 || v > h - 2) return false;
    const float uf = (float)u, vf = (float)v;
    double x, y, p[3];
    if (!trk_undistort(cam, (double)uf, (double)vf, x, y)) return false;
    if (!depth_world_point(depth, w, h, uf, vf, x, y, R, t, p)) return false;
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) return false;
    X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
    return true;
}

// The sample of the cell with centre (px, py): the centre, then the rings r = 1 .. radius, each walked dy = -r .. r and inside
// that dx = -r .. r over the pixels with |dx| = r or |dy| = r; the first candidate with a point.  Returns the ring it was found
// on, or -1 with X = NaN when the cell has no point.
LVBA_TRK_FN int covis_sample(const float *__restrict__ depth, int w, int h, const TrkIntr &cam, int px, int py, int radius,
                             const double *__restrict__ R, const double *__restrict__ t, double *__restrict__ X)
{
    if (covis_candidate(depth, w, h, cam, px, py, R, t, X)) return 0;
    for (int r = 1; r <= radius; ++r)
        for (int dy = -r; dy <= r; ++dy) {
            const int step = (dy == -r || dy == r) ? 1 : 2 * r; // the two full rows of the ring, else its two end pixels
            for (int dx = -r; dx <= r; dx += step)
                if (covis_candidate(depth, w, h, cam, px + dx, py + dy, R, t, X)) return r;
        }
    X[0] = X[1] = X[2] = NAN;
    return -1;
}

// what became of a sample of image i in image j
enum CovisFate : int { COVIS_NO_POINT = 0, COVIS_BEHIND = 1, COVIS_OUTSIDE = 2, COVIS_HIDDEN = 3, COVIS_SEEN_HOLE = 4, COVIS_SEEN = 5 };

// (Rj, tj) = T_cam<-world of j, depth_j its depth image.  A fetch that fails is a hole in j: no evidence of occlusion.
LVBA_TRK_FN int covis_fate(const TrkIntr &cam, const float *__restrict__ depth_j, int w, int h, const double *__restrict__ Rj,
                           const double *__restrict__ tj, const double *__restrict__ X, const CovisRule &o)
{
    if (X[0] != X[0]) return COVIS_NO_POINT;
    double u, v;
    if (!trk_project(cam, Rj, tj, X, u, v)) return COVIS_BEHIND;
    if (!(u >= 0.0 && u < (double)(w - 1) && v >= 0.0 && v < (double)(h - 1))) return COVIS_OUTSIDE;
    if (!o.occlusion) return COVIS_SEEN;
    float d;
    if (!fetch_depth_bilinear(depth_j, w, h, (float)u, (float)v, d)) return COVIS_SEEN_HOLE;
    const double Z = Rj[6] * X[0] + Rj[7] * X[1] + Rj[8] * X[2] + tj[2]; // the expression trk_project evaluates
    return Z > (double)d * (1.0 + o.occlusion_rel) + o.occlusion_abs ? COVIS_HIDDEN : COVIS_SEEN;
}
LVBA_TRK_FN bool covis_seen(const TrkIntr &cam, const float *__restrict__ depth_j, int w, int h, const double *__restrict__ Rj,
                            const double *__restrict__ tj, const double *__restrict__ X, const CovisRule &o)
{
    return covis_fate(cam, depth_j, w, h, Rj, tj, X, o) >= COVIS_SEEN_HOLE;
}

// The unordered pair {i, j} from the two counts and the two sample numbers; symmetric in its images.
struct CovisPair { double score; int32_t shared; bool eligible; };

LVBA_TRK_FN CovisPair covis_pair(int32_t c_ij, int32_t c_ji, int32_t n_i, int32_t n_j, const CovisRule &o)
{
    const double r_ij = n_i > 0 ? (double)c_ij / (double)n_i : 0.0, r_ji = n_j > 0 ? (double)c_ji / (double)n_j : 0.0;
    CovisPair p;
    if (o.both_ways) { p.score = r_ij < r_ji ? r_ij : r_ji; p.shared = c_ij < c_ji ? c_ij : c_ji; }
    else { p.score = r_ij > r_ji ? r_ij : r_ji; p.shared = c_ij > c_ji ? c_ij : c_ji; }
    p.eligible = p.shared >= o.min_shared && p.score >= o.min_overlap;
    return p;
}

// The cap ranks the partners of an image by (score descending, partner index ascending).  CovisRank is a place in that order:
// the first place is before every partner, the last place behind every one.
struct CovisRank { double score; int32_t partner; };
LVBA_TRK_FN CovisRank covis_rank_first() { CovisRank r; r.score = INFINITY; r.partner = -1; return r; }
LVBA_TRK_FN CovisRank covis_rank_last() { CovisRank r; r.score = -INFINITY; r.partner = INT32_MAX; return r; }
LVBA_TRK_FN bool covis_rank_before(const CovisRank &a, const CovisRank &b) // strictly
{
    return a.score > b.score || (a.score == b.score && a.partner < b.partner);
}
// a partner is among the K best of an image iff it is not behind the image's K-th best (the last place where the image has
// fewer than K eligible partners)
LVBA_TRK_FN bool covis_within_cap(double score, int32_t partner, const CovisRank &kth)
{
    CovisRank a; a.score = score; a.partner = partner;
    return !covis_rank_before(kth, a);
}

} // namespace lvba
