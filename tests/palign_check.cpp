// palign_check.cpp -- csrc/palign_device.h compiled for the host (tests/test_palign_host.py): the per-sample records, the sums,
// the damped solve and the per-image iteration, walked the way the kernels of palign.hip walk them, with the header's own
// functions.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include "../global-lvba_amd/csrc/palign_device.h"

using namespace lvba;

namespace {

struct Image { const uint8_t *bgr; int w; };
inline uint32_t texel_of(const Image &im, int y, int x) { return photo_texel_of(im.bgr + 3 * ((int64_t)y * im.w + x)); }

// the sums of one image at (R, t): a lane's walk over all points in index order
void sums_at(int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid, int w, int h, const float *depth, const double *R,
             const double *t, const uint8_t *bgr, const TrkIntr &cam, const PhotoRule &o, int loss_kind, double loss_scale, double *s)
{
    const Image im{bgr, w};
    for (int q = 0; q < PAL_NS; ++q) s[q] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (!valid[i]) continue;
        const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        pal_point(cam, depth, w, h, R, t, X, ref16 + 3 * i, o, loss_kind, loss_scale, [&](int y, int x) { return texel_of(im, y, x); }, s);
    }
}

} // namespace

extern "C" {

// bounds: occlusion_rel, occlusion_abs, max_depth, loss_scale; flags: holes, loss_kind.  One image: depth [h][w] or null, bgr
// [h][w][3].  Per point: seen, and where seen c16 [3], gu, gv, r [3], J [3][6], rho, wt [3] (untouched elsewhere); sums [31] as
// sums_at adds them.
void emul_records(int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid, int w, int h, const float *depth,
                  const double *R, const double *t, const uint8_t *bgr, const double *intr, const double *bounds, const int32_t *flags,
                  uint8_t *seen, int32_t *c16, double *gu, double *gv, double *r, double *J, double *rho, double *wt, double *sums)
{
    const TrkIntr cam = trk_intr_of(intr);
    const PhotoRule o = photo_rule_of(depth != nullptr, bounds[0], bounds[1], bounds[2], flags[0], 2);
    const Image im{bgr, w};
    for (int64_t i = 0; i < n; ++i) {
        seen[i] = 0;
        if (!valid[i]) continue;
        const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        double u, v;
        if (!photo_locate(cam, depth, w, h, R, t, X, o, u, v)) continue;
        seen[i] = 1;
        const PhotoTap p = photo_tap(u, v, [&](int y, int x) { return texel_of(im, y, x); });
        double Xc[3], Ju[3], Jv[3];
        pal_camera_point(R, t, X, Xc);
        pal_jpi(cam, Xc, Ju, Jv);
        for (int k = 0; k < 3; ++k) {
            const PalColour c = pal_colour(p, k);
            double rr, row[6], rh[3];
            pal_channel(c, ref16[3 * i + k], Xc, Ju, Jv, flags[1], bounds[3], rr, row, rh);
            c16[3 * i + k] = c.c16; gu[3 * i + k] = c.gu; gv[3 * i + k] = c.gv; r[3 * i + k] = rr;
            for (int a = 0; a < 6; ++a) J[6 * (3 * i + k) + a] = row[a];
            rho[3 * i + k] = rh[0]; wt[3 * i + k] = rh[1];
        }
    }
    sums_at(n, xyz, ref16, valid, w, h, depth, R, t, bgr, cam, o, flags[1], bounds[3], sums);
}

// the gradient numerators of channel k from four texel words and the fractions (a, b)
void emul_gradient(int32_t a, int32_t b, uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11, int k, int32_t *nu, int32_t *nv)
{
    const PhotoTap p{a, b, t00, t10, t01, t11};
    pal_gradient_num(p, k, *nu, *nv);
}

// Ju, Jv [3] at Xc
void emul_jpi(const double *intr, const double *Xc, double *Ju, double *Jv) { pal_jpi(trk_intr_of(intr), Xc, Ju, Jv); }

// trk_project_cam at Xc: 1 and (u, v), or 0
int emul_project_cam(const double *intr, const double *Xc, double *uv)
{
    return trk_project_cam(trk_intr_of(intr), Xc[0], Xc[1], Xc[2], uv[0], uv[1]) ? 1 : 0;
}

int emul_solve(const double *sums, double lambda, double *d) { return pal_solve(sums, lambda, d) ? 1 : 0; }

void emul_retract(const double *R, const double *t, const double *d, double *Rn, double *tn) { pal_retract(R, t, d, Rn, tn); }

// The iteration of one image as palign_step_kernel runs it.  par: loss_scale, eps_rot, eps_trans, max_chord_sq, max_translation;
// ipar: loss_kind, min_samples, max_iterations.  out_i: status, passes, accepted; out_d: R [9], t [3], cur [31], first [31].
void emul_align(int64_t n, const float *xyz, const uint16_t *ref16, const uint8_t *valid, int w, int h, const float *depth, const double *R0,
                const double *t0, const uint8_t *bgr, const double *intr, const double *bounds, const int32_t *flags, const double *par,
                const int32_t *ipar, int32_t *out_i, double *out_d)
{
    const TrkIntr cam = trk_intr_of(intr);
    const PhotoRule o = photo_rule_of(depth != nullptr, bounds[0], bounds[1], bounds[2], flags[0], 2);
    const PalParams pp{par[0], par[1], par[2], par[3], par[4], ipar[0], ipar[1], ipar[2], 0};
    PalState st;
    pal_state_init(st, R0, t0);
    while (st.status == PAL_RUNNING) {
        double s[PAL_NS];
        sums_at(n, xyz, ref16, valid, w, h, depth, st.Rt, st.tt, bgr, cam, o, pp.loss_kind, pp.loss_scale, s);
        st.status = pal_step(s, pp, st);
    }
    out_i[0] = st.status; out_i[1] = st.passes; out_i[2] = st.accepted;
    for (int e = 0; e < 9; ++e) out_d[e] = st.R[e];
    for (int e = 0; e < 3; ++e) out_d[9 + e] = st.t[e];
    for (int q = 0; q < PAL_NS; ++q) { out_d[12 + q] = st.cur[q]; out_d[12 + PAL_NS + q] = st.first[q]; }
}

} // extern "C"
