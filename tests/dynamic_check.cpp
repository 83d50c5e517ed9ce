// dynamic_check.cpp -- csrc/dynamic_device.h compiled for the host (tests/test_dynamic_host.py): the range images, the dilation,
// the votes and the labels of a scan set in plain loops, with the header's own arithmetic and comparisons.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../global-lvba_amd/csrc/dynamic_device.h"

using namespace lvba;

extern "C" {

struct emul_opts { // lvba_dynamic_opts without the header
    int32_t n_rows, n_cols, halo, window, min_free, batch_frames;
    double el_min, el_max, min_range, max_range, abs_tol, rel_tol, free_ratio;
};

static DynParams params(const emul_opts *o)
{
    DynParams p;
    p.n_rows = o->n_rows; p.n_cols = o->n_cols; p.halo = o->halo; p.window = o->window; p.min_free = o->min_free;
    p.el_min = o->el_min; p.el_max = o->el_max; p.min_range = o->min_range; p.max_range = o->max_range;
    p.abs_tol = o->abs_tol; p.rel_tol = o->rel_tol; p.free_ratio = o->free_ratio;
    return p;
}

// one frame: xyz [n][3]; cell [n] (-1: none); I, M [n_rows][n_cols]
void emul_image(int64_t n, const float *xyz, const emul_opts *o, int32_t *cell, float *I, float *M)
{
    const DynParams p = params(o);
    const int cells = p.n_rows * p.n_cols;
    std::vector<uint32_t> bits((size_t)cells, DYN_EMPTY_BITS);
    for (int64_t i = 0; i < n; ++i) {
        double r = 0.0;
        cell[i] = dyn_cell((double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], p, &r);
        if (cell[i] < 0) continue;
        const float rf = (float)r;
        uint32_t b;
        memcpy(&b, &rf, 4);
        if (b < bits[(size_t)cell[i]]) bits[(size_t)cell[i]] = b; // the integer minimum of the device
    }
    memcpy(I, bits.data(), 4 * (size_t)cells);
    for (int c = 0; c < cells; ++c) M[c] = dyn_dilate(I, p.n_rows, p.n_cols, p.halo, c / p.n_cols, c % p.n_cols);
}

// frames with offsets off [n_frames + 1] into xyz, poses [n_frames][12]; label, n_free, n_support [off[n_frames]];
// the dilated images are made batch frames at a time, as the device makes them
void emul_labels(int n_frames, const int64_t *off, const float *xyz, const double *poses, const emul_opts *o, int batch, uint8_t *label,
                 int32_t *n_free, int32_t *n_support)
{
    const DynParams p = params(o);
    const int64_t cells = (int64_t)p.n_rows * p.n_cols, P = off[n_frames];
    for (int64_t i = 0; i < P; ++i) n_free[i] = n_support[i] = 0;
    if (batch < 1) batch = n_frames;
    std::vector<float> I((size_t)cells), M((size_t)(cells * batch));
    std::vector<int32_t> cell;
    for (int b0 = 0; b0 < n_frames; b0 += batch) {
        const int b1 = b0 + batch < n_frames ? b0 + batch : n_frames;
        for (int g = b0; g < b1; ++g) {
            cell.assign((size_t)(off[g + 1] - off[g]) + 1, 0);
            emul_image(off[g + 1] - off[g], xyz + 3 * off[g], o, cell.data(), I.data(), M.data() + (size_t)(cells * (g - b0)));
        }
        for (int f = 0; f < n_frames; ++f) {
            int g0, g1;
            dyn_window(f, n_frames, p.window, &g0, &g1);
            const int ga = g0 > b0 ? g0 : b0, gb = g1 < b1 ? g1 : b1;
            for (int64_t i = off[f]; i < off[f + 1]; ++i) {
                double w[3];
                pose_apply(poses + 12 * f, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], w);
                dyn_votes(w, f, ga, gb, poses, M.data(), b0, cells, p, &n_free[i], &n_support[i]);
            }
        }
    }
    for (int64_t i = 0; i < P; ++i) label[i] = dyn_label(n_free[i], n_support[i], p);
}

} // extern "C"
