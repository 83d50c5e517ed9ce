// place_check.cpp -- csrc/place_device.h compiled for the host (tests/test_place_host.py): the descriptor of a cloud and the
// search over descriptors in plain loops, with the header's own arithmetic, comparisons and selection.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>
#include "../global-lvba_amd/csrc/place_device.h"

using namespace lvba;

extern "C" {

struct emul_opts { // lvba_place_opts without the header
    int32_t n_rings, n_sectors;
    double min_range, max_range, z_offset;
    int32_t submap_size, min_gap, n_key_candidates, max_per_frame, query_stride, pad;
    double max_distance;
};

static PlaceParams params(const emul_opts *o)
{
    PlaceParams p;
    p.n_rings = o->n_rings; p.n_sectors = o->n_sectors; p.submap_size = o->submap_size; p.min_gap = o->min_gap;
    p.n_key = o->n_key_candidates; p.max_per_frame = o->max_per_frame; p.query_stride = o->query_stride;
    p.min_range = o->min_range; p.max_range = o->max_range; p.z_offset = o->z_offset; p.max_distance = o->max_distance;
    return p;
}

// xyz [n][3]; cell [n] (-1: dropped), h [n]; D [Nr][Ns], key [Nr]
void emul_descriptor(int64_t n, const float *xyz, const emul_opts *o, int32_t *cell, float *h, float *D, float *key)
{
    const PlaceParams p = params(o);
    for (int c = 0; c < p.n_rings * p.n_sectors; ++c) D[c] = 0.0f;
    for (int64_t i = 0; i < n; ++i) {
        h[i] = 0.0f;
        cell[i] = place_bin(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], p, &h[i]);
        if (cell[i] >= 0 && h[i] > D[cell[i]]) D[cell[i]] = h[i];
    }
    for (int r = 0; r < p.n_rings; ++r) key[r] = place_ring_key(D + r * p.n_sectors, p.n_sectors);
}

// desc [n][Nr][Ns]; out_* [capacity]; returns the true number of candidates
int64_t emul_search(int n, const float *desc, const emul_opts *o, int64_t capacity, int32_t *out_query, int32_t *out_submap,
                    int32_t *out_ref, int32_t *out_shift, double *out_distance, double *out_yaw)
{
    const PlaceParams p = params(o);
    const int nr = p.n_rings, ns = p.n_sectors, cells = nr * ns, K = p.n_key, S = p.submap_size;
    std::vector<float> key((size_t)n * nr);
    std::vector<double> U((size_t)n * cells);
    std::vector<uint64_t> mask(2 * (size_t)n, 0);
    for (int f = 0; f < n; ++f) {
        for (int r = 0; r < nr; ++r) key[(size_t)f * nr + r] = place_ring_key(desc + (size_t)f * cells + r * ns, ns);
        for (int j = 0; j < ns; ++j)
            if (place_column(desc + (size_t)f * cells, nr, ns, j, U.data() + (size_t)f * cells)) mask[2 * f + (j >> 6)] |= (uint64_t)1 << (j & 63);
    }
    int64_t total = 0;
    for (int j = 0; j < n; j += p.query_stride) {
        PlaceKey top[PLACE_MAX_K];
        int kept = 0;
        for (int f = 0; f < n; ++f) {
            const int f0 = f / S * S, f1 = f0 + S < n ? f0 + S : n;
            if (loop_gap_ok(j, f0, f1, p.min_gap)) place_keep(top, &kept, K, place_key_d2(&key[(size_t)j * nr], &key[(size_t)f * nr], nr), f);
        }
        int32_t pick[PLACE_MAX_K], shift[PLACE_MAX_K];
        double dist[PLACE_MAX_K];
        uint8_t eligible[PLACE_MAX_K], keep[PLACE_MAX_K];
        for (int k = 0; k < K; ++k) {
            pick[k] = k < kept ? top[k].idx : -1;
            dist[k] = 1.0; shift[k] = 0;
            if (pick[k] < 0) continue;
            LoopBest b = loop_none();
            for (int s = 0; s < ns; ++s) {
                const double d = place_dist_at(&U[(size_t)j * cells], &U[(size_t)pick[k] * cells], &mask[2 * j], &mask[2 * pick[k]], nr, ns, s);
                if (loop_less(d, s, b.d2, b.idx)) { b.d2 = d; b.idx = s; }
            }
            dist[k] = b.d2; shift[k] = b.idx;
        }
        for (int k = 0; k < K; ++k) eligible[k] = place_eligible(k, K, pick, dist, S, p.max_distance);
        for (int k = 0; k < K; ++k) keep[k] = place_kept(k, K, pick, dist, eligible, S, p.max_per_frame);
        int n_keep = 0;
        for (int k = 0; k < K; ++k) n_keep += keep[k];
        for (int k = 0; k < K; ++k) {
            if (!keep[k]) continue;
            const int64_t at = total + place_slot(k, K, pick, keep, S);
            if (at >= capacity) continue;
            out_query[at] = j; out_submap[at] = pick[k] / S; out_ref[at] = pick[k]; out_shift[at] = shift[k];
            out_distance[at] = dist[k]; out_yaw[at] = place_yaw(shift[k], ns);
        }
        total += n_keep;
    }
    return total;
}

} // extern "C"
