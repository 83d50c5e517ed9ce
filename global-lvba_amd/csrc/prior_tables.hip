// prior_tables.hip -- see prior_tables.h.  The model is in prior_device.h / visual_prior_device.h, the passes in priors.hip /
// visual_priors.hip.  Host logic only.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>

#include "prior_tables.h"

#define fail lvba_fail

namespace lvba {

// ------------------------------------------------------------------------------------------ argument checks
static bool prior_rot_ok(const double *R)
{
    for (int a = 0; a < 9; ++a)
        if (!isfinite(R[a])) return false;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b] - (a == b ? 1.0 : 0.0);
            if (!(fabs(d) <= 1e-6)) return false;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return det > 0.0;
}
static bool prior_is_zero(const double *o)
{
    for (int a = 0; a < 12; ++a)
        if (o[a] != 0.0) return false;
    return true;
}
void prior_offset_or_identity(const double *o, double *out) // twelve zeros: the identity
{
    static const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    memcpy(out, prior_is_zero(o) ? I : o, 12 * sizeof(double));
}
static int32_t prior_check_one(const lvba_prior &q, int32_t N, int32_t k)
{
    if (q.kind < LVBA_PRIOR_POSE || q.kind > LVBA_PRIOR_RELATIVE) return fail(LVBA_ERR_ARG, "prior %d: unknown kind %d", k, q.kind);
    const bool rel = q.kind == LVBA_PRIOR_RELATIVE;
    if (q.i < 0 || q.i >= N || (rel && (q.j < 0 || q.j >= N))) return fail(LVBA_ERR_ARG, "prior %d: pose index out of range [0,%d)", k, N);
    if (rel && q.i == q.j) return fail(LVBA_ERR_ARG, "prior %d: a relative prior needs two different poses", k);
    const int m = q.kind == LVBA_PRIOR_POSITION ? 3 : 6;
    for (int a = 0; a < m; ++a)
        for (int b = 0; b < m; ++b)
            if (!isfinite(q.sqrt_info[6 * a + b])) return fail(LVBA_ERR_ARG, "prior %d: non-finite sqrt_info", k);
    for (int a = q.kind == LVBA_PRIOR_POSITION ? 9 : 0; a < 12; ++a)
        if (!isfinite(q.meas[a])) return fail(LVBA_ERR_ARG, "prior %d: non-finite measurement", k);
    if (q.kind != LVBA_PRIOR_POSITION && !prior_rot_ok(q.meas)) return fail(LVBA_ERR_ARG, "prior %d: the measured rotation is not orthonormal", k);
    for (int s = 0; s < (rel ? 2 : 1); ++s) {
        const double *o = s ? q.offset_j : q.offset_i;
        if (prior_is_zero(o)) continue;
        for (int a = 9; a < 12; ++a)
            if (!isfinite(o[a])) return fail(LVBA_ERR_ARG, "prior %d: non-finite offset", k);
        if (!prior_rot_ok(o)) return fail(LVBA_ERR_ARG, "prior %d: an offset rotation is not orthonormal", k);
    }
    return LVBA_OK;
}
int32_t prior_validate(int32_t n, const lvba_prior *priors, int32_t n_poses)
{
    if (n < 0 || (n > 0 && !priors)) return fail(LVBA_ERR_ARG, "n must be >= 0 and priors non-NULL");
    for (int32_t k = 0; k < n; ++k) TRY(prior_check_one(priors[k], n_poses, k));
    return LVBA_OK;
}

int32_t prior_cap(int32_t n)
{
    if (n > (1 << 22)) return fail(LVBA_ERR_ARG, "more than 2^22 priors");
    return LVBA_OK;
}

int32_t prior_pairs_in_store(const BlockSys &bs, int32_t n, const lvba_prior *priors, const lvba::hvec<int64_t> *slots_a,
                             const lvba::hvec<int64_t> *slots_b, const char *what, const char *call)
{
    for (int32_t k = 0; k < n; ++k) {
        if (priors[k].kind != LVBA_PRIOR_RELATIVE) continue;
        const int32_t I = bs.iperm[(size_t)priors[k].i], J = bs.iperm[(size_t)priors[k].j];
        const int32_t lo = std::min(I, J), hi = std::max(I, J);
        bool ok = hi - lo <= bs.Bb;
        if (ok && (slots_a || slots_b)) {
            const int64_t slot = (int64_t)lo * (bs.Bb + 1) + (hi - lo);
            ok = (slots_a && std::binary_search(slots_a->begin(), slots_a->end(), slot)) ||
                 (slots_b && std::binary_search(slots_b->begin(), slots_b->end(), slot));
        }
        if (!ok) return fail(LVBA_ERR_STATE, "prior %d joins %s %d and %d, which are no block of the store laid out at the first "
                             "cost / %s / refine call: set such priors before it", k, what, priors[k].i, priors[k].j, call);
    }
    return LVBA_OK;
}

void prior_store(BlockSys &bs, bool finalized, int32_t n, const lvba_prior *priors, std::vector<lvba_prior> &stored)
{
    stored.assign(priors, priors + n);
    for (lvba_prior &q : stored) {
        q.reserved = 0;
        if (q.kind != LVBA_PRIOR_RELATIVE) { q.j = 0; memset(q.offset_j, 0, sizeof q.offset_j); }
    }
    if (finalized) return;
    bs.edge_i.clear(); bs.edge_j.clear();
    for (const lvba_prior &q : stored)
        if (q.kind == LVBA_PRIOR_RELATIVE) { bs.edge_i.push_back(q.i); bs.edge_j.push_back(q.j); }
}

int64_t prior_hash(const std::vector<lvba_prior> &stored)
{
    uint64_t hs = 1469598103934665603ull;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(stored.data());
    for (size_t a = 0; a < stored.size() * sizeof(lvba_prior); ++a) { hs ^= b[a]; hs *= 1099511628211ull; }
    return (int64_t)(hs >> 2);
}

// ------------------------------------------------------------------------------------------ device tables
void PriorTables::free_mem()
{
    for (void *p : mem) lvba::DevicePool::get().free(p);
    mem.clear();
}

int32_t PriorTables::release(BlockSys &bs)
{
    HIPCHK(hipSetDevice(bs.device));
    launch_prior_zero_slots(bs.Hblk(), d_wslot, n_wslot, bs.stream); // what only the old priors filled
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(bs.stream));
    free_mem();
    dev = PriorDev{};
    d_wslot = nullptr;
    n_wslot = 0;
    return LVBA_OK;
}

template <typename T>
static int32_t prior_upload(BlockSys &bs, std::vector<void *> &mem, T **p, size_t n, const T *src)
{
    TRY(bs_dmalloc(bs, p, (int64_t)n));
    mem.push_back(*p);
    if (src && n) HIPCHK(lvba::copy_h2d(*p, src, n * sizeof(T)));
    return LVBA_OK;
}

int32_t PriorTables::bind(BlockSys &bs, const std::vector<lvba_prior> &priors, const lvba::hvec<int64_t> &other_slots, bool all_add,
                          int n_sums, lvba::hvec<int64_t> *offdiag)
{
    const int32_t n = (int32_t)priors.size();
    const int64_t Bb1 = (int64_t)bs.Bb + 1;
    std::vector<PriorRec> rec((size_t)n);
    std::map<int64_t, std::vector<int32_t>> hb; // slot -> contributions, ascending prior index
    std::map<int32_t, std::vector<int32_t>> gb; // solver pose -> contributions
    for (int32_t k = 0; k < n; ++k) {
        const lvba_prior &q = priors[(size_t)k];
        PriorRec &r = rec[(size_t)k];
        const bool rel = q.kind == LVBA_PRIOR_RELATIVE;
        r.kind = q.kind;
        r.I = bs.iperm[(size_t)q.i];
        r.J = rel ? bs.iperm[(size_t)q.j] : r.I;
        r.flip = r.I < r.J ? 1 : 0;
        memcpy(r.meas, q.meas, sizeof r.meas);
        prior_offset_or_identity(q.offset_i, r.oi);
        prior_offset_or_identity(q.offset_j, r.oj);
        memcpy(r.L, q.sqrt_info, sizeof r.L);
        hb[(int64_t)r.I * Bb1].push_back(k << 2);
        gb[r.I].push_back(k << 2);
        if (rel) {
            hb[(int64_t)r.J * Bb1].push_back(k << 2 | 1);
            gb[r.J].push_back(k << 2 | 1);
            const int32_t lo = std::min(r.I, r.J), hi = std::max(r.I, r.J);
            hb[(int64_t)lo * Bb1 + (hi - lo)].push_back(k << 2 | 2);
        }
    }
    lvba::hvec<int64_t> hslot, wslot;
    lvba::hvec<int32_t> hmode, hoff(1, 0), hsrc, gpose, goff(1, 0), gsrc;
    for (const auto &t : hb) {
        const bool diag = t.first % Bb1 == 0;
        const bool add = diag || all_add || std::binary_search(other_slots.begin(), other_slots.end(), t.first);
        hslot.push_back(t.first);
        hmode.push_back((add ? 0 : 1) | (diag ? 2 : 0));
        if (!add) wslot.push_back(t.first);
        if (!diag && offdiag) offdiag->push_back(t.first);
        hsrc.insert(hsrc.end(), t.second.begin(), t.second.end());
        hoff.push_back((int32_t)hsrc.size());
    }
    for (const auto &t : gb) {
        gpose.push_back(t.first);
        gsrc.insert(gsrc.end(), t.second.begin(), t.second.end());
        goff.push_back((int32_t)gsrc.size());
    }
    PriorRec *d_rec = nullptr;
    double *d_lin = nullptr, *d_part = nullptr;
    unsigned *d_ticket = nullptr;
    int64_t *d_hslot = nullptr;
    int32_t *d_hmode = nullptr, *d_hoff = nullptr, *d_hsrc = nullptr, *d_gpose = nullptr, *d_goff = nullptr, *d_gsrc = nullptr;
    TRY(prior_upload(bs, mem, &d_rec, rec.size(), rec.data()));
    TRY(prior_upload<double>(bs, mem, &d_lin, 128 * (size_t)n, nullptr));
    TRY(prior_upload<double>(bs, mem, &d_part, (size_t)n_sums * ((size_t)(n + 63) / 64), nullptr));
    const unsigned zero = 0;
    TRY(prior_upload(bs, mem, &d_ticket, 1, &zero));
    TRY(prior_upload(bs, mem, &d_hslot, hslot.size(), hslot.data()));
    TRY(prior_upload(bs, mem, &d_hmode, hmode.size(), hmode.data()));
    TRY(prior_upload(bs, mem, &d_hoff, hoff.size(), hoff.data()));
    TRY(prior_upload(bs, mem, &d_hsrc, hsrc.size(), hsrc.data()));
    TRY(prior_upload(bs, mem, &d_gpose, gpose.size(), gpose.data()));
    TRY(prior_upload(bs, mem, &d_goff, goff.size(), goff.data()));
    TRY(prior_upload(bs, mem, &d_gsrc, gsrc.size(), gsrc.data()));
    if (!wslot.empty()) TRY(prior_upload(bs, mem, &d_wslot, wslot.size(), wslot.data()));
    n_wslot = (int64_t)wslot.size();
    PriorDev &d = dev;
    d.pr = d_rec; d.lin = d_lin; d.part = d_part; d.ticket = d_ticket;
    d.n_hblk = (int64_t)hslot.size(); d.hslot = d_hslot; d.hmode = d_hmode; d.hoff = d_hoff; d.hsrc = d_hsrc;
    d.n_g = (int32_t)gpose.size(); d.gpose = d_gpose; d.goff = d_goff; d.gsrc = d_gsrc;
    d.n = n; // (last: a failed upload above leaves a handle without priors)
    return LVBA_OK;
}

} // namespace lvba
