// CPU check of global-lvba_amd/csrc/ldlt_layout.h (test infrastructure; compiled by tests/test_ordering.py).
//
// The look-ahead LDL^T loads whole tiles unconditionally and masks afterwards: it is memory-safe iff every offset it forms lies
// inside the store / workspace it was given.  This program replays the launch list of ldlt.hip's run_phase (ldlt_schedule_phase
// + the same `geom` rule) for a list of geometries and, for every role, q_extra product, qx_helper, bulk job (64 x 64 and
// 128 x 64) and forward passenger, forms the largest element offset of every load and store from the tile origin and the loader's
// index expression -- each expression is re-stated ONCE below, next to the kernel line it comes from -- and checks
//   * every offset <= the closed-form reach bound of ldlt_layout.h, every bound < the capacity of ldlt_layout.h's size helper;
//   * for the 128 x 64 tiles, every byte offset < 2^32 whenever ldlt_offsets_fit_32bit admits them;
//   * the workspace: regions disjoint and in order, total = sum, Z-tile over-reads end inside the problem's part;
//   * the sizes are the ones every handle has had so far (the literal formulas below): a change of a handle's memory fails here.
// -DLVBA_LAYOUT_SLACK_LESS must FAIL: the store is then taken one ldab (band) / 64 doubles (dense) smaller -- or, where even the
// tightest geometry of the list leaves more room than that, exactly as small as that geometry's reach.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../global-lvba_amd/csrc/ldlt_layout.h"
#include "../global-lvba_amd/csrc/ldlt_schedule.h"

using namespace lvba;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail < 20) { printf("FAILED line %d: %s  ", __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

// ---- the parent's rules, copied (NOT through the header): what a handle's memory has been so far
static int64_t pinned_store(int64_t n, int64_t ld)
{
    if (ld != n) { const int64_t ldab = ld + 1; return 2 * (ldab * (n + 1)) + 65 * ldab; }
    return n * n + 64 * n + 128;
}
static int64_t pinned_ldz(int64_t n, int64_t bw) { const int64_t w = bw + 64 + 64; return w < n ? w : n; }
static int64_t pinned_ws_one(int64_t n, int64_t bw)
{
    const int64_t nsteps = (n + 64 - 1) / 64;
    return nsteps * 4096 + 3 * n + 4 * pinned_ldz(n, bw) * 64 + 64 + 2 * 4096 + 2 * 4096;
}
static int64_t pinned_workspace(int64_t n, int64_t bw)
{
    return 2 * pinned_ws_one(n, bw) + n + 64 + (std::min<int64_t>(n, bw + 2 * 64) * (bw + 2) + 64) + 8;
}
static bool pinned_32bit(int64_t n, int64_t ld) { return ((uint64_t)ld * (uint64_t)(n + 128) + (uint64_t)n + 256) * 8 < 0xFFFF0000ull; }

struct Geo { int64_t k, w0, rend, T; int nbe; };

// one solve's worth of offsets: the largest formed relative to M.a of a problem, to a Z slot's start, to a 64 x 64 tile's start
struct Replay {
    int64_t n, ld, bw, nf, ldz;
    bool big;
    int64_t store_max = -1, z_max = -1, tile_max = -1, byte_max = -1, g_panel_max = -1;
    Geo geom(int64_t st) const // ldlt.hip: geom in ldlt_solve
    {
        Geo q;
        q.k = st * 64;
        q.nbe = (int)((nf - q.k) < 64 ? (nf - q.k) : 64);
        q.w0 = q.k + q.nbe;
        q.rend = q.k + q.nbe + bw;
        if (q.rend > nf) q.rend = nf;
        q.T = q.w0 < q.rend ? (q.rend - q.w0 + 63) / 64 : 0;
        return q;
    }
    void a(int64_t row, int64_t col) { store_max = std::max(store_max, row + col * ld); }
    void z(int64_t row, int64_t col) { z_max = std::max(z_max, row + col * ldz); }
    void tile() { tile_max = std::max<int64_t>(tile_max, 63 * 64 + 63); } // [(w + 4 it) 64 + row], [(16 w + kk + 4 reg) 64 + 16 t + i]
    // ldlt_lookahead.h:184-187  base = M.a + (r0 + row) + (kc + w) ld; base[it 4 ld], row < 64, w + 4 it < 64 -- unconditional
    void load_panel_tile(int64_t r0, int64_t kc) { a(r0 + 63, kc + 63); }
    // ldlt_lookahead.h:194-197  base = Z + (r0 + row - w0) + w ldz; base[it 4 ldz] -- unconditional
    void load_z_tile(int64_t r0, int64_t w0) { z(r0 + 63 - w0, 63); }
    // ldlt_lookahead.h:204-209  base = M.a + (R0 + i) + (C0 + 16 w + kk) ld; base[16 t + reg 4 ld] -- unconditional
    void load_c_tile(int64_t R0, int64_t C0) { a(R0 + 15 + 48, C0 + 48 + 3 + 12); }
    // ldlt_lookahead.h:230-256  L to M.a + (R0 + i) + (p.k + 16 w + kk) ld, Z to Zp + (R0 + i - p.w0) + (16 w + kk) ldz; the whole
    // tile if it lies inside the window, else the entries with 16 t + i < rend - R0 and column < nbe
    void store_lz_tile(const Geo &p, int64_t R0)
    {
        const int64_t rows = std::min<int64_t>(64, p.rend - R0);
        a(R0 + rows - 1, p.k + p.nbe - 1);
        z(R0 + rows - 1 - p.w0, p.nbe - 1);
    }
    // ldlt_lookahead.h:264-281  M.a + (R0 + i) + (C0 + 16 w + kk) ld: the whole tile if R0 + 64 <= rlim and C0 + 64 <= clim, else
    // the entries with row < rlim - R0, column < clim - C0
    void store_c_tile(int64_t R0, int64_t C0, int64_t rlim, int64_t clim)
    {
        const int64_t rows = std::min<int64_t>(64, rlim - R0), cols = std::min<int64_t>(64, clim - C0);
        if (rows > 0 && cols > 0) a(R0 + rows - 1, C0 + cols - 1);
    }
    void chain_role(const Geo &p, const Geo &q, bool has_q_, bool do_diag, int64_t panel, int64_t nbe_next)
    {
        const int64_t r0 = p.w0;
        if (has_q_ && r0 < q.rend) { // (:297-:304; with a ready-made share, :317, the two loads are skipped: both forms are counted)
            load_panel_tile(r0, q.k);
            load_z_tile(r0, q.w0);
            tile();
        }
        load_panel_tile(r0, p.k); // :305
        tile();                   // :307 Gp[tid + 256 it]
        load_c_tile(r0, r0);      // :344
        store_lz_tile(p, r0);     // :355
        if (!do_diag) { if (nbe_next > 0) a(r0 + nbe_next - 1, r0 + nbe_next - 1); } // :374, rl < nbn && cl <= rl
        else g_panel_max = std::max(g_panel_max, panel + 1);                         // :401 Gn = G of panel p + 1
    }
    void row_role(const Geo &p, const Geo &q, bool has_q_, bool q_extra, bool qx_helper, bool dfr, int64_t t)
    {
        const int64_t r0 = p.w0 + 64 * t, s0 = p.w0; // :424-:425
        const bool use_q = has_q_ && r0 < q.rend, pre = dfr && use_q;
        if (use_q) {
            load_panel_tile(r0, q.k); // :440
            load_z_tile(s0, q.w0);    // :441
            const bool qx = q_extra && !(qx_helper && t == 1);
            if (qx) load_z_tile(s0 + 64, q.w0);  // :477
            if (pre) load_z_tile(q.w0, q.w0);    // :478
            if (dfr) load_c_tile(r0, p.k);       // :469
            else load_panel_tile(r0, p.k);       // :470
            if (qx) {
                load_c_tile(r0, s0 + 64);                      // :490
                store_c_tile(r0, s0 + 64, q.rend, q.rend);     // :497
            }
        } else
            load_panel_tile(r0, p.k); // :443
        tile();                        // :436 Gp, :525 side_r
        load_c_tile(r0, s0);           // :457 (load_cv)
        store_c_tile(r0, s0, p.rend, p.rend); // :485 / :575
        store_lz_tile(p, r0);          // :541 / :562 (lean rows stop here; :582 side_w, :596 dq_w are whole tiles)
    }
    void qx_diag_role(const Geo &p, const Geo &q, bool has_q_)
    {
        const int64_t r0 = p.w0 + 64; // :608
        if (!(has_q_ && r0 < q.rend)) return;
        load_panel_tile(r0, q.k); // :611
        load_z_tile(r0, q.w0);    // :612
        load_c_tile(r0, r0);      // :614
        store_c_tile(r0, r0, q.rend, q.rend); // :622
    }
    // ldlt_tiles.h:23-78, :83-145  update_tile[2]: every access behind r < rend && c < rend (&& m < nbe)
    void update_tile(const Geo &o, int64_t ti, int64_t tj)
    {
        const int64_t r0 = o.w0 + 64 * ti, c0 = o.w0 + 64 * tj;
        a(std::min(r0 + 63, o.rend - 1), o.k + o.nbe - 1);
        z(std::min(c0 + 63, o.rend - 1) - o.w0, o.nbe - 1);
        a(std::min(r0 + 63, o.rend - 1), std::min(c0 + 63, o.rend - 1));
    }
    void bulk_tile_128(const Geo &o, const Geo *e, int64_t R0, int64_t tj)
    {
        const int64_t r0 = o.w0 + 64 * (R0 + 1), c0 = o.w0 + 64 * (tj + 1); // ldlt_tiles.h:213
        const bool two = r0 + 64 < o.rend;                                    // :214
        for (const Geo *g : {&o, e}) {
            if (!g) continue;
            // :225, :230, :235  lvoff = 8 (2 lane), lsoff = 8 (r0 + (qk + m0 + w) ld) + it 8 (32 ld), m0 <= 32, w + 4 it <= 31; 16 bytes
            const int64_t lrow = r0 + 2 * 63 + 1, lcol = g->k + 32 + 31;
            a(lrow, lcol);
            byte_max = std::max(byte_max, 8 * (lrow + lcol * ld) + 7);
            // :225, :230, :240  zvoff = 8 (2 (lane & 31) + (lane >> 5) ldz), zsoff = 8 (c0 - w0 + (m0 + 2 w) ldz) + it 8 (64 ldz); 16 bytes
            const int64_t zrow = c0 - g->w0 + 2 * 31 + 1, zcol = 32 + 2 * 3 + 1 + 8 * 3;
            z(zrow, zcol);
            byte_max = std::max(byte_max, 8 * (zrow + zcol * ldz) + 7);
        }
        // :309-:322, :355, :372  cvoff = 8 (i + kk ld) + 128 tl, csoff = 8 (r0 + 32 w + c0 ld) + 8 (16 cq + 4 reg) ld; wavefronts 2, 3 only
        // if the second tile row exists (`busy`, :278)
        const int64_t crow = r0 + 32 * (two ? 3 : 1) + 16 + 15, ccol = c0 + 3 + 48 + 12;
        a(crow, ccol);
        byte_max = std::max(byte_max, 8 * (crow + ccol * ld) + 7);
    }
    // ldlt_lookahead.h:642-:716 (ldlt.hip: fwd_stage): Y role of panel qq - 1, U role of panel qq - 2; B and Y are the border's
    void fwd_stage(int64_t qq, int64_t nsteps)
    {
        if (qq - 1 < nsteps && qq - 2 >= 0) { const Geo ga = geom(qq - 1), gm = geom(qq - 2); load_panel_tile(ga.k, gm.k); } // :648
        if (qq - 2 >= 0) {
            const Geo gc = geom(qq - 2);
            if (gc.T >= 2)
                for (int64_t ti = 2; ti <= gc.T; ++ti) load_panel_tile(gc.w0 + 64 * (ti - 1), gc.k); // :696-:704
        }
    }
    // ldlt.hip: run_phase
    void run_phase(int64_t sa, int64_t sb, bool close, bool defer, int64_t nsteps)
    {
        std::vector<SchedLaunch> sched;
        ldlt_schedule_phase(sa, sb, close, true, [&](int64_t st) { return st < nsteps ? geom(st).T : (int64_t)0; }, sched, close && defer);
        for (const SchedLaunch &L : sched) {
            if (L.kind == 0) { // ldlt_diag.h:103, :205: guarded (row < nbe, col <= row; r < rend, m < nbe)
                const Geo g = geom(L.p);
                a(g.k + g.nbe - 1, g.k + g.nbe - 1);
                if (g.T > 0) { a(std::min(g.w0 + 63, g.rend - 1), g.k + g.nbe - 1); tile(); }
                g_panel_max = std::max(g_panel_max, L.p);
                continue;
            }
            if (L.roles) {
                const Geo p = geom(L.p), q = L.has_q ? geom(L.p - 1) : Geo{}, gn = geom(L.p + 1);
                const bool qx_helper = L.q_extra && p.T >= 2;
                chain_role(p, q, L.has_q, L.do_diag, L.p, gn.nbe);
                for (int64_t t = 1; t < p.T; ++t) row_role(p, q, L.has_q, L.q_extra, qx_helper, L.defer, t);
                if (qx_helper) qx_diag_role(p, q, L.has_q);
            }
            for (int j = 0; j < L.njobs; ++j) {
                const SchedJob &sj = L.job[j];
                const Geo o = geom(sj.o), e = sj.pair ? geom(sj.o - 1) : Geo{};
                const int64_t Tb = o.T - 1;
                for (int64_t tj = sj.ca; tj < sj.cb; ++tj) {
                    if (big) { // ldlt_tiles.h:165-173: pair_col_items, pair_decode
                        for (int64_t u = 0; u < (Tb - tj + 1) / 2; ++u) bulk_tile_128(o, sj.pair ? &e : nullptr, tj + 2 * u, tj);
                    } else { // ldlt_tiles.h:12-22: col_decode; ldlt_lookahead.h:805: (ti + 1, tj + 1)
                        for (int64_t ti = tj; ti < Tb; ++ti) {
                            update_tile(o, ti + 1, tj + 1);
                            if (sj.pair) update_tile(e, ti + 2, tj + 2); // (panel e's window starts one tile earlier)
                        }
                    }
                }
            }
        }
    }
};

struct Margins { int64_t store = INT64_MAX, store_real = INT64_MAX, n = 0, bw = 0, nr = 0, bwr = 0; };
static Margins g_margin[2]; // [band ? 0 : 1]: capacity - 1 - bound / - largest offset formed, where it is smallest
static bool g_mutate = false;      // LVBA_LAYOUT_SLACK_LESS: the store is taken one ldab / 64 doubles smaller,
static int64_t g_cut[2] = {0, 0}; // and by this much at least

static void check_workspace(int64_t n, int64_t bw)
{
    const LdltWork L = ldlt_work_layout(n, bw);
    const int64_t npan = (n + 63) / 64;
    CHECK(L.ldz == pinned_ldz(n, bw), "ldz n=%lld bw=%lld", (long long)n, (long long)bw);
    // today's order, each region exactly behind the one before
    CHECK(L.G == 0 && L.d == L.G + npan * 4096 && L.b == L.d + n && L.bacc == L.b + n && L.Z[0] == L.bacc + n, "G, d, b, bacc, Z");
    for (int j = 0; j < 3; ++j) CHECK(L.Z[j + 1] == L.Z[j] + L.ldz * 64, "Z ring");
    CHECK(L.side[0] == L.Z[3] + L.ldz * 64 + 64 && L.side[1] == L.side[0] + 4096, "side copies");
    CHECK(L.dq[0] == L.side[1] + 4096 && L.dq[1] == L.dq[0] + 4096 && L.sW == L.dq[1] + 4096, "diagonal shares");
    CHECK(L.sW == pinned_ws_one(n, bw), "one problem's part");
    CHECK(L.x2 == 2 * L.sW && L.E == L.x2 + n + 64 && L.total == L.counter + 8, "x2, exchange buffer, counter");
    CHECK(L.total == pinned_workspace(n, bw) && L.counter == pinned_workspace(n, bw) - 8, "workspace total n=%lld bw=%lld: %lld, was %lld", (long long)n,
          (long long)bw, (long long)L.total, (long long)pinned_workspace(n, bw));
    // the second problem's regions lie at + sW and end before x2
    CHECK(L.sW + L.dq[1] + 4096 == L.x2, "second problem");
}

// one (n, bw) in the storage form band_frac = 1 gives it (band iff ldab < n) or forced dense
static void run_case(int64_t n, int64_t bw_in, bool force_dense)
{
    const LdltGeom g = ldlt_geometry(n, bw_in, !force_dense && ldlt_use_band(n, bw_in, 1.0));
    CHECK(g.band == (!force_dense && bw_in + 128 < n) && g.ld == (g.band ? bw_in + 127 : n) && g.bw == (g.band ? bw_in : n - 1), "geometry");
    const int64_t ld = g.ld, bw = g.bw, cap = ldlt_store_doubles(n, ld), sA = ldlt_mat2_offset(n, ld);
    CHECK(cap == pinned_store(n, ld), "store size n=%lld ld=%lld: %lld, was %lld", (long long)n, (long long)ld, (long long)cap, (long long)pinned_store(n, ld));
    CHECK(sA == (ld + 1) * (n + 1), "offset of matrix 2");
    CHECK(ldlt_offsets_fit_32bit(n, ld) == pinned_32bit(n, ld), "32-bit predicate");
    check_workspace(n, bw);
    const LdltWork W = ldlt_work_layout(n, bw);
    const int form = g.band ? 0 : 1;
    const int64_t cap_used = g_mutate ? cap - std::max<int64_t>(g_cut[form], g.band ? g.ldab : 64) : cap;
    for (int tw = 0; tw < (g.band ? 2 : 1); ++tw) { // ldlt.hip: ldlt_twist_panels
        int64_t P1 = tw ? (n - bw) / 128 : 0;
        if (P1 < 4) P1 = 0;
        if (tw && P1 == 0) continue;
        const int64_t nf = n - 64 * P1, nsteps = (nf + 63) / 64;
        const int64_t room = ldlt_store_room(cap_used, n, ld, P1 > 0); // matrix 2 has the least room
        const int64_t bound = ldlt_reach_store(nf, ld), zbound = ldlt_reach_z(nf, bw, W.ldz);
        CHECK(bound < room, "n=%lld bw=%lld ld=%lld P1=%lld: reach bound %lld, room %lld", (long long)n, (long long)bw, (long long)ld, (long long)P1,
              (long long)bound, (long long)room);
        LdltRoom have{cap_used, W.total};
        CHECK((ldlt_solve_fit(n, ld, bw, P1, have) == nullptr) == (bound < room), "ldlt_solve_fit disagrees");
        have.work = W.total - 1;
        CHECK(ldlt_solve_fit(n, ld, bw, P1, have) != nullptr, "a short workspace is not refused");
        have = LdltRoom{bound + (P1 > 0 ? sA : 0), W.total}; // one double short of the reach
        CHECK(ldlt_solve_fit(n, ld, bw, P1, have) != nullptr, "a short store is not refused");
        if (nf > 64) CHECK(W.Z[3] + zbound < W.sW, "Z reach %lld from slot 3 at %lld leaves the problem's part %lld", (long long)zbound, (long long)W.Z[3], (long long)W.sW);
        if (room - 1 - bound < g_margin[form].store) { g_margin[form].store = room - 1 - bound; g_margin[form].n = n; g_margin[form].bw = bw; }
        for (int bigf = 0; bigf < 2; ++bigf)
            for (int df = 0; df < 2; ++df) {
                if (bigf && !ldlt_offsets_fit_32bit(n, ld)) continue;
                Replay R{n, ld, bw, nf, W.ldz, bigf != 0};
                if (P1 > 0) R.run_phase(0, P1, true, df != 0, nsteps);
                R.run_phase(P1, nsteps, false, df != 0, nsteps);
                if (P1 == 0) for (int64_t qq = 1; qq <= nsteps; ++qq) R.fwd_stage(qq, nsteps); // (a border rides plain factorisations only)
                // ldlt_back.h:52-83, :131, :140: colp = M.a + colc ld, colp[r] with r clamped to rvalid <= n - 1
                R.a(nf - 1, nf - 1);
                CHECK(R.store_max <= bound, "n=%lld bw=%lld ld=%lld P1=%lld big=%d defer=%d: offset %lld beyond the bound %lld", (long long)n, (long long)bw,
                      (long long)ld, (long long)P1, bigf, df, (long long)R.store_max, (long long)bound);
                CHECK(R.z_max <= zbound, "n=%lld bw=%lld P1=%lld big=%d defer=%d: Z offset %lld beyond the bound %lld", (long long)n, (long long)bw, (long long)P1,
                      bigf, df, (long long)R.z_max, (long long)zbound);
                CHECK(R.tile_max <= LDLT_REACH_TILE && LDLT_REACH_TILE < LDLT_TILE, "tile reach");
                CHECK((R.g_panel_max + 1) * LDLT_TILE <= W.d, "G of panel %lld lies outside its region", (long long)R.g_panel_max);
                if (bigf) CHECK(R.byte_max < ((int64_t)1 << 32), "n=%lld ld=%lld: byte offset %lld does not fit 32 bits", (long long)n, (long long)ld, (long long)R.byte_max);
                if (room - 1 - R.store_max < g_margin[form].store_real) { g_margin[form].store_real = room - 1 - R.store_max; g_margin[form].nr = n; g_margin[form].bwr = bw; }
            }
    }
    // the covariance: Z in the matrix-2 slot (band) or a buffer of n n + 64 (dense), every access guarded
    const int64_t zroom = g.band ? ldlt_store_room(cap, n, ld, true) : ldlt_cov_z_dense_doubles(n);
    CHECK(ldlt_cov_z_dense_doubles(n) == n * n + 64, "dense Z buffer");
    const LdltSelinvScratch S = ldlt_selinv_scratch(n, bw, 8);
    CHECK(S.total == ((std::min(bw, n) + 63) / 64 + 1) * (8 + 1) * 4096 + 64 && S.qpart == S.tiles * 8 * 4096, "selinv scratch");
    CHECK(ldlt_selinv_fit(n, ld, bw, 8, LdltSelinvRoom{cap, zroom, W.total, S.total}) == nullptr, "selinv refused at its own sizes");
    CHECK(ldlt_selinv_fit(n, ld, bw, 8, LdltSelinvRoom{cap, (n - 1) * (ld + 1), W.total, S.total}) != nullptr, "a short Z store is not refused");
    CHECK(ldlt_selinv_fit(n, ld, bw, 8, LdltSelinvRoom{cap, zroom, W.total, S.total - 1}) != nullptr, "a short scratch is not refused");
}

static void run_all()
{
    // the list of ldlt_schedule_check.cpp (C3: n = 12000, bw = 2597; C4's; its edge cases)
    const int64_t cases[][2] = {{12000, 2597}, {12000, 143}, {4200, 155}, {4200, 1000}, {640, 600}, {700, 23}, {64, 5}, {65, 64}, {128, 127},
                                {1000, 999}, {6000, 767}, {6000, 768}, {6000, 769}, {3001, 333}, {60000, 2549}};
    for (auto &c : cases) run_case(c[0], c[1], false);
    run_case(3001, 333, true); // dense, n >= 1000 and no multiple of 64 (as {1000, 999} above)
    run_case(4200, 155, true);
    // the smallest shapes at which the reach can still go wrong
    const int64_t ns[] = {6, 63, 64, 65, 127, 128, 129, 191, 192, 193};
    for (int64_t n : ns) {
        const int64_t bws[] = {5, 63, 64, 65, 127, 128, n - 1};
        for (int64_t bw : bws)
            if (bw >= 1 && bw <= n - 1) run_case(n, bw, false);
    }
    for (int64_t bw : {5, 65}) { // the first n at which the twist switches on, (n - bw) / 128 >= 4, and the one before it
        run_case(bw + 512, bw, false);
        run_case(bw + 511, bw, false);
    }
    { // neighbours across the 32-bit predicate's threshold (C3's bandwidth)
        const int64_t bw = 2597, ld = bw + 127;
        int64_t n = 100000;
        while (ldlt_offsets_fit_32bit(n, ld)) ++n;
        CHECK(ldlt_offsets_fit_32bit(n - 1, ld) && !ldlt_offsets_fit_32bit(n, ld), "threshold");
        run_case(n - 1, bw, false);
        run_case(n, bw, false);
    }
}

int main()
{
#ifdef LVBA_LAYOUT_SLACK_LESS
    run_all(); // first pass: where each storage form is tightest
    if (g_fail) { printf("%d check(s) failed before the mutation\n", g_fail); return 2; }
    // one ldab / 64 doubles less (run_case), and at least down to the reach of the tightest geometry
    g_cut[0] = g_margin[0].store + 1;
    g_cut[1] = g_margin[1].store + 1;
    printf("slack less: band store - max(ldab, %lld), dense store - max(64, %lld) doubles\n", (long long)g_cut[0], (long long)g_cut[1]);
    g_margin[0] = g_margin[1] = Margins{};
    g_mutate = true;
#endif
    run_all();
    for (int f = 0; f < 2; ++f)
        printf("%s store: %lld doubles between the reach bound and the end at n=%lld bw=%lld (the tightest of the list); %lld between the largest offset "
               "formed and the end at n=%lld bw=%lld\n", f ? "dense" : "band", (long long)g_margin[f].store, (long long)g_margin[f].n, (long long)g_margin[f].bw,
               (long long)g_margin[f].store_real, (long long)g_margin[f].nr, (long long)g_margin[f].bwr);
    if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
    printf("ldlt layout ok\n");
    return 0;
}
