// ldlt_layout.h -- where the band / dense LDL^T keeps what, and how far its kernels reach (host-only, no HIP: block_system.hip,
// lvba_api.hip and ldlt.hip size and address everything through it; tests/ldlt_layout_check.cpp replays the launch list of
// ldlt_schedule.h, forms every offset the tile loaders form and holds them to the bounds and sizes below).
//
// WHY THE SIZES CARRY SLACK.  The look-ahead kernels load whole 64 x 64 (128 x 64) tiles UNCONDITIONALLY and mask afterwards
// (ldlt_lookahead.h: load_panel_tile, load_z_tile, load_c_tile; ldlt_tiles.h: bulk_tile_128's fetch and load_c): a tile that starts
// on the last row of the matrix still reads 63 (127) rows and 63 columns past it.  Those reads must land inside the allocation.
// Every store, and every load of the other kernels (ldlt_diag.h, ldlt_back.h, ldlt_prepare.h, ldlt_selinv.h, update_tile[2] of
// ldlt_tiles.h) is guarded and stays inside the matrix proper: (nf - 1) (ld + 1) at most -- ldlt_selinv.h's reads and writes of
// z among them (every one sits behind `i < rlim && c < ke`, `a < p.nbe` or the like), so the Z store needs no slack.
// ldlt_solve and ldlt_selinv refuse (ldlt_solve_fit, ldlt_selinv_fit) a store or workspace smaller than what is stated here.
#pragma once
#include <cstdint>

namespace lvba {

constexpr int64_t LDLT_NB = 64;      // panel width (= LVBA_NB)
constexpr int64_t LDLT_TILE = 4096;  // doubles of a 64 x 64 tile: G of a panel, a side copy, a share of a diagonal block

// ---------------------------------------------------------------------------------------------- the matrix store
// Storage of an n x n system of half-bandwidth bw (scalars): LAPACK lower-band storage with ldab = bw + 64 + 64 rows per column
// -- the band, and the rows a panel's window [k + 64, k + 64 + bw) gains over its first column's -- when that is narrower than
// band_frac n, else dense.  ld / bw: as LdltMat carries them (band: ld = ldab - 1; dense: ld = n, bw = n - 1).
struct LdltGeom { bool band; int64_t ld, bw, ldab; };
inline int64_t ldlt_ldab(int64_t bw) { return bw + LDLT_NB + 64; }
inline bool ldlt_use_band(int64_t n, int64_t bw, double band_frac) { return (double)ldlt_ldab(bw) < band_frac * (double)n; }
inline LdltGeom ldlt_geometry(int64_t n, int64_t bw, bool band)
{
    if (band) return LdltGeom{true, ldlt_ldab(bw) - 1, bw, ldlt_ldab(bw)};
    return LdltGeom{false, n, n - 1, 0};
}
// offset of matrix 2 (the reversed trailing block of the twisted factorisation, ldlt_prepare.h: LdltTwist::sA; the covariance
// keeps Z there): n + 1 columns of matrix 1 come first
inline int64_t ldlt_mat2_offset(int64_t n, int64_t ld) { return (ld + 1) * (n + 1); }
// doubles of the store.  band (ld != n): both matrices' n + 1 columns + 65 columns of slack; dense: n columns + 64 + 128 doubles
inline int64_t ldlt_store_doubles(int64_t n, int64_t ld)
{
    if (ld != n) return 2 * ldlt_mat2_offset(n, ld) + 65 * (ld + 1);
    return n * n + 64 * n + 128;
}
// what one problem may address from ITS base pointer (matrix 2: a + sA) in a store of `cap` doubles
inline int64_t ldlt_store_room(int64_t cap, int64_t n, int64_t ld, bool second) { return second ? cap - ldlt_mat2_offset(n, ld) : cap; }

// Largest element offset relative to M.a that a kernel of one solve forms, for a problem of nf columns (nf = n, or n - 64 P for the
// two ends of a twisted factorisation).  One panel (nf <= 64): only guarded accesses.  Else the maximum is taken by
//   load_c_tile  (ldlt_lookahead.h:204)  M.a + (R0 + i) + (C0 + 16 w + kk) ld, + 16 t + reg 4 ld: row R0 + 63, column C0 + 63, with
//                R0 = C0 = p.w0 <= nf - 1 (chain_role :344; qx_diag_role :614 and row_role's c2 :490 reach the same column: their
//                tile column p.w0 + 64 lies inside panel q's window)                                     -> (nf + 62) (ld + 1)
// and the others stay below it:
//   load_panel_tile (:184)  M.a + (r0 + row) + (kc + w) ld, + it 4 ld: row r0 + 63 <= nf + 62, column kc + 63 <= nf - 2 (kc is the
//                first column of a panel that has a window: kc + 64 < nf)
//   bulk_tile_128 fetch (ldlt_tiles.h:230, :235)  8 (r0 + (qk + m0 + w) ld) + 8 (2 lane) + it 32 ld 8, 16 bytes: row r0 + 127 <=
//                nf + 126, column qk + 63 <= nf - 2:  (nf + 126) + (nf - 2) ld  =  (nf + 62) (ld + 1) - 64 (ld - 1)
//   bulk_tile_128 load_c / stores (:309-:322, :355, :372)  row r0 + 32 w + 16 tl + i, column c0 + 16 cq + 4 reg + kk, c0 <= r0: the
//                second 64 rows only if r0 + 64 < rend (`busy`), so row <= nf + 62, column <= nf + 62
//   store_lz_tile (:230), store_c_tile (:264), chain_role's write-back (:374): unguarded only for tiles wholly inside the window
inline int64_t ldlt_reach_store(int64_t nf, int64_t ld) { return nf <= LDLT_NB ? (nf - 1) * (ld + 1) : (nf + 62) * (ld + 1); }
// May the 128 x 64 bulk tiles address one problem's storage with 32-bit BYTE offsets (buffer instructions, ldlt_tiles.h:215)?
// The last byte read lies below 8 (ldlt_reach_store + 1) <= 8 (ld (n + 128) + n + 256) for every nf <= n, and the buffer's range
// check ends at 0xFFFFFFF0.
inline bool ldlt_offsets_fit_32bit(int64_t n, int64_t ld)
{
    return ((uint64_t)ld * (uint64_t)(n + 128) + (uint64_t)n + 256) * 8 < 0xFFFF0000ull;
}

// ---------------------------------------------------------------------------------------------- the workspace
// Offsets (doubles) into ldlt_solve's workspace.  One problem's part, in this order:
//   G [panels][64 x 64] | d [n] | b [n] | bacc [n] | Z[0..3] [64][ldz] (panel st's Z = L D in slot st % 4) | 64 spare |
//   side[0..1] (A(p+1, p) as the row roles read it) | dq[0..1] (panel q's share of the next diagonal block)
// the second problem of a twisted factorisation has the same at + sW; behind both: matrix 2's solution vector x2 [n] | 64 spare |
// the exchange buffer of the multi-rank form (|S| <= bw + 2 * 64 columns of bw + 1 entries, and the S part of the rhs) |
// LVBA_CHECK_BAND's counter (8).
struct LdltWork {
    int64_t ldz;
    int64_t G, d, b, bacc, Z[4], side[2], dq[2];
    int64_t sW;
    int64_t x2, E, counter, total;
};
inline LdltWork ldlt_work_layout(int64_t n, int64_t bw)
{
    LdltWork L{};
    L.ldz = ldlt_ldab(bw) < n ? ldlt_ldab(bw) : n;
    int64_t at = 0;
    auto take = [&](int64_t cnt) { const int64_t o = at; at += cnt; return o; };
    L.G = take((n + LDLT_NB - 1) / LDLT_NB * LDLT_TILE);
    L.d = take(n); L.b = take(n); L.bacc = take(n);
    for (int j = 0; j < 4; ++j) L.Z[j] = take(L.ldz * LDLT_NB);
    take(64);
    for (int j = 0; j < 2; ++j) L.side[j] = take(LDLT_TILE);
    for (int j = 0; j < 2; ++j) L.dq[j] = take(LDLT_TILE);
    L.sW = at;
    at = 2 * L.sW;
    L.x2 = take(n + 64);
    L.E = take((n < bw + 2 * LDLT_NB ? n : bw + 2 * LDLT_NB) * (bw + 2) + 64);
    L.counter = take(8);
    L.total = at;
    return L;
}
// Largest offset relative to a Z slot's start that a load of it forms (the stores are guarded or wholly inside the window):
//   load_z_tile (ldlt_lookahead.h:194)  Z + (r0 + row - w0) + w ldz, + it 4 ldz: row r0 - w0 + 63, column 63; r0 is the first row of a
//                tile that starts inside the panel's window, r0 < rend <= min(w0 + bw, nf), and w0 >= 64
//   bulk_tile_128 fetch (ldlt_tiles.h:225, :230, :240)  8 (zr + (m0 + 2 w) ldz) + 8 (zrow + zc ldz) + it 64 ldz 8, 16 bytes: row
//                c0 - w0 + 63, column 63; for the partner panel e the tile may start up to 64 rows past e's window (c0 < rend_o <=
//                rend_e + 64)
// -> row <= min(bw + 126, nf - 2).  What lies past a slot is the next slot, the spare 64 or the side copies: inside the problem's part.
inline int64_t ldlt_reach_z(int64_t nf, int64_t bw, int64_t ldz) { return (bw + 126 < nf - 2 ? bw + 126 : nf - 2) + 63 * ldz; }
// side / dq / G tiles: [(w + 4 it) 64 + row] (ldlt_lookahead.h:525, :582, :596, :317, :307): the tile exactly
constexpr int64_t LDLT_REACH_TILE = LDLT_TILE - 1;

// ---------------------------------------------------------------------------------------------- the covariance (ldlt_selinv.h)
// Z = A^-1 on the band of the factor lives in the matrix-2 slot of a band store (ldlt_store_room(.., true) doubles), in a buffer
// of its own for a dense one
inline int64_t ldlt_cov_z_dense_doubles(int64_t n) { return n * n + 64; }
// partial products of the selected inversion: xpart [tiles][ksmax][64 x 64] | qpart [tiles][64 x 64] | 64 spare
struct LdltSelinvScratch { int64_t tiles, xpart, qpart, total; };
inline LdltSelinvScratch ldlt_selinv_scratch(int64_t n, int64_t bw, int64_t ksmax)
{
    LdltSelinvScratch S{};
    S.tiles = ((bw < n ? bw : n) + 63) / 64 + 1;
    S.xpart = 0; S.qpart = S.tiles * ksmax * LDLT_TILE;
    S.total = S.qpart + S.tiles * LDLT_TILE + 64;
    return S;
}

// ---------------------------------------------------------------------------------------------- what a caller hands over
// capacities, in doubles, of the buffers a solve is given (as they were ALLOCATED, not as this header would size them)
struct LdltRoom { int64_t store, work; };
struct LdltSelinvRoom { int64_t store, z, work, scratch; };
// nullptr, or why a solve of (n, ld, bw) with `twist_panels` panels per end must not be launched on these buffers
inline const char *ldlt_solve_fit(int64_t n, int64_t ld, int64_t bw, int64_t twist_panels, const LdltRoom &room)
{
    const int64_t nf = n - twist_panels * LDLT_NB;
    if (ldlt_reach_store(nf, ld) >= ldlt_store_room(room.store, n, ld, twist_panels > 0)) return "the matrix store is smaller than the tiles' reach";
    const LdltWork L = ldlt_work_layout(n, bw);
    if (L.total > room.work) return "the workspace is smaller than its layout";
    if (nf > LDLT_NB && L.Z[3] + ldlt_reach_z(nf, bw, L.ldz) >= L.sW) return "a Z tile's reach leaves the problem's workspace";
    return nullptr;
}
inline const char *ldlt_selinv_fit(int64_t n, int64_t ld, int64_t bw, int64_t ksmax, const LdltSelinvRoom &room)
{
    const int64_t last = (n - 1) * (ld + 1); // every access is guarded (above)
    if (last >= room.store || last >= room.z) return "the factor's or the inverse's store is smaller than the matrix";
    if (ldlt_work_layout(n, bw).b > room.work) return "the workspace does not hold G and d";
    if (ldlt_selinv_scratch(n, bw, ksmax).total > room.scratch) return "the scratch buffer is smaller than its layout";
    return nullptr;
}

} // namespace lvba
