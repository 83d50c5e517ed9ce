// ldlt_selinv.h -- marginal covariance from the one-ended LDL^T (lvba_balm_covariance; included by ldlt.hip only, inside namespace
// lvba): the selected inverse Z = A^-1 on the band of the factor, by blocked Takahashi recurrences, one launch per 64-column panel
// from the last panel to the first.
//
// A = L D L^T, so Z L = L^-T D^-1, which is upper triangular.  For panel P (columns [k, k + nbe)) and its window W (the rows
// [k + nbe, rend) the factorisation's panel P touches, rend = min(k + nbe + bw, n)), with the pieces the factorisation leaves:
//   L(W, P)  in the band store below the diagonal block (the row roles' L(i, p) = A(i, p) G_p, ldlt_lookahead.h store_lz_tile)
//   G_P      = L_PP^-T D_P^-1, [m][c] row-major in the workspace;  d_P  in the workspace
// and M_P = L_PP^-1 = D_P G_P^T (stored operands, no triangular solve):
//   Z(W, P) = -Z(W, W) L(W, P) M_P
//   Z(P, P) = (G_P - Z(W, P)^T L(W, P)) M_P, symmetrised
// Z(W, W) is only ever read within the band (|i - j| < bw), and every such entry was written by a later panel (as part of its
// diagonal block or of its window), so Z lives in a store of the factor's shape: the second-matrix slot of the band allocation,
// which a one-ended factorisation leaves unused (ldlt_solve, LdltTwist), or a dense n x n buffer for dense handles.
//
// Three launches per panel (kernel boundaries order them; one launch with an agent-scope fence + ticket counter per workgroup took
// 125 us per panel at C3 against 92 us for the three launches):
//   stage 0, T KS workgroups  X_ts = Z(W_t, W_s) L(W_s, P) for row tile t (64 rows of W), inner slice s   (MFMA, inner |W_s|)
//   stage 1, T workgroups     X_t = sum_s X_ts (slice order); Z(W_t, P) = -X_t M_P -> store; Q_t = Z(W_t, P)^T L(W_t, P)
//   stage 2, 1 workgroup      Z(P, P) = (G_P - sum_t Q_t) M_P (tile order), symmetrised -> store
// The sums run in index order, so the result is bitwise reproducible.  Products are v_mfma_f64_16x16x4_f64 on LDS operands:
// wave w owns the output columns [16 w, 16 w + 16), register block rb the rows [16 rb, 16 rb + 16) (ldlt.hip's operand layout).
#pragma once

#define LVBA_SI_LS 68        // LDS row stride of a 64-wide operand (doubles)
#define LVBA_SI_KSMAX 8      // most inner-dimension slices per row tile

struct SelinvPanel {
    double *z;                 // Z store, Z(r, c) = z[r + c ld] for r >= c
    const double *a;           // the factor's store (L below the diagonal blocks)
    int64_t ld, n;
    int64_t k, w0, rend, ksz;  // panel columns [k, k + nbe), window rows [w0, rend), inner slice length (a multiple of 64)
    int nbe, T, KS, stage;
    const double *G, *d;       // G_P [m][c] row-major; d + k
    double *xpart, *qpart;     // [T][KS][4096], [T][4096] partial products
};

// acc[rb] += As (64 x K, k-major: As[kk LS + row]) * Bs (K x 64, Bs[kk LS + col]); lane l, wave w
__device__ __forceinline__ void si_mm(const double *As, const double *Bs, int K, d4 (&acc)[4], int w, int l)
{
    for (int kk = 0; kk < K; kk += 4) {
        const double b = Bs[(kk + (l >> 4)) * LVBA_SI_LS + 16 * w + (l & 15)];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            const double a = As[(kk + (l >> 4)) * LVBA_SI_LS + 16 * rb + (l & 15)];
            acc[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[rb], 0, 0, 0);
        }
    }
}
// register (rb, r) of lane l, wave w holds D[16 rb + (l >> 4) + 4 r][16 w + (l & 15)]
#define SI_ROW(rb, r) (16 * (rb) + (l >> 4) + 4 * (r))
#define SI_COL (16 * w + (l & 15))

// Ms[m LS + c] = (M_P)[m][c] = d_m G_P[c][m] (zero outside the panel's nbe columns)
__device__ __forceinline__ void si_load_m(double *Ms, const SelinvPanel &p, int tid)
{
    for (int e = tid; e < 4096; e += 256) {
        const int m = e & 63, c = e >> 6;
        Ms[m * LVBA_SI_LS + c] = (m < p.nbe && c < p.nbe) ? p.d[m] * p.G[c * 64 + m] : 0.0;
    }
}

__global__ void __launch_bounds__(256) ldlt_selinv_panel_kernel(SelinvPanel p)
{
    __shared__ double buf0[64 * LVBA_SI_LS], buf1[64 * LVBA_SI_LS];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    d4 acc[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) acc[rb] = d4{0.0, 0.0, 0.0, 0.0};
    if (p.stage == 0) {
        const int t = (int)blockIdx.x / p.KS, s = (int)blockIdx.x - t * p.KS;
        const int64_t R0 = p.w0 + 64 * (int64_t)t;
        const int rlim = (int)(p.rend - R0 < 64 ? p.rend - R0 : 64);
        // ---- X_ts = Z(W_t, W_s) L(W_s, P), 64 inner indices per step through LDS (each thread's 16 loads issued together)
        const int64_t kb = p.w0 + s * p.ksz, ke = kb + p.ksz < p.rend ? kb + p.ksz : p.rend;
        for (int64_t k0 = kb; k0 < ke; k0 += 64) {
            double va[16], vb[16];
            if (k0 >= R0 + 64) { // the chunk lies above the diagonal of Z: read its transpose, 64 consecutive doubles per row
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const int kk = tid & 63, i = (tid >> 6) + 4 * it;
                    const int64_t c = k0 + kk;
                    va[it] = (i < rlim && c < ke) ? p.z[c + (R0 + i) * p.ld] : 0.0;
                }
            } else {
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const int i = tid & 63, kk = (tid >> 6) + 4 * it;
                    const int64_t r = R0 + i, c = k0 + kk;
                    double v = 0.0;
                    if (i < rlim && c < ke) v = r >= c ? p.z[r + c * p.ld] : p.z[c + r * p.ld];
                    va[it] = v;
                }
            }
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int kk = tid & 63, m = (tid >> 6) + 4 * it;
                const int64_t r = k0 + kk;
                vb[it] = (r < ke && m < p.nbe) ? p.a[r + (p.k + m) * p.ld] : 0.0;
            }
            __syncthreads(); // (the previous step's products are done with the operands)
            if (k0 >= R0 + 64) {
#pragma unroll
                for (int it = 0; it < 16; ++it) buf0[(tid & 63) * LVBA_SI_LS + (tid >> 6) + 4 * it] = va[it];
            } else {
#pragma unroll
                for (int it = 0; it < 16; ++it) buf0[((tid >> 6) + 4 * it) * LVBA_SI_LS + (tid & 63)] = va[it];
            }
#pragma unroll
            for (int it = 0; it < 16; ++it) buf1[(tid & 63) * LVBA_SI_LS + (tid >> 6) + 4 * it] = vb[it];
            __syncthreads();
            si_mm(buf0, buf1, 64, acc, w, l);
        }
        double *xp = p.xpart + ((int64_t)t * p.KS + s) * 4096;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) xp[(rb * 4 + r) * 256 + tid] = acc[rb][r];
        return;
    }
    if (p.stage == 1) {
        const int t = (int)blockIdx.x;
        const int64_t R0 = p.w0 + 64 * (int64_t)t;
        const int rlim = (int)(p.rend - R0 < 64 ? p.rend - R0 : 64);
        for (int q = 0; q < p.KS; ++q) { // X_t: the slices in order
            const double *xq = p.xpart + ((int64_t)t * p.KS + q) * 4096;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[rb][r] += xq[(rb * 4 + r) * 256 + tid];
        }
        // ---- Z(W_t, P) = -X_t M_P
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) buf0[SI_COL * LVBA_SI_LS + SI_ROW(rb, r)] = acc[rb][r]; // A operand: [m][i]
        si_load_m(buf1, p, tid);
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) acc[rb] = d4{0.0, 0.0, 0.0, 0.0};
        si_mm(buf0, buf1, 64, acc, w, l);
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) buf0[SI_ROW(rb, r) * LVBA_SI_LS + SI_COL] = -acc[rb][r]; // Z(W_t, P) as [i][c]
        for (int e = tid; e < 4096; e += 256) { // L(W_t, P) as [i][b]
            const int i = e & 63, b = e >> 6;
            buf1[i * LVBA_SI_LS + b] = (i < rlim && b < p.nbe) ? p.a[(R0 + i) + (p.k + b) * p.ld] : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < 4096; e += 256) {
            const int i = e & 63, c = e >> 6;
            if (i < rlim && c < p.nbe) p.z[(R0 + i) + (p.k + c) * p.ld] = buf0[i * LVBA_SI_LS + c];
        }
        // ---- Q_t = Z(W_t, P)^T L(W_t, P)
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) acc[rb] = d4{0.0, 0.0, 0.0, 0.0};
        si_mm(buf0, buf1, 64, acc, w, l);
        double *qp = p.qpart + (int64_t)t * 4096;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) qp[(rb * 4 + r) * 256 + tid] = acc[rb][r];
        return;
    }
    for (int q = 0; q < p.T; ++q) { // stage 2: sum_t Q_t in tile order
        const double *qq = p.qpart + (int64_t)q * 4096;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[rb][r] += qq[(rb * 4 + r) * 256 + tid];
    }
    // ---- Z(P, P) = (G_P - sum_t Q_t) M_P, symmetrised (acc holds sum_t Q_t: zero for a panel without a window)
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = SI_ROW(rb, r), m = SI_COL;
            buf0[m * LVBA_SI_LS + a] = (a < p.nbe && m < p.nbe) ? p.G[a * 64 + m] - acc[rb][r] : 0.0; // A operand: [m][a]
        }
    si_load_m(buf1, p, tid);
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) acc[rb] = d4{0.0, 0.0, 0.0, 0.0};
    si_mm(buf0, buf1, 64, acc, w, l);
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) buf0[SI_ROW(rb, r) * LVBA_SI_LS + SI_COL] = acc[rb][r];
    __syncthreads();
    for (int e = tid; e < 4096; e += 256) {
        const int a = e & 63, c = e >> 6;
        if (a >= c && a < p.nbe) p.z[(p.k + a) + (p.k + c) * p.ld] = 0.5 * (buf0[a * LVBA_SI_LS + c] + buf0[c * LVBA_SI_LS + a]);
    }
}
#undef SI_ROW
#undef SI_COL

// The anchor (lvba_cov_opts::anchor) after the fill: its six rows and columns become those of the identity inside the stored
// triangle (band: offsets [0, ld]), i.e. the pose is held fixed.  c0 = first scalar column of the anchor's block.
__global__ void ldlt_anchor_kernel(LdltMat M, int64_t c0)
{
    const int64_t span = M.ld + 1, n = M.n;
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= 12 * span) return;
    const int j = (int)(e / (2 * span));
    const int64_t o = e - j * 2 * span;
    const int64_t C = c0 + j;
    if (o < span) { // column C, rows C + o
        const int64_t R = C + o;
        if (R < n) M.a[R + C * M.ld] = o == 0 ? 1.0 : 0.0;
    } else { // row C, columns C - 1 - (o - span)
        const int64_t Cc = C - 1 - (o - span);
        if (Cc >= 0 && C - Cc <= M.ld) M.a[C + Cc * M.ld] = 0.0;
    }
}

// flag[0] = 1 if the factorisation reported a bad pivot or a pivot d_i fails d_i > ratio * A_ii with A_ii > 0, finite (A_ii from
// the block store's diagonal; 1 for the anchor's columns)
__global__ void ldlt_cov_pivot_kernel(const double *__restrict__ Hblk, int band_blocks, int64_t n, const double *__restrict__ d,
                                      int64_t c0, double ratio, const int *__restrict__ status, int *__restrict__ flag)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i == 0 && status[0]) atomicOr(flag, 1);
    if (i >= n) return;
    const int64_t J = i / 6;
    const int c = (int)(i - 6 * J);
    const double aii = (c0 >= 0 && i >= c0 && i < c0 + 6) ? 1.0 : Hblk[J * (band_blocks + 1) * 36 + c * 7];
    const double di = d[i];
    if (!(isfinite(di) && isfinite(aii) && aii > 0.0 && di > ratio * aii)) atomicOr(flag, 1);
}

// Blocks of Z in the caller's pose order: item q < N the diagonal block of caller pose q, item N + k pair k; one thread per entry.
// band_blocks < 0: dense store (every pair available).  The anchor's entries are returned as zeros.
__global__ void ldlt_cov_gather_kernel(const double *__restrict__ z, int64_t ld, int band_blocks, const int32_t *__restrict__ iperm,
                                       int N, int anchor, int64_t n_pairs, const int32_t *__restrict__ pi, const int32_t *__restrict__ pj,
                                       double *__restrict__ diag, double *__restrict__ blk, uint8_t *__restrict__ avail)
{
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= ((int64_t)N + n_pairs) * 36) return;
    const int64_t q = e / 36;
    const int rc = (int)(e - q * 36), r = rc / 6, c = rc - 6 * (rc / 6);
    int a, b;
    if (q < N) a = b = (int)q;
    else { a = pi[q - N]; b = pj[q - N]; }
    const int64_t I = iperm[a], J = iperm[b];
    const bool ok = band_blocks < 0 || (I > J ? I - J : J - I) <= band_blocks;
    const int64_t R = 6 * I + r, C = 6 * J + c;
    double v = ok ? (R >= C ? z[R + C * ld] : z[C + R * ld]) : __builtin_nan("");
    if (a == anchor || b == anchor) v = ok ? 0.0 : v;
    if (q < N) diag[e] = v;
    else {
        blk[e - (int64_t)N * 36] = v;
        if (rc == 0) avail[q - N] = ok ? 1 : 0;
    }
}
