// closure_device.h -- pairwise consistency of loop closures (lvba_closure_consistency): the scalar arithmetic and the bit-set steps
// of the rule.  Also compiles as plain C++ (tests/closure_check.cpp).  The including file is built without floating-point
// contraction: the two clauses are discrete decisions on rot and trans.
//   A closure k = (i, j, Z) measures Z = T_i^-1 T_j.  With the current poses X, for a < b
//     E_ab = Z_a (X_ja^-1 X_jb) Z_b^-1 (X_ib^-1 X_ia),   rot = |Log(R_E)|,   trans = |t_E|,   L = |j_a - j_b| + |i_a - i_b|
//     consistent iff rot <= rot_tol + rot_rate L and trans <= trans_tol + trans_rate L
//   Prepared form: P_k = X_j Z_k^-1 X_i^-1 (a world-frame transform, the identity for a closure that agrees with the poses), so that
//     E_ab = X_ia^-1 (P_a^-1 P_b) X_ia.  With Q = P_a^-1 P_b the conjugation keeps the angle, and |t_E| = |R_Q t_ia + t_Q - t_ia|:
//     a pair costs one 3 x 3 product, two matrix-vector products and one Log, not six compositions.
//   Adjacency rows are bit-sets of W = ceil(M / 64) words; the greedy clique (include/lvba_hip.h has the rule) works on them word
//   by word.
#pragma once
#include <math.h>
#include <stdint.h>
#include "prior_device.h"

namespace lvba {

constexpr int CLOSURE_MAX = 16384;               // closures per call: the adjacency is then 32 MB
constexpr int CLOSURE_MAX_WORDS = CLOSURE_MAX / 64; // a candidate set: 2 KB of LDS
constexpr int CLOSURE_PREP = 15;                 // doubles per prepared closure: P (R row-major | t), then t_i

struct ClosureParams { // the tolerances of lvba_closure_opts on the device
    double rot_tol, rot_rate, trans_tol, trans_rate;
};

// P = X_j Z^-1 X_i^-1 and t_i into out [CLOSURE_PREP] (poses and Z as R row-major | t)
LVBA_HD void closure_prepare(const double *Xi, const double *Xj, const double *Z, double *out)
{
    double R1[9], u[3], t1[3];
    m3_mult(Xj, Z, R1);      // R_j R_z^T
    m3_tvec(Z, Z + 9, u);    // R_z^T t_z
    m3_vec(Xj, u, t1);
    t1[0] = Xj[9] - t1[0]; t1[1] = Xj[10] - t1[1]; t1[2] = Xj[11] - t1[2]; // X_j Z^-1 = (R1, t_j - R_j R_z^T t_z)
    m3_mult(R1, Xi, out);    // R_P = R1 R_i^T
    m3_vec(out, Xi + 9, u);  // R_P t_i
    out[9] = t1[0] - u[0]; out[10] = t1[1] - u[1]; out[11] = t1[2] - u[2];
    out[12] = Xi[9]; out[13] = Xi[10]; out[14] = Xi[11];
}

// rot and trans of the ordered pair (a, b), a < b: Pa [CLOSURE_PREP] (P_a and t_ia), Pb [12]
LVBA_HD void closure_measures(const double *Pa, const double *Pb, double *rot, double *trans)
{
    double RQ[9], d[3], tQ[3], phi[3], v[3];
    m3_tmul(Pa, Pb, RQ); // R_Pa^T R_Pb
    d[0] = Pb[9] - Pa[9]; d[1] = Pb[10] - Pa[10]; d[2] = Pb[11] - Pa[11];
    m3_tvec(Pa, d, tQ);  // R_Pa^T (t_Pb - t_Pa)
    so3_log(RQ, phi);
    *rot = sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    m3_vec(RQ, Pa + 12, v);
    v[0] = (v[0] - Pa[12]) + tQ[0]; v[1] = (v[1] - Pa[13]) + tQ[1]; v[2] = (v[2] - Pa[14]) + tQ[2];
    *trans = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

// the odometry steps of the cycle
LVBA_HD int32_t closure_path(int32_t ia, int32_t ja, int32_t ib, int32_t jb)
{
    return (ja > jb ? ja - jb : jb - ja) + (ia > ib ? ia - ib : ib - ia);
}

LVBA_HD bool closure_consistent(double rot, double trans, int32_t L, const ClosureParams &o)
{
    return rot <= o.rot_tol + o.rot_rate * (double)L && trans <= o.trans_tol + o.trans_rate * (double)L;
}

// (key descending, index ascending): the order of the seeds by degree and of a round's pick by |A[v] & C|
LVBA_HD bool closure_before(int32_t key_u, int32_t u, int32_t key_v, int32_t v) { return key_u > key_v || (key_u == key_v && u < v); }

// popcount of row[w] (of row[w] & set[w]) over the words w0, w0 + stride, ... < W
LVBA_HD int32_t closure_row_bits(const uint64_t *row, int w0, int W, int stride)
{
    int32_t c = 0;
    for (int w = w0; w < W; w += stride) c += __builtin_popcountll(row[w]);
    return c;
}
LVBA_HD int32_t closure_row_count(const uint64_t *row, const uint64_t *set, int w0, int W, int stride)
{
    int32_t c = 0;
    for (int w = w0; w < W; w += stride) c += __builtin_popcountll(row[w] & set[w]);
    return c;
}

// the set step on word w after the pick v: C <- (C & A[v]) \ {v}
LVBA_HD uint64_t closure_take(uint64_t c_word, uint64_t a_word, int w, int32_t v)
{
    const uint64_t c = c_word & a_word;
    return w == (v >> 6) ? c & ~((uint64_t)1 << (v & 63)) : c;
}

LVBA_HD uint64_t closure_bit(int w, int32_t v) { return w == (v >> 6) ? (uint64_t)1 << (v & 63) : (uint64_t)0; }

} // namespace lvba
