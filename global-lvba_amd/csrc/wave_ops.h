// wave_ops.h -- the wavefront and workgroup reductions, each tree written once (device code only: included from .hip files and from
// headers that only hipcc compiles).  Every caller promises bytes that do not change run to run, so what fixes the order of a
// reduction is stated here and nowhere else; DESIGN.md, "Wavefront reductions", says which tree to use when.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace lvba {

// ---- moving values between lanes ------------------------------------------------------------------------------------------
// v of the lane that the DPP control CTRL names; a lane without such a source, or in a row that ROW_MASK leaves out, gets `old`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false); }
// the same for a double, as its two 32-bit halves
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double old, double v)
{
    const int lo = dpp_i32<CTRL, ROW_MASK>(__double2loint(old), __double2loint(v));
    const int hi = dpp_i32<CTRL, ROW_MASK>(__double2hiint(old), __double2hiint(v));
    return __hiloint2double(hi, lo);
}
// v of lane `lane` (uniform), in every lane
__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// ---- the DPP tree: result in lane 63 ----------------------------------------------------------------------------------------
// Four row shifts and two row broadcasts on the DPP path of the vector ALU: no LDS, no ds_bpermute (as ds_bpermute shuffles the
// six reductions of the key kernel cost 0.2 ms per 16 M points).  Step::step<CTRL, ROW_MASK>(v) returns v combined with the
// value of its DPP source -- and with the operation's identity where a lane has no source.  After the shifts by 1, 2, 4, 8 lane
// 15 of every row of 16 holds its row, ((l15 + l14) + (l13 + l12)) + ... pairwise; then row 1 takes in row 0 and row 3 row 2,
// then rows 2 and 3 take in rows 0 + 1: lane 63 holds (row 3 + row 2) + (row 1 + row 0), `own + source` at every step.  The
// other lanes hold partial results of no use.  The order is a function of the lane numbers alone.
template <class Step, class T>
__device__ __forceinline__ T wave_fold_to_lane63(T v)
{
    v = Step::template step<0x111, 0xf>(v); // row_shr:1
    v = Step::template step<0x112, 0xf>(v); // row_shr:2
    v = Step::template step<0x114, 0xf>(v); // row_shr:4
    v = Step::template step<0x118, 0xf>(v); // row_shr:8   -> lane 15 of every row of 16: the row
    v = Step::template step<0x142, 0xa>(v); // row_bcast:15 -> rows 1 and 3 take in rows 0 and 2
    v = Step::template step<0x143, 0xc>(v); // row_bcast:31 -> rows 2 and 3 take in rows 0 + 1
    return v;
}
struct MaxStepI32 { // of values >= 0
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ int step(int v) { return max(v, dpp_i32<CTRL, ROW_MASK>(0, v)); }
};
struct SumStepI32 { // integers add exactly: the order is of no account
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ int step(int v) { return v + dpp_i32<CTRL, ROW_MASK>(0, v); }
};
struct SumStepI64 { // the same in 64 bits, as two 32-bit halves through the DPP path and one 64-bit add
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ unsigned long long step(unsigned long long v)
    {
        const unsigned lo = (unsigned)dpp_i32<CTRL, ROW_MASK>(0, (int)(unsigned)v);
        const unsigned hi = (unsigned)dpp_i32<CTRL, ROW_MASK>(0, (int)(unsigned)(v >> 32));
        return v + (((unsigned long long)hi << 32) | lo);
    }
};
struct SumStepF64 {
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ double step(double v) { return v + dpp_f64<CTRL, ROW_MASK>(0.0, v); }
};
// min of (d2, idx) pairs in lexicographic order -- the lower idx wins a tie, so the result does not depend on which lane held
// what.  Pair: any struct with a float or double `d2` and an int32_t `idx`.  A lane without a source sees (inf, INT32_MAX), which
// loses against every real pair (the candidate searches: loop_candidates.hip, place.hip).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_val(float old, float v)
{
    return __int_as_float(dpp_i32<CTRL, ROW_MASK>(__float_as_int(old), __float_as_int(v)));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_val(double old, double v) { return dpp_f64<CTRL, ROW_MASK>(old, v); }
template <class Pair>
struct MinPairStep {
    template <int CTRL, int ROW_MASK>
    static __device__ __forceinline__ Pair step(Pair v)
    {
        Pair o = v;
        o.d2 = dpp_val<CTRL, ROW_MASK>((decltype(v.d2))INFINITY, v.d2);
        o.idx = dpp_i32<CTRL, ROW_MASK>(INT32_MAX, v.idx);
        return (o.d2 < v.d2 || (o.d2 == v.d2 && o.idx < v.idx)) ? o : v;
    }
};
__device__ __forceinline__ int wave_max_to_lane63(int v) { return wave_fold_to_lane63<MaxStepI32>(v); } // v >= 0
__device__ __forceinline__ double wave_sum_to_lane63(double v) { return wave_fold_to_lane63<SumStepF64>(v); }

// ---- the shuffle tree: result in lane 0 ---------------------------------------------------------------------------------------
// x = op(x, x of lane + off) for off = 32, 16, ..., 1: lane 0 ends with ((l0 + l32) + (l16 + l48)) + ... -- `own op the lane
// above` at every step, a function of the lane numbers alone.  The other lanes hold partial results of no use.
template <class T, class Op>
__device__ __forceinline__ T wave_reduce_down(T x, Op op)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = op(x, __shfl_down(x, off, 64));
    return x;
}
__device__ __forceinline__ double wave_sum(double x)
{
    return wave_reduce_down(x, [](double a, double b) { return a + b; });
}

// ---- the workgroup sum ----------------------------------------------------------------------------------------------------------
// Sum over the 64 * WAVES threads of a workgroup: the shuffle tree, lane 0 of every wavefront parks its share in red (>= WAVES
// doubles of LDS), a barrier, then ((red[0] + red[1]) + red[2]) + ... in index order.  For thread 0 (every thread forms the
// same total, but `red` may be written again by the others before they read it: block_sum_all for a total that all may use).
// The sum starts AT share 0, not at 0.0.  The 16-wavefront reductions (reduce_chunks_kernel, predicted_decrease_kernel,
// vis_reduce_kernel) once started at 0.0; the sign of a total whose shares are ALL -0.0 (now -0.0, then +0.0) is the single
// representable difference between the two forms.  Their callers' per-thread sums start at +0.0, and a sum is -0.0 only when
// both operands are, so no share of theirs is ever -0.0; and what reads the totals (cost comparisons, norms, sums) takes the
// value, not the sign.
template <int WAVES>
__device__ __forceinline__ double block_sum(double x, double *red)
{
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) t += red[i];
    return t;
}
// the same, valid in every thread, and `red` free again on return
template <int WAVES>
__device__ __forceinline__ double block_sum_all(double x, double *red)
{
    const double t = block_sum<WAVES>(x, red);
    __syncthreads();
    return t;
}

} // namespace lvba
