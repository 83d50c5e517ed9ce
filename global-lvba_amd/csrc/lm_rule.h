// lm_rule.h -- the damping rule of BALM2::damping_iter (reference include/BALM/bavoxel.hpp:736-760), host only, plain C++ (also
// compiled by tests/lm_rule_check.cpp): the accept / reject decision, u, v, whether the next iteration evaluates again, the stop
// test and the trace row.  Its drivers -- lvba_balm_lm_step, lvba_balm_refine_groups (a rule per group; lvba_api.hip),
// lvba_posegraph_relax (pose_graph.hip) -- pass costs normalised their own way (by the voxel count, the group's, not at all) and:
//   flagged         a zero or non-finite pivot of the solve.  The reference checks neither the LDLT's info() nor the cost (:706-710,
//                   :731): a broken factorisation gives a NaN residual2, `q > 0` is false, the step is rejected, u *= v, and the loop
//                   goes on with more damping (it can recover).  Same here, whatever r2 holds.  (The grouped driver never flags.)
//   stop_on_reject  true (BALM, :760): any row with |r1 - r2| / r1 < rel_tol ends the loop.  false (the pose graph): only an
//                   accepted row does, its documented q / C1 < rel_tol on acceptance.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/lvba_hip.h"

namespace lvba {

struct LmRule {
    double u = 0.01, v = 2.0;
    bool evaluate = true; // the next iteration starts with an evaluation at the current point (is_calc_hess)
    bool done = false;
    int32_t iter = 0;

    void begin(double u0, double v0, int32_t max_iter)
    {
        u = u0; v = v0; evaluate = true; iter = 0;
        done = max_iter == 0;
    }

    // One iteration's costs r1 (current point), r2 (trial point) and predicted decrease q1 -> its trace row (u, v as the solve used
    // them); then the state moves on.
    lvba_lm_trace step(double r1, double r2, double q1, bool flagged, double rel_tol, int32_t max_iter, bool stop_on_reject)
    {
        const double q = flagged ? NAN : r1 - r2;                                              // :736
        lvba_lm_trace row{};
        row.iter = iter; row.accepted = q > 0; row.evaluated = evaluate;
        row.status = flagged ? LVBA_NUM_FACTORIZATION : (!isfinite(r2) || !isfinite(r1)) ? LVBA_NUM_NONFINITE : LVBA_OK;
        row.residual1 = r1; row.residual2 = r2; row.u = u; row.v = v; row.q = q; row.q1 = q1;
        if (row.accepted) {                                                                    // :744-752
            const double t = 1.0 - pow(2.0 * (q / q1) - 1.0, 3.0);
            v = 2.0;
            u *= t < 1.0 / 3.0 ? 1.0 / 3.0 : t;
        } else {                                                                               // :753-758
            u = u * v;
            v = 2.0 * v;
        }
        evaluate = row.accepted;
        iter += 1;
        if ((row.accepted || stop_on_reject) && fabs(r1 - r2) / r1 < rel_tol) done = true;     // :760
        if (iter >= max_iter) done = true;                                                     // :686
        return row;
    }
};

} // namespace lvba
