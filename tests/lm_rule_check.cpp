// lm_rule_check.cpp -- csrc/lm_rule.h compiled for the host (tests/test_lm_rule_host.py loads it with ctypes): rows of costs are fed
// through the rule, and every row's decisions and the state they leave come back.
#include "../global-lvba_amd/csrc/lm_rule.h"

extern "C" {

// in [n][4] = r1 | r2 | q1 | flagged (non-zero).  Returns whether the rule is done before any step; per row
// iout [n][4] = accepted | evaluated | status | done after the row, dout [n][3] = u | v (as the row used them) | q.
int lmr_replay(int n, const double *in, double u0, double v0, double rel_tol, int max_iter, int stop_on_reject, int32_t *iout, double *dout)
{
    lvba::LmRule lm;
    lm.begin(u0, v0, max_iter);
    const int done0 = lm.done;
    for (int k = 0; k < n; ++k) {
        const double *r = in + 4 * k;
        const lvba_lm_trace row = lm.step(r[0], r[1], r[2], r[3] != 0.0, rel_tol, max_iter, stop_on_reject != 0);
        iout[4 * k] = row.accepted; iout[4 * k + 1] = row.evaluated; iout[4 * k + 2] = row.status; iout[4 * k + 3] = lm.done;
        dout[3 * k] = row.u; dout[3 * k + 1] = row.v; dout[3 * k + 2] = row.q;
        if (row.iter != k) return -1;
    }
    return done0;
}

}
