// Host build of csrc/visual_prior_device.h (the device code's camera-prior model) for tests/test_visual_priors_host.py: reads
// lines "kind qi[4] ti[3] qj[4] tj[3] Oi[12] Oj[12] meas[12] L[36]" of exact hexadecimal doubles on stdin and prints, per line,
// e[6] Wi[36] Wj[36] (whitened, in the visual tangent) and the cost 1/2 |e|^2 as exact hexadecimal doubles.
#include <stdio.h>

#include "../global-lvba_amd/csrc/visual_prior_device.h"

static bool rd(double *v, int n)
{
    for (int a = 0; a < n; ++a)
        if (scanf("%la", v + a) != 1) return false;
    return true;
}

int main()
{
    int kind;
    while (scanf("%d", &kind) == 1) {
        double qi[4], ti[3], qj[4], tj[3], Oi[12], Oj[12], meas[12], L[36], e[6], Wi[36] = {}, Wj[36] = {};
        if (!rd(qi, 4) || !rd(ti, 3) || !rd(qj, 4) || !rd(tj, 3) || !rd(Oi, 12) || !rd(Oj, 12) || !rd(meas, 12) || !rd(L, 36)) return 1;
        const double c = lvba::vprior_eval(kind, meas, Oi, Oj, L, qi, ti, qj, tj, e, true, Wi, Wj);
        for (double v : e) printf("%a ", v);
        for (double v : Wi) printf("%a ", v);
        for (double v : Wj) printf("%a ", v);
        printf("%a\n", c);
    }
    return 0;
}
