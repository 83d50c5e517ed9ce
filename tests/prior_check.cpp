// Host build of csrc/prior_device.h (the device code's pose-prior model) for tests/test_priors_host.py: reads lines
// "kind Ti[12] Tj[12] Oi[12] Oj[12] meas[12] L[36]" of exact hexadecimal doubles on stdin and prints, per line, r[6] e[6]
// Ji[36] Jj[36] (whitened) and the cost 1/2 |e|^2 as exact hexadecimal doubles.
#include <stdio.h>

#include "../global-lvba_amd/csrc/prior_device.h"

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
        double Ti[12], Tj[12], Oi[12], Oj[12], meas[12], L[36], r[6], e[6], Ji[36] = {}, Jj[36] = {}, Wi[36], Wj[36];
        if (!rd(Ti, 12) || !rd(Tj, 12) || !rd(Oi, 12) || !rd(Oj, 12) || !rd(meas, 12) || !rd(L, 36)) return 1;
        lvba::prior_raw(kind, meas, Ti, Oi, Tj, Oj, r, true, Ji, Jj);
        const double c = lvba::prior_whiten(kind, L, r, e);
        lvba::prior_whiten_jac(kind, L, Ji, Wi);
        lvba::prior_whiten_jac(kind, L, Jj, Wj);
        for (double v : r) printf("%a ", v);
        for (double v : e) printf("%a ", v);
        for (double v : Wi) printf("%a ", v);
        for (double v : Wj) printf("%a ", v);
        printf("%a\n", c);
    }
    return 0;
}
