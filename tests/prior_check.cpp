// Host build of csrc/prior_device.h (the device code's pose-prior model) for tests/test_priors_host.py: reads lines
// "kind Ti[12] Tj[12] Oi[12] Oj[12] meas[12] L[36]" of exact hexadecimal doubles on stdin and prints, per line, r[6] e[6]
// Ji[36] Jj[36] (whitened), the cost 1/2 |e|^2 and the lin record [PL_LIN] for flip = 0 and for flip = 1, each written over a
// record full of SENTINEL, as exact hexadecimal doubles.
#include <stdio.h>

#include "../global-lvba_amd/csrc/prior_device.h"

static const double SENTINEL = -777.0;

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
        double Ti[12], Tj[12], Oi[12], Oj[12], meas[12], L[36], r[6], e[6], Wi[36], Wj[36] = {}, o[2][lvba::PL_LIN];
        if (!rd(Ti, 12) || !rd(Tj, 12) || !rd(Oi, 12) || !rd(Oj, 12) || !rd(meas, 12) || !rd(L, 36)) return 1;
        lvba::prior_raw(kind, meas, Ti, Oi, Tj, Oj, r, false, nullptr, nullptr);
        const double c = lvba::prior_eval(kind, meas, Oi, Oj, L, Ti, Tj, e, true, Wi, Wj); // (Wj: RELATIVE only)
        for (int flip = 0; flip < 2; ++flip) {
            for (double &v : o[flip]) v = SENTINEL;
            lvba::prior_record(kind, e, Wi, Wj, flip != 0, o[flip]);
        }
        for (double v : r) printf("%a ", v);
        for (double v : e) printf("%a ", v);
        for (double v : Wi) printf("%a ", v);
        for (double v : Wj) printf("%a ", v);
        printf("%a", c);
        for (int flip = 0; flip < 2; ++flip)
            for (double v : o[flip]) printf(" %a", v);
        printf("\n");
    }
    return 0;
}
