// Host build of csrc/visual_loss.h (the device code's loss functions) for tests/test_visual_loss_host.py: reads lines
// "kind a s" on stdin and prints rho, rho', rho'' of each as exact hexadecimal doubles.
#include <stdio.h>

#include "../global-lvba_amd/csrc/visual_loss.h"

int main()
{
    int kind;
    double a, s;
    while (scanf("%d %la %la", &kind, &a, &s) == 3) {
        double rho[3];
        lvba::loss_eval(kind, a, s, rho);
        printf("%a %a %a\n", rho[0], rho[1], rho[2]);
    }
    return 0;
}
