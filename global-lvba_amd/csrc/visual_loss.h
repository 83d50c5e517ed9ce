// visual_loss.h -- robust loss functions of the visual bundle adjustment (lvba_visual_set_loss).  Also compiles as plain C++
// (tests/visual_loss_check.cpp).
//   rho(s), rho'(s), rho''(s) of Ceres Solver 2.1.0's HuberLoss, SoftLOneLoss, CauchyLoss, ArctanLoss and TukeyLoss
//   (internal/ceres/loss_function.cc; not in the reference tree, restated from its published sources).  `a` is the loss
//   scale in whitened residual units, s = |f|^2 of one residual block.  rho' is clamped below by DBL_MIN where Ceres clamps it.
// Every kind here has rho'' <= 0 for s >= 0, so Ceres' Corrector (internal/ceres/corrector.cc) only takes its scaling branch:
//   r~ = sqrt(rho'(s)) r,  J~ = sqrt(rho'(s)) J,  and the block contributes 1/2 rho(s) to the cost.
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define LVBA_HD __host__ __device__ __forceinline__
#else
#ifndef LVBA_HD
#define LVBA_HD inline
#endif
#endif

namespace lvba {

// kinds: the LVBA_LOSS_* values of include/lvba_hip.h
enum { VLOSS_TRIVIAL = 0, VLOSS_HUBER = 1, VLOSS_SOFTLONE = 2, VLOSS_CAUCHY = 3, VLOSS_ARCTAN = 4, VLOSS_TUKEY = 5 };

LVBA_HD void loss_eval(int kind, double a, double s, double *rho)
{
    const double b = a * a;
    switch (kind) {
    case VLOSS_HUBER:
        if (s > b) {
            const double r = sqrt(s);
            rho[0] = 2.0 * a * r - b;
            rho[1] = fmax(DBL_MIN, a / r);
            rho[2] = -rho[1] / (2.0 * s);
        } else {
            rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
        }
        return;
    case VLOSS_SOFTLONE: {
        const double c = 1.0 / b;
        const double sum = 1.0 + s * c, tmp = sqrt(sum);
        rho[0] = 2.0 * b * (tmp - 1.0);
        rho[1] = fmax(DBL_MIN, 1.0 / tmp);
        rho[2] = -(c * rho[1]) / (2.0 * sum);
        return;
    }
    case VLOSS_CAUCHY: {
        const double c = 1.0 / b;
        const double sum = 1.0 + s * c, inv = 1.0 / sum;
        rho[0] = b * log(sum);
        rho[1] = fmax(DBL_MIN, inv);
        rho[2] = -c * (inv * inv);
        return;
    }
    case VLOSS_ARCTAN: {
        const double c = 1.0 / b;
        const double sum = 1.0 + s * s * c, inv = 1.0 / sum;
        rho[0] = a * atan2(s, a);
        rho[1] = fmax(DBL_MIN, inv);
        rho[2] = -2.0 * s * c * (inv * inv);
        return;
    }
    case VLOSS_TUKEY:
        if (s <= b) {
            const double v = 1.0 - s / b, v2 = v * v;
            rho[0] = b / 3.0 * (1.0 - v2 * v);
            rho[1] = v2;
            rho[2] = -2.0 / b * v;
        } else {
            rho[0] = b / 3.0; rho[1] = 0.0; rho[2] = 0.0;
        }
        return;
    default:
        rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
        return;
    }
}

} // namespace lvba
