// bn_ci_dev.hpp -- the chi-square upper tail as a stated fp64 function (include/bn_mi355x.h, "conditional-independence tests"):
// chisq_sf(G, df) = Q(df / 2, G / 2), the regularised upper incomplete gamma function.  Every operation is a plain fp64 one (no
// contraction); the library calls are the device's log and exp, and lgamma_pos (bn_learn_dev.hpp) for log Gamma(a).
#pragma once

#include <hip/hip_runtime.h>

#include "bn_learn_dev.hpp"

namespace bnmi {
namespace {

constexpr int kChisqMaxIter = 100000;          // both loops: about sqrt(2 a log(1 / eps)) ~ 6500 steps at df = 2^20 (a = 2^19)
constexpr double kChisqEps = 0x1p-52;          // termination: the last term (series) or factor - 1 (fraction) below eps relative
constexpr double kChisqTiny = 0x1p-1000;       // modified Lentz: what replaces a vanishing denominator

// G >= 0 finite, df >= 0.  Never NaN; a vanishing tail is 0.0 or a denormal.
__device__ inline double chisq_sf(double g, long long df) {
    if (df <= 0 || !(g > 0.0)) return 1.0;
    const double a = 0.5 * double(df), x = 0.5 * g;
    const double pref = exp(((a * log(x)) - x) - lgamma_pos(a));
    double q;
    if (x < a + 1.0) {
        // P(a, x) = pref * sum over n >= 0 of x^n / (a (a + 1) ... (a + n))
        double ap = a, del = 1.0 / a, sum = del;
        for (int n = 0; n < kChisqMaxIter; ++n) {
            ap = ap + 1.0;
            del = (del * x) / ap;
            sum = sum + del;
            if (del < sum * kChisqEps) break;
        }
        q = 1.0 - (sum * pref);
    } else {
        // Q(a, x) = pref * 1 / (x + 1 - a - 1 (1 - a) / (x + 3 - a - 2 (2 - a) / (x + 5 - a - ...)))
        double b = (x + 1.0) - a, c = 1.0 / kChisqTiny, d = 1.0 / b, h = d;
        for (int i = 1; i <= kChisqMaxIter; ++i) {
            const double an = (-double(i)) * (double(i) - a);
            b = b + 2.0;
            d = (an * d) + b;
            if (fabs(d) < kChisqTiny) d = kChisqTiny;
            c = b + (an / c);
            if (fabs(c) < kChisqTiny) c = kChisqTiny;
            d = 1.0 / d;
            const double del = d * c;
            h = h * del;
            if (fabs(del - 1.0) < kChisqEps) break;
        }
        q = pref * h;
    }
    if (!(q > 0.0)) return 0.0;   // (a rounding below zero, and NaN)
    return q > 1.0 ? 1.0 : q;
}

}  // namespace
}  // namespace bnmi
