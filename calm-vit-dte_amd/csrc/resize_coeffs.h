// The coefficients of PIL's 8-bit antialiased bilinear resample (Image.resize(size, BILINEAR): precompute_coeffs and
// normalize_coeffs_8bpc of its Resample.c, restated), one axis at a time.  This file is the definition: the kernel of
// resize.hip, the host entry point calm_resize_coeffs and, through it, the tests all evaluate these functions.
//
// Per axis, `in` source and `out` output pixels:
//   scale = (double)in / out;  fs = max(scale, 1);  support = fs;  ss = 1 / fs
//   output o:  center = (o + 0.5) * scale
//              lo = max((int)(center - support + 0.5), 0);  hi = min((int)(center + support + 0.5), in);  n = hi - lo
//              w[j] = tri((j + lo - center + 0.5) * ss), tri(t) = max(1 - |t|, 0);  ww = w[0] + w[1] + ... in this order
//              k[j] = (int)(0.5 + w[j] / ww * 2^22)       (w[j] itself when ww == 0)
// Every operation is one IEEE double operation in the order written: contraction is switched off, because a fused
// multiply-add in `center - support + 0.5` or in the weight changes the truncations.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CALM_RESIZE_HD __host__ __device__
#else
#define CALM_RESIZE_HD
#endif

#define CALM_RESIZE_PRECISION_BITS 22          /* 32 - 8 - 2: 255 * 2^22 + 2^21 < 2^31 */

struct CalmResizeAxis {
    double scale, support, ss;
    int kmax;                                  // 2 ceil(support) + 1: no output pixel has more taps
};
struct CalmResizeTaps {
    int lo, n;                                 // taps lo .. lo + n - 1
    double center, ww;
};

CALM_RESIZE_HD inline CalmResizeAxis calm_resize_axis(int in, int out) {
#pragma clang fp contract(off)
    CalmResizeAxis a;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = fs;                            // the triangle's support of 1.0, times fs
    a.ss = 1.0 / fs;
    a.kmax = 2 * (in > out ? (in + out - 1) / out : 1) + 1;
    return a;
}

CALM_RESIZE_HD inline double calm_resize_tri(double t) {
#pragma clang fp contract(off)
    if (t < 0.0) t = -t;
    return t < 1.0 ? 1.0 - t : 0.0;
}

CALM_RESIZE_HD inline double calm_resize_weight(const CalmResizeAxis& a, int lo, double center, int j) {
#pragma clang fp contract(off)
    return calm_resize_tri(((double)(j + lo) - center + 0.5) * a.ss);
}

// bounds, centre and weight sum of output pixel o (a loop over its n taps: the sum is taken in tap order)
CALM_RESIZE_HD inline CalmResizeTaps calm_resize_taps(const CalmResizeAxis& a, int in, int o) {
#pragma clang fp contract(off)
    CalmResizeTaps t;
    t.center = ((double)o + 0.5) * a.scale;
    int lo = (int)(t.center - a.support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(t.center + a.support + 0.5);
    if (hi > in) hi = in;
    t.lo = lo;
    t.n = hi - lo;
    double ww = 0.0;
    for (int j = 0; j < t.n; ++j) ww += calm_resize_weight(a, lo, t.center, j);
    t.ww = ww;
    return t;
}

// the fixed-point coefficient of tap j (0 <= j < t.n) of that pixel
CALM_RESIZE_HD inline int32_t calm_resize_k(const CalmResizeAxis& a, const CalmResizeTaps& t, int j) {
#pragma clang fp contract(off)
    double w = calm_resize_weight(a, t.lo, t.center, j);
    if (t.ww != 0.0) w = w / t.ww;
    return (int32_t)(0.5 + w * (double)(1 << CALM_RESIZE_PRECISION_BITS));
}
