// Whether a calm_rcrop_sample record describes something calm_resized_crop may read and write (include/calm_vit.h lists
// the conditions).  This file is the definition: the kernel of resized_crop.hip calls it before it forms any address and
// calm_resized_crop_check is the same function on the host.  Every comparison is made on 64-bit values, so no sum or
// product of the record's 32-bit fields wraps.
#pragma once
#include <stdint.h>
#include "../../include/calm_vit.h"

#if defined(__HIPCC__)
#define CALM_RCROP_HD __host__ __device__
#else
#define CALM_RCROP_HD
#endif

#define CALM_RCROP_MAX_SIDE 16384

CALM_RCROP_HD inline bool calm_rcrop_valid(const calm_rcrop_sample& s, int64_t nbytes, int32_t H, int32_t W) {
    const int64_t side = CALM_RCROP_MAX_SIDE;
    const int64_t h = s.h, w = s.w, by0 = s.by0, bx0 = s.bx0, bh = s.bh, bw = s.bw, vh = s.vh, vw = s.vw, wy0 = s.wy0,
                  wx0 = s.wx0;
    if (h < 1 || h > side || w < 1 || w > side) return false;
    if (s.offset < 0 || s.offset > nbytes || 3 * h * w > nbytes - s.offset) return false;     // 3 h w <= 3 * 2^28
    if (by0 < 0 || bx0 < 0 || bh < 1 || bw < 1 || by0 + bh > h || bx0 + bw > w) return false;
    if (vh < 1 || vh > side || vw < 1 || vw > side) return false;
    if (H < 1 || W < 1 || wy0 < 0 || wx0 < 0 || wy0 + (int64_t)H > vh || wx0 + (int64_t)W > vw) return false;
    return true;
}
