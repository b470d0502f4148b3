// The arithmetic of the bilinear upsampling by an integer factor (align_corners = False), stated once: upsample_kernel and
// its gather backward (bn_act.hip) and the fused segmentation loss (seg_loss.hip) all take their taps and their blend from
// here, so an interpolated value has the same bits wherever it is formed.  No contraction of a*b+c into one rounding, whatever
// the including file's setting: ATen's kernel, which the values are compared with bit for bit, rounds every operation.
#pragma once
#include <hip/hip_runtime.h>

namespace irn {

// Output index `o` of an axis with `n` inputs reads inputs i0 and i1 = i0 + 1 (clamped to n - 1) with weights 1 - l and l.
// ATen's upsample_bilinear2d: src = (o + 0.5) / factor - 0.5 clamped at 0, l = src - floor(src); rscale = (float)(1.0 / factor).
struct UpsampleTap {
    int i0, i1;
    float l;
};

__host__ __device__ __forceinline__ UpsampleTap upsample_tap(int o, int n, float rscale) {
#pragma clang fp contract(off)
    float s = rscale * ((float)o + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    const int i0 = (int)s;
    return UpsampleTap{i0, i0 + (i0 < n - 1 ? 1 : 0), s - (float)i0};
}

// a, b: the taps of row i0 at columns x0, x1; c, d: those of row i1.  ly0 = 1 - ly, lx0 = 1 - lx.
__device__ __forceinline__ float upsample_blend(float a, float b, float c, float d, float lx0, float lx, float ly0, float ly) {
#pragma clang fp contract(off)
    return ly0 * (lx0 * a + lx * b) + ly * (lx0 * c + lx * d);
}

// The weight with which input index `i` enters output `o`: both taps where the clamp folds them onto one index.
__device__ __forceinline__ float upsample_weight(int o, int i, int n, float rscale) {
    const UpsampleTap t = upsample_tap(o, n, rscale);
    return (t.i0 == i ? 1.f - t.l : 0.f) + (t.i1 == i ? t.l : 0.f);
}

// Outputs that can touch input index i lie in [factor * i - upsample_below(factor), factor * i + upsample_above(factor)):
// those whose first tap is i - 1 or i (f*i - f/2 - 0.5 <= o < f*i + 3f/2 - 0.5 in exact arithmetic), widened by one output
// on each side for the rounding of the fp32 mapping; an output outside the true support weighs exactly 0.
__host__ __device__ constexpr int upsample_below(int factor) { return factor / 2 + 2; }
__host__ __device__ constexpr int upsample_above(int factor) { return (3 * factor + 1) / 2 + 1; }

}  // namespace irn
