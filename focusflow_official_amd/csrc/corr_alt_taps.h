// The on-the-fly correlation's tap arithmetic (corr_alt.hip's lookup, corr_alt_bwd.hip's backward): one definition, so the
// backward scatters through exactly the corners and weights the forward blended.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int BIG = 1 << 24;          // tap indices are clamped to +-BIG for the window geometry (wild coordinates)

// corr_lookup_dma.hip's taps_a for one axis: x = c 2^-l + off, g = 2 x / (n - 1) - 1 as the correctly rounded quotient (two
// exact remainders), u = ((g + 1) / 2) (n - 1), corner floor(u), weight u - floor(u) - every step a separately rounded fp32
// operation, so the corners and weights are bit-identical to the tiled lookup's (and to grid_sample's).
__device__ __forceinline__ void tap(float c, float inv, float off, float nm1, float r2, int& i0, float& wgt) {
    const float x = __fadd_rn(__fmul_rn(c, inv), off);
    const float dh = 0.5f * nm1;
    const float q0 = __fmul_rn(x, r2);
    const float e0 = __builtin_fmaf(-q0, dh, x);
    const float q1 = __builtin_fmaf(e0, r2, q0);
    const float e1 = __builtin_fmaf(-q1, dh, x);
    const float g = __fsub_rn(__builtin_fmaf(e1, r2, q1), 1.f);
    const float u = __fmul_rn(__fmul_rn(__fadd_rn(g, 1.f), 0.5f), nm1);
    const float f = floorf(u);
    i0 = (int)f;
    wgt = __fsub_rn(u, f);
}

__device__ __forceinline__ int clampi(int v) { return min(max(v, -BIG), BIG); }

}  // namespace
