// Tiled layout of the correlation pyramid (CorrBlock, corr.py:12-27), shared by the build, lookup and backward kernels.
//
// Level l of query i is a plane of h_l x w_l values (h_l = h0 >> l: avg_pool2d floors).  A plane is stored as 128-byte
// 2-D tiles so that the 11 x 11 window a lookup reads touches few HBM lines:
//     fp32 storage: tile = 8 wide x 4 high floats        fp16 storage: tile = 8 wide x 8 high halfs
//     element (y, x)  ->  ((y / TH) * ntx + (x / 8)) * (8 * TH) + (y % TH) * 8 + (x % 8)
// The tile grid covers the plane padded to the build kernel's 16 x 8 patch of level-0 positions (wp0 = ceil16(w0),
// hp0 = ceil8(h0), level l: wp0 >> l by hp0 >> l), rounded up to whole tiles.  Pad elements are ZERO by contract
// (ff_corr_build clears what its patches do not cover; ff_corr_retile fills zero-initialised storage; the backward
// kernels mask their updates), so the lookup needs no per-element masks.
#pragma once
#include <hip/hip_runtime.h>

namespace ff {

// One separately-rounded replay of the sampler's coordinate chain (corr.py:41-43, utils.py:61-62, ATen's un-normalise): the
// corner and weight of one axis, for the plain lookup (corr.hip) and the tiled pyramid's backward (corr_lookup_tiled.hip) alike.
__device__ __forceinline__ void tap_1d(float c, float inv_scale, int off, int n, int& i0, float& w1) {
    const float cl = __fmul_rn(c, inv_scale);                 // coords / 2**i   (exact: power of two)
    const float x = __fadd_rn(cl, (float)off);                // + delta
    const float nm1 = (float)(n - 1);
    const float g = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, x), nm1), 1.f);   // 2*x/(n-1) - 1
    const float u = __fmul_rn(__fmul_rn(__fadd_rn(g, 1.f), 0.5f), nm1);  // ((g+1)/2)*(n-1)
    const float f = floorf(u);
    i0 = (int)f;
    w1 = __fsub_rn(u, f);
}

struct CorrLayout {
    int h[4], w[4];        // plane sizes
    int ntx[4], nty[4];    // tile grid
    int plane[4];          // elements per plane (ntx * nty * 8 * th)
    int th;                // tile height: 4 (fp32) or 8 (fp16)
    int npx, npy;          // 16 x 8 patches of level 0
};

__host__ __device__ inline CorrLayout corr_layout(int h0, int w0, bool half) {
    CorrLayout L;
    L.th = half ? 8 : 4;
    L.npx = (w0 + 15) / 16;
    L.npy = (h0 + 7) / 8;
    for (int l = 0; l < 4; ++l) {
        L.h[l] = h0 >> l;
        L.w[l] = w0 >> l;
        const int wp = (L.npx * 16) >> l, hp = (L.npy * 8) >> l;
        L.ntx[l] = (wp + 7) / 8;
        L.nty[l] = (hp + L.th - 1) / L.th;
        L.plane[l] = L.ntx[l] * L.nty[l] * 8 * L.th;
    }
    return L;
}

// element offset inside a plane; TH = 4 or 8
template <int TH>
__host__ __device__ inline int tiled_offset(int y, int x, int ntx) {
    return ((y / TH) * ntx + (x >> 3)) * (8 * TH) + (y % TH) * 8 + (x & 7);
}

}  // namespace ff
