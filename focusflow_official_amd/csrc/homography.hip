// Homography check of a video session (frames.FrameSequence(homography=...), geometry.HomographyCheck): a RANSAC over 4-point
// homographies (the DLT of Hartley & Zisserman, alg. 4.1, on frame-normalised coordinates) on the rows of a matches / valid
// pair, scored by the one-sided transfer error, with a verdict on whether ONE plane-induced map (a planar scene, or a camera
// that only rotates) explains the pair; and the dense residual of a flow field against that map.  Definitions:
// include/focusflow_hip.h; restated in numpy by tests/homography_ref.py.  Everything but the model - candidates, normalisation,
// draws, workspace and the four launches - is that of the epipolar check (ransac_common.h), so both see the same rows of a session.
// Every step is exact (fp32, every operation rounded separately: no FMA), so the tests ask for equality.
//
//   epi_compact_kernel                     the candidate rows in row order as four planes, their number M
//   ransac_hypotheses_kernel<Homography>   one thread per hypothesis: 4 distinct ranks (Floyd), the 8 x 9 DLT system in LDS,
//                                          elimination with full pivoting, back-substitution; the sign of w on its own four points
//   ransac_score_kernel<Homography>        one wave per hypothesis: lanes over the candidates, the inlier count by ballot and popcount
//   ransac_select_kernel<Homography>       one block per sample: argmax over K, the two verdicts (ok, planar), per row status, dist2,
//                                          valid and the culled table; H; the epoch word
//   hom_residual_kernel                    one thread per four pixels of a row: |(x + u, y + v) - pi(H (x, y, 1))|^2, a single pass
//                                          over the flow
//
// Every output element is written by exactly one thread: no atomics, no allocation, no synchronisation; every launch goes to the
// caller's stream.
#pragma clang fp contract(off)
#include "ransac_common.h"

namespace {

struct Homography {
    static constexpr int SAMPLE = 4;
    static constexpr bool PLANAR = true;

    // (x', y', 1) ~ H (x, y, 1): the two DLT rows of a draw
    static __device__ __forceinline__ void rows(float* sys, int lane, int j, float x, float y, float xp, float yp) {
        EPI_A(2 * j, 0) = x;
        EPI_A(2 * j, 1) = y;
        EPI_A(2 * j, 2) = 1.f;
        EPI_A(2 * j, 3) = 0.f;
        EPI_A(2 * j, 4) = 0.f;
        EPI_A(2 * j, 5) = 0.f;
        EPI_A(2 * j, 6) = -(xp * x);
        EPI_A(2 * j, 7) = -(xp * y);
        EPI_A(2 * j, 8) = -xp;
        EPI_A(2 * j + 1, 0) = 0.f;
        EPI_A(2 * j + 1, 1) = 0.f;
        EPI_A(2 * j + 1, 2) = 0.f;
        EPI_A(2 * j + 1, 3) = x;
        EPI_A(2 * j + 1, 4) = y;
        EPI_A(2 * j + 1, 5) = 1.f;
        EPI_A(2 * j + 1, 6) = -(yp * x);
        EPI_A(2 * j + 1, 7) = -(yp * y);
        EPI_A(2 * j + 1, 8) = -yp;
    }

    // w on the sample's own points: strictly of one sign, or three of them are collinear or the map folds the plane.  (The
    // thread wrote the nine values it reads back.)
    static __device__ __forceinline__ bool accept(bool good, float* model, const float* px, const float* py) {
        float hm[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) hm[i] = model[i];
        int pos = 0, neg = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float w = (hm[6] * px[j] + hm[7] * py[j]) + hm[8];
            pos += w > 0.f;
            neg += w < 0.f;
        }
        good = good && (pos == 4 || neg == 4);
        if (good && neg == 4) {      // (exact: every stored model has w > 0 on its sample)
#pragma unroll
            for (int i = 0; i < 9; ++i) model[i] = -hm[i];
        }
        return good;
    }

    // The one-sided transfer error in the second image; a row that the map sends to w <= 0 is no inlier and has no distance.
    static __device__ __forceinline__ bool judge(const float* h, const float4 p, float t, float& d2) {
        const float u = (h[0] * p.x + h[1] * p.y) + h[2];
        const float v = (h[3] * p.x + h[4] * p.y) + h[5];
        const float w = (h[6] * p.x + h[7] * p.y) + h[8];
        const float du = u - p.z * w, dv = v - p.w * w;
        const float num = du * du + dv * dv;
        const float den = w * w;
        const bool in = w > 0.f && num <= t * den;
        d2 = w > 0.f ? quotient(num, den, in) : __builtin_inff();
        return in;
    }

    // T^-1 Hn T from g = Hn T
    static __device__ __forceinline__ void to_pixels(const float* g, const Frame fr, float* H) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            H[j] = __fdiv_rn(g[j], fr.s) + fr.cx * g[6 + j];
            H[3 + j] = __fdiv_rn(g[3 + j], fr.s) + fr.cy * g[6 + j];
            H[6 + j] = g[6 + j];
        }
    }
};

// One pixel of the residual: the flow's target against the map's.
__device__ __forceinline__ float residual_at(const float* h, float x, float y, float u, float v) {
    const float pu = (h[0] * x + h[1] * y) + h[2];
    const float pv = (h[3] * x + h[4] * y) + h[5];
    const float pw = (h[6] * x + h[7] * y) + h[8];
    if (!(pw > 0.f)) return __builtin_inff();
    const float dx = (x + u) - __fdiv_rn(pu, pw), dy = (y + v) - __fdiv_rn(pv, pw);
    return dx * dx + dy * dy;
}

constexpr int RES_X = 64, RES_Y = 4;      // a block: 64 threads of four pixels along x (a wave reads 1 KB of a row), four rows

// Memory bound: 8 B read and 4 B written per pixel, every byte once.  A thread takes four consecutive pixels of a row; where the
// three addresses are 16-byte aligned (a dense innermost dimension, the usual crop) it moves them as float4, else one by one.
__global__ void __launch_bounds__(RES_X* RES_Y) hom_residual_kernel(const float* __restrict__ flow, long long ld_b, long long ld_c, long long ld_row,
                                                                    long long ld_col, const float* __restrict__ Hm, const unsigned char* __restrict__ ok,
                                                                    int H, int W, float* __restrict__ out) {
    const int b = blockIdx.z, y = blockIdx.y * RES_Y + threadIdx.y, x0 = 4 * (blockIdx.x * RES_X + threadIdx.x);
    if (y >= H || x0 >= W) return;
    float* o = out + ((long long)b * H + y) * W + x0;
    const int n = min(4, W - x0);
    const bool vec_out = n == 4 && ((size_t)o & 15) == 0;
    if (!ok[b]) {      // (uniform over the block)
        if (vec_out) {
            *reinterpret_cast<float4*>(o) = make_float4(-1.f, -1.f, -1.f, -1.f);
        } else {
            for (int i = 0; i < n; ++i) o[i] = -1.f;
        }
        return;
    }
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = Hm[b * 9 + i];
    const float* u = flow + b * ld_b + y * ld_row + x0 * ld_col;
    const float* v = u + ld_c;
    const float fy = (float)y;
    if (vec_out && ld_col == 1 && (((size_t)u | (size_t)v) & 15) == 0) {
        const float4 u4 = *reinterpret_cast<const float4*>(u), v4 = *reinterpret_cast<const float4*>(v);
        *reinterpret_cast<float4*>(o) = make_float4(residual_at(h, (float)x0, fy, u4.x, v4.x), residual_at(h, (float)(x0 + 1), fy, u4.y, v4.y),
                                                    residual_at(h, (float)(x0 + 2), fy, u4.z, v4.z), residual_at(h, (float)(x0 + 3), fy, u4.w, v4.w));
    } else {
        for (int i = 0; i < n; ++i) o[i] = residual_at(h, (float)(x0 + i), fy, u[i * ld_col], v[i * ld_col]);
    }
}

}  // namespace

extern "C" int ff_homography_ws(int B, int N, int K) { return ws_or_0(B, N, K); }

extern "C" int ff_homography_ransac(const float* matches, unsigned char* valid, int B, int N, int H, int W, float threshold, int K, int min_inliers,
                                    int permille, int planar_permille, unsigned int seed, int* epoch, int cull, float* pos, long long* ids, int* age,
                                    float* Hout, float* dist2, unsigned char* status, int* inliers, int* candidates, unsigned char* ok,
                                    unsigned char* planar, void* ws, long long ws_size, void* stream) {
    return ransac<Homography>("ff_homography_ransac", matches, valid, B, N, H, W, threshold, K, min_inliers, permille, planar_permille, seed, epoch, cull, pos,
                              ids, age, Hout, dist2, status, inliers, candidates, ok, planar, ws, ws_size, nullptr, stream);
}

extern "C" int ff_homography_residual(const float* flow, long long ld_b, long long ld_c, long long ld_row, long long ld_col, const float* Hm,
                                      const unsigned char* ok, int B, int Himg, int Wimg, float* out, void* stream) {
    FF_REQUIRE(B > 0 && B <= 65535, "ff_homography_residual: B = %d (1 .. 65535: a grid dimension)", B);
    FF_REQUIRE(Himg > 0 && Wimg > 0 && Himg <= (1 << 18) && Wimg <= (1 << 24), "ff_homography_residual: H = %d (1 .. 2^18), W = %d (1 .. 2^24)", Himg, Wimg);
    FF_REQUIRE(flow && Hm && ok && out, "ff_homography_residual: null pointer");
    FF_REQUIRE(ld_b >= 0 && ld_c >= 0 && ld_row >= 0 && ld_col >= 0, "ff_homography_residual: negative stride");
    FF_REQUIRE(((size_t)flow & 3) == 0 && ((size_t)out & 3) == 0, "ff_homography_residual: flow and out must be 4-byte aligned");
    const dim3 grid((Wimg + 4 * RES_X - 1) / (4 * RES_X), (Himg + RES_Y - 1) / RES_Y, B);
    hom_residual_kernel<<<grid, dim3(RES_X, RES_Y), 0, static_cast<hipStream_t>(stream)>>>(flow, ld_b, ld_c, ld_row, ld_col, Hm, ok, Himg, Wimg, out);
    return ff::check_launch("ff_homography_residual");
}
