// Epipolar check of a video session (frames.FrameSequence(epipolar=...), geometry.EpipolarCheck): a RANSAC over 8-point
// fundamental matrices (Fischler & Bolles 1981; normalised coordinates after Hartley 1997) on the rows of a matches / valid
// pair, scored by the Sampson distance.  Definitions: include/focusflow_hip.h; restated in numpy by tests/epipolar_ref.py.
// Every step is exact (fp32, every operation rounded separately: no FMA; the draws are a 32-bit integer hash), so the tests ask
// for equality.  Everything but the model is shared with the homography check (homography.hip) and lives in ransac_common.h:
//
//   epi_compact_kernel                      one block per sample: the candidate rows in row order (a prefix sum over N <= 4096),
//                                           their normalised coordinates as four planes, their number M
//   ransac_hypotheses_kernel<Fundamental>   one thread per hypothesis: 8 distinct ranks (Floyd), the 8 x 9 system in LDS,
//                                           elimination with full pivoting, back-substitution
//   ransac_score_kernel<Fundamental>        one wave per hypothesis: lanes over the candidates, the inlier count by ballot and popcount
//   ransac_select_kernel<Fundamental>       one block per sample: argmax over K (the lowest k of equal counts), the verdict, then per
//                                           row status, dist2, valid and the culled table; F; the epoch word
//
// Everything is a few million flops per frame: what counts is the number of launches (four) and their latency.  Every output
// element is written by exactly one thread: no atomics, no allocation, no synchronisation; every launch goes to the caller's
// stream.
#pragma clang fp contract(off)
#include "ransac_common.h"

namespace {

struct Fundamental {
    static constexpr int SAMPLE = 8;
    static constexpr bool PLANAR = false;

    // x'^t F x = 0: one row per draw
    static __device__ __forceinline__ void rows(float* sys, int lane, int j, float x, float y, float xp, float yp) {
        EPI_A(j, 0) = xp * x;
        EPI_A(j, 1) = xp * y;
        EPI_A(j, 2) = xp;
        EPI_A(j, 3) = yp * x;
        EPI_A(j, 4) = yp * y;
        EPI_A(j, 5) = yp;
        EPI_A(j, 6) = x;
        EPI_A(j, 7) = y;
        EPI_A(j, 8) = 1.f;
    }

    static __device__ __forceinline__ bool accept(bool good, float*, const float*, const float*) { return good; }

    // Sampson: x' F x squared over the squared gradient norm.
    static __device__ __forceinline__ bool judge(const float* f, const float4 p, float t, float& d2) {
        const float fx0 = (f[0] * p.x + f[1] * p.y) + f[2];
        const float fx1 = (f[3] * p.x + f[4] * p.y) + f[5];
        const float fx2 = (f[6] * p.x + f[7] * p.y) + f[8];
        const float ft0 = (f[0] * p.z + f[3] * p.w) + f[6];
        const float ft1 = (f[1] * p.z + f[4] * p.w) + f[7];
        const float e = (p.z * fx0 + p.w * fx1) + fx2;
        const float num = e * e;
        const float den = ((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1;
        const bool in = num <= t * den;
        d2 = quotient(num, den, in);
        return in;
    }

    // T^t F T from g = F T
    static __device__ __forceinline__ void to_pixels(const float* g, const Frame fr, float* F) {
        float out[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            out[j] = fr.s * g[j];
            out[3 + j] = fr.s * g[3 + j];
            out[6 + j] = g[6 + j] - (out[j] * fr.cx + out[3 + j] * fr.cy);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = out[i];
    }
};

}  // namespace

extern "C" int ff_epipolar_ws(int B, int N, int K) { return ws_or_0(B, N, K); }

extern "C" int ff_epipolar_ransac_hold(const float* matches, unsigned char* valid, int B, int N, int H, int W, float threshold, int K,
                                       int min_inliers, int permille, unsigned int seed, int* epoch, int cull, float* pos, long long* ids, int* age,
                                       float* F, float* dist2, unsigned char* status, int* inliers, int* candidates, unsigned char* ok, void* ws,
                                       long long ws_size, const unsigned char* hold, void* stream) {
    return ransac<Fundamental>("ff_epipolar_ransac", matches, valid, B, N, H, W, threshold, K, min_inliers, permille, 0, seed, epoch, cull, pos, ids, age, F,
                               dist2, status, inliers, candidates, ok, nullptr, ws, ws_size, hold, stream);
}

extern "C" int ff_epipolar_ransac(const float* matches, unsigned char* valid, int B, int N, int H, int W, float threshold, int K, int min_inliers,
                                  int permille, unsigned int seed, int* epoch, int cull, float* pos, long long* ids, int* age, float* F,
                                  float* dist2, unsigned char* status, int* inliers, int* candidates, unsigned char* ok, void* ws,
                                  long long ws_size, void* stream) {
    return ff_epipolar_ransac_hold(matches, valid, B, N, H, W, threshold, K, min_inliers, permille, seed, epoch, cull, pos, ids, age, F, dist2, status,
                                   inliers, candidates, ok, ws, ws_size, nullptr, stream);
}
