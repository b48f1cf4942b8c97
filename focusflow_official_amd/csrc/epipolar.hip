// Epipolar check of a video session (frames.FrameSequence(epipolar=...), geometry.EpipolarCheck): a RANSAC over 8-point
// fundamental matrices (Fischler & Bolles 1981; normalised coordinates after Hartley 1997) on the rows of a matches / valid
// pair, scored by the Sampson distance.  Definitions: include/focusflow_hip.h; restated in numpy by tests/epipolar_ref.py.
// Every step is exact (fp32, every operation rounded separately: no FMA; the draws are a 32-bit integer hash), so the tests ask
// for equality.  What the homography check (homography.hip) shares with it - candidates, normalisation, hash, workspace, the
// compaction launch, the elimination, the argmax - lives in ransac_common.h.
//
//   epi_compact_kernel      (ransac_common.h) one block per sample: the candidate rows in row order (a prefix sum over N <= 4096), their
//                           normalised coordinates as four planes, their number M
//   epi_hypotheses_kernel   one thread per hypothesis: 8 distinct ranks (Floyd), the 8 x 9 system, elimination with full
//                           pivoting, back-substitution.  The system lives in LDS as [element][thread]: a pivot's row and column are
//                           run-time indices, which a register array would answer with scratch, and lane l of a wave reads bank
//                           l mod 64 whatever element it asks for
//   epi_score_kernel        one wave per hypothesis: lanes over the candidates, the inlier count by ballot and popcount
//   epi_select_kernel       one block per sample: argmax over K (the lowest k of equal counts), the verdict, then per row status,
//                           dist2, valid and the culled table; F; the epoch word
//
// Everything is a few million flops per frame: what counts is the number of launches (four) and their latency.  Every output
// element is written by exactly one thread: no atomics, no allocation, no synchronisation; every launch goes to the caller's
// stream.
#pragma clang fp contract(off)
#include "ransac_common.h"

namespace {

// The one expression of the scoring pass and of the final flags: x' F x squared, and the squared gradient norm.
__device__ __forceinline__ void sampson(const float* f, const float4 p, float& num, float& den) {
    const float fx0 = (f[0] * p.x + f[1] * p.y) + f[2];
    const float fx1 = (f[3] * p.x + f[4] * p.y) + f[5];
    const float fx2 = (f[6] * p.x + f[7] * p.y) + f[8];
    const float ft0 = (f[0] * p.z + f[3] * p.w) + f[6];
    const float ft1 = (f[1] * p.z + f[4] * p.w) + f[7];
    const float e = (p.z * fx0 + p.w * fx1) + fx2;
    num = e * e;
    den = ((fx0 * fx0 + fx1 * fx1) + ft0 * ft0) + ft1 * ft1;
}

__global__ void __launch_bounds__(WAVE) epi_hypotheses_kernel(int N, int K, unsigned seed, const int* __restrict__ epoch, Workspace ws) {
    __shared__ float sys[72 * WAVE];
    __shared__ int perm[9 * WAVE];
    const int b = blockIdx.y, lane = threadIdx.x, k = blockIdx.x * WAVE + lane;
    if (k >= K) return;      // (no barrier below: a thread works on its own column of the LDS arrays)
    const int M = ws.m[b];
    int* count = ws.counts + (long long)b * K + k;
    if (M < 8) {
        *count = -1;
        return;
    }
    // the draws: Floyd's algorithm, 8 distinct ranks below M
    unsigned h = mix(seed + 0x9e3779b9u);
    h = mix(h ^ (unsigned)*epoch);
    h = mix(h ^ (unsigned)b);
    int pick[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = M - 8 + j;
        int t = (int)(mix(h ^ (unsigned)(8 * k + j)) % (unsigned)(n + 1));
        bool taken = false;
#pragma unroll
        for (int i = 0; i < j; ++i) taken |= pick[i] == t;
        pick[j] = taken ? n : t;
    }
    const float* planes = ws.planes + (long long)b * 4 * N;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = planes[pick[j]], y = planes[N + pick[j]], xp = planes[2 * N + pick[j]], yp = planes[3 * N + pick[j]];
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
    const bool good = solve_8x9(sys, perm, lane, ws.models + ((long long)b * K + k) * 9);
    *count = good ? 0 : -1;
}

// counts in: 0 a model, -1 degenerate; out: the inliers (0 for a degenerate hypothesis)
__global__ void __launch_bounds__(SCORE_WAVES* WAVE) epi_score_kernel(int N, int K, float t, Workspace ws) {
    const int b = blockIdx.y, lane = threadIdx.x % WAVE, k = blockIdx.x * SCORE_WAVES + threadIdx.x / WAVE;
    if (k >= K) return;
    int* count = ws.counts + (long long)b * K + k;
    const int M = ws.m[b];
    int inliers = 0;
    if (*count == 0) {      // (uniform over the wave)
        const float* model = ws.models + ((long long)b * K + k) * 9;
        float f[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = model[i];
        const float* planes = ws.planes + (long long)b * 4 * N;
        for (int r0 = 0; r0 < M; r0 += WAVE) {
            const int r = r0 + lane;
            bool in = false;
            if (r < M) {
                float num, den;
                sampson(f, make_float4(planes[r], planes[N + r], planes[2 * N + r], planes[3 * N + r]), num, den);
                in = num <= t * den;
            }
            inliers += __popcll(__ballot(in));
        }
    }
    if (lane == 0) *count = inliers;
}

__global__ void __launch_bounds__(BLOCK) epi_select_kernel(const float4* __restrict__ matches, unsigned char* __restrict__ valid, int N, int K, Frame fr,
                                                           float t, float s2, int min_inliers, int permille, int cull, float2* __restrict__ pos,
                                                           long long* __restrict__ ids, int* __restrict__ age, float* __restrict__ F,
                                                           float* __restrict__ dist2, unsigned char* __restrict__ status,
                                                           int* __restrict__ inliers, int* __restrict__ candidates, unsigned char* __restrict__ ok_out,
                                                           int* __restrict__ epoch, const unsigned char* __restrict__ hold, Workspace ws) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int bc, bk;
    best_hypothesis(ws.counts + (long long)b * K, K, bc, bk);
    const int M = ws.m[b];
    const bool held = hold && hold[b];      // (ff_epipolar_ransac_hold: this sample gets no verdict, whatever its hypotheses scored)
    const bool ok = !held && M >= 8 && bc >= min_inliers && 1000ll * bc >= (long long)permille * M;
    float f[9];
    const float* model = ws.models + ((long long)b * K + bk) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = ok ? model[i] : 0.f;
    for (int n = tid; n < N; n += BLOCK) {
        const long long r = (long long)b * N + n;
        const float4 m = matches[r];
        float d = -1.f;
        unsigned char st = 0;
        if (!(m.x < 0.f)) {      // a row: a no-row holds x = -1
            const bool cand = candidate(m, valid[r]);
            st = cand ? 4 : 2;
            d = __builtin_inff();
            if (ok && finite4(m)) {
                float num, den;
                sampson(f, normalise(m, fr), num, den);
                const bool in = num <= t * den;
                d = __fdiv_rn(den > 0.f ? __fdiv_rn(num, den) : (in ? 0.f : __builtin_inff()), s2);
                if (cand) st = in ? 1 : 3;
            }
        }
        dist2[r] = d;
        status[r] = st;
        if (st == 3) {
            valid[r] = 0;
            if (cull && pos) {
                pos[r] = make_float2(-1.f, -1.f);
                ids[r] = -1;
                age[r] = 0;
            }
        }
    }
    if (tid == 0) {
        inliers[b] = ok ? bc : 0;
        candidates[b] = M;
        ok_out[b] = ok;
        // pixel coordinates: T^t F T with T = [[s, 0, -cx s], [0, s, -cy s], [0, 0, 1]] (all zero without a verdict)
        float g[9], out[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            g[3 * i] = f[3 * i] * fr.s;
            g[3 * i + 1] = f[3 * i + 1] * fr.s;
            g[3 * i + 2] = f[3 * i + 2] - (g[3 * i] * fr.cx + g[3 * i + 1] * fr.cy);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            out[j] = fr.s * g[j];
            out[3 + j] = fr.s * g[3 + j];
            out[6 + j] = g[6 + j] - (out[j] * fr.cx + out[3 + j] * fr.cy);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) F[b * 9 + i] = out[i];
        if (b == 0) *epoch = *epoch + 1;      // (the hypotheses of this call read it in an earlier launch)
    }
}

}  // namespace

extern "C" int ff_epipolar_ws(int B, int N, int K) {
    if (B <= 0 || B > MAX_BATCH || N < 1 || N > MAX_ROWS || K < 1 || K > MAX_HYP) return 0;
    return (int)ws_bytes(B, N, K);
}

extern "C" int ff_epipolar_ransac_hold(const float* matches, unsigned char* valid, int B, int N, int H, int W, float threshold, int K,
                                       int min_inliers, int permille, unsigned int seed, int* epoch, int cull, float* pos, long long* ids, int* age,
                                       float* F, float* dist2, unsigned char* status, int* inliers, int* candidates, unsigned char* ok, void* ws,
                                       long long ws_size, const unsigned char* hold, void* stream) {
    FF_REQUIRE_RANSAC_SHAPE("ff_epipolar_ransac");
    FF_REQUIRE(H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 24), "ff_epipolar_ransac: H = %d, W = %d (1 .. 2^24: positions are fp32)", H, W);
    FF_REQUIRE(threshold >= 0.f && threshold < __builtin_inff(), "ff_epipolar_ransac: threshold = %g (>= 0 and finite, no NaN)", (double)threshold);
    FF_REQUIRE(min_inliers >= 1, "ff_epipolar_ransac: min_inliers = %d (at least 1: a degenerate hypothesis scores 0)", min_inliers);
    FF_REQUIRE(permille >= 0 && permille <= 1000, "ff_epipolar_ransac: permille = %d (0 .. 1000)", permille);
    FF_REQUIRE(matches && valid && epoch && F && dist2 && status && inliers && candidates && ok && ws, "ff_epipolar_ransac: null pointer");
    FF_REQUIRE((pos && ids && age) || (!pos && !ids && !age), "ff_epipolar_ransac: a track table is pos, ids and age: all three or none");
    FF_REQUIRE(((size_t)matches & 15) == 0 && ((size_t)pos & 7) == 0, "ff_epipolar_ransac: matches must be 16-byte aligned, pos 8-byte aligned");
    FF_REQUIRE(((size_t)ws & 15) == 0 && ws_size >= (long long)ws_bytes(B, N, K), "ff_epipolar_ransac: ws must be 16-byte aligned and hold %lld bytes, got %lld",
               (long long)ws_bytes(B, N, K), ws_size);
    const Frame fr = frame_of(H, W);
    const float t = (float)((double)threshold * (double)threshold * (double)fr.s * (double)fr.s), s2 = (float)((double)fr.s * (double)fr.s);
    const Workspace w = carve(ws, B, N, K);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const float4* m4 = reinterpret_cast<const float4*>(matches);
    epi_compact_kernel<<<B, BLOCK, 0, s>>>(m4, valid, N, fr, w);
    epi_hypotheses_kernel<<<dim3((K + WAVE - 1) / WAVE, B), WAVE, 0, s>>>(N, K, seed, epoch, w);
    epi_score_kernel<<<dim3((K + SCORE_WAVES - 1) / SCORE_WAVES, B), SCORE_WAVES * WAVE, 0, s>>>(N, K, t, w);
    epi_select_kernel<<<B, BLOCK, 0, s>>>(m4, valid, N, K, fr, t, s2, min_inliers, permille, cull, reinterpret_cast<float2*>(pos), ids, age, F, dist2,
                                          status, inliers, candidates, ok, epoch, hold, w);
    return ff::check_launch("ff_epipolar_ransac");
}

extern "C" int ff_epipolar_ransac(const float* matches, unsigned char* valid, int B, int N, int H, int W, float threshold, int K, int min_inliers,
                                  int permille, unsigned int seed, int* epoch, int cull, float* pos, long long* ids, int* age, float* F,
                                  float* dist2, unsigned char* status, int* inliers, int* candidates, unsigned char* ok, void* ws,
                                  long long ws_size, void* stream) {
    return ff_epipolar_ransac_hold(matches, valid, B, N, H, W, threshold, K, min_inliers, permille, seed, epoch, cull, pos, ids, age, F, dist2, status,
                                   inliers, candidates, ok, ws, ws_size, nullptr, stream);
}
