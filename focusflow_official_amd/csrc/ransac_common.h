// What the two RANSAC checks of a video session share (epipolar.hip: fundamental matrices from 8 rows; homography.hip:
// homographies from 4): which rows are candidates, the frame normalisation, the hash of the draws, the workspace, the
// compaction launch, the elimination of an 8 x 9 system and the argmax over the hypotheses.  Both checks must see the same rows
// of a session in the same order, so these are spelled once.  Exact fp32: a file that includes this sets
// `#pragma clang fp contract(off)` first.
#pragma once
#include <climits>
#include "ff_common.h"

namespace {

constexpr int MAX_ROWS = 4096;      // N: the slots of a track table, the points of a detector
constexpr int MAX_HYP = 4096;       // K
constexpr int MAX_BATCH = 1024;    // B: a grid dimension, and the workspace stays below 2^31 bytes
constexpr int BLOCK = 1024;         // compact and select: four rows per thread cover MAX_ROWS
constexpr int WAVE = 64;
constexpr int SCORE_WAVES = 4;      // hypotheses per block of the scoring kernel

struct Frame {
    float cx, cy, s;                // xn = (x - cx) s
};

__device__ __forceinline__ unsigned mix(unsigned x) {      // lowbias32
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool finite4(const float4 m) { return isfinite(m.x) && isfinite(m.y) && isfinite(m.z) && isfinite(m.w); }
__device__ __forceinline__ bool candidate(const float4 m, unsigned char valid) { return valid && m.x >= 0.f && finite4(m); }
__device__ __forceinline__ float4 normalise(const float4 m, const Frame fr) {
    return make_float4((m.x - fr.cx) * fr.s, (m.y - fr.cy) * fr.s, (m.z - fr.cx) * fr.s, (m.w - fr.cy) * fr.s);
}

// workspace of one call: M (B) int | planes (B,4,N) float | models (B,K,9) float | counts (B,K) int
struct Workspace {
    int* m;
    float* planes;
    float* models;
    int* counts;
};
__host__ __device__ inline size_t ws_bytes(long long B, long long N, long long K) { return (size_t)(B * (1 + 4 * N + 9 * K + K)) * 4; }
inline Workspace carve(void* ws, long long B, long long N, long long K) {
    Workspace w;
    w.m = static_cast<int*>(ws);
    w.planes = reinterpret_cast<float*>(w.m + B);
    w.models = w.planes + B * 4 * N;
    w.counts = reinterpret_cast<int*>(w.models + B * K * 9);
    return w;
}

// (the host side of both checks: centre and scale of an H x W frame, made in double and rounded once)
inline Frame frame_of(int H, int W) { return {(float)((W - 1) / 2.0), (float)((H - 1) / 2.0), (float)(2.0 / ((double)H + (double)W))}; }

// thread t takes rows 4 t .. 4 t + 3
__global__ void __launch_bounds__(BLOCK) epi_compact_kernel(const float4* __restrict__ matches, const unsigned char* __restrict__ valid, int N, Frame fr,
                                                            Workspace ws) {
    __shared__ int wave_total[BLOCK / WAVE];
    const int b = blockIdx.x, t = threadIdx.x, lane = t % WAVE, wv = t / WAVE;
    matches += (long long)b * N;
    valid += (long long)b * N;
    float4 m[4];
    bool is[4];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = 4 * t + j;
        is[j] = false;
        if (n < N) {
            m[j] = matches[n];
            is[j] = candidate(m[j], valid[n]);
        }
        mine += is[j];
    }
    int incl = mine;      // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < WAVE; d *= 2) {
        const int up = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += up;
    }
    if (lane == WAVE - 1) wave_total[wv] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / WAVE; ++i) {
        const int c = wave_total[i];
        if (i < wv) before += c;
        total += c;
    }
    float* planes = ws.planes + (long long)b * 4 * N;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (is[j]) {
            const float4 p = normalise(m[j], fr);
            planes[before] = p.x;
            planes[N + before] = p.y;
            planes[2 * N + before] = p.z;
            planes[3 * N + before] = p.w;
            ++before;
        }
    if (t == 0) ws.m[b] = total;
}

// A(r, c) of this thread's system, and the unknown a column stands for: LDS as [element][thread]
#define EPI_A(r, c) sys[((r) * 9 + (c)) * WAVE + lane]
#define EPI_PERM(c) perm[(c) * WAVE + lane]

// The 8 x 9 system of lane `lane` in sys (72 x WAVE floats; perm: 9 x WAVE ints): elimination with full pivoting, then
// back-substitution with the free unknown 1 into model[0 .. 8].  -> every step met a pivot > 0 and every unknown is finite.
__device__ __forceinline__ bool solve_8x9(float* sys, int* perm, int lane, float* model) {
#pragma unroll
    for (int c = 0; c < 9; ++c) EPI_PERM(c) = c;
    bool good = true;
#pragma unroll 1
    for (int p = 0; p < 8; ++p) {
        float big = 0.f;
        int pr = p, pc = p;
        for (int r = p; r < 8; ++r)
            for (int c = p; c < 9; ++c) {
                const float a = fabsf(EPI_A(r, c));
                if (a > big) big = a, pr = r, pc = c;      // (strict: the first of equal entries in (row, column) order)
            }
        good = good && big > 0.f;
        for (int c = 0; c < 9; ++c) {      // (pr == p or pc == p: a swap with itself)
            const float u = EPI_A(p, c), v = EPI_A(pr, c);
            EPI_A(p, c) = v;
            EPI_A(pr, c) = u;
        }
        for (int r = 0; r < 8; ++r) {
            const float u = EPI_A(r, p), v = EPI_A(r, pc);
            EPI_A(r, p) = v;
            EPI_A(r, pc) = u;
        }
        const int u = EPI_PERM(p), v = EPI_PERM(pc);
        EPI_PERM(p) = v;
        EPI_PERM(pc) = u;
        const float pivot = EPI_A(p, p);
        for (int r = p + 1; r < 8; ++r) {
            const float factor = __fdiv_rn(EPI_A(r, p), pivot);
            for (int c = p + 1; c < 9; ++c) EPI_A(r, c) = EPI_A(r, c) - factor * EPI_A(p, c);
        }
    }
    // back-substitution, the free unknown 1; z(i) takes the place of A(i, 8)
    model[EPI_PERM(8)] = 1.f;
#pragma unroll 1
    for (int i = 7; i >= 0; --i) {
        float acc = EPI_A(i, 8);
        for (int c = i + 1; c < 8; ++c) acc = acc + EPI_A(i, c) * EPI_A(c, 8);
        const float z = __fdiv_rn(-acc, EPI_A(i, i));
        EPI_A(i, 8) = z;
        good = good && isfinite(z);
        model[EPI_PERM(i)] = z;
    }
    return good;
}

// By a block of BLOCK threads: the largest of counts[0 .. K), the lowest k among equal ones.  Contains a barrier.
__device__ __forceinline__ void best_hypothesis(const int* counts, int K, int& bc, int& bk) {
    __shared__ int best_count[BLOCK / WAVE], best_k[BLOCK / WAVE];
    const int tid = threadIdx.x, lane = tid % WAVE, wv = tid / WAVE;
    bc = -1, bk = INT_MAX;
    for (int k = tid; k < K; k += BLOCK) {
        const int c = counts[k];
        if (c > bc) bc = c, bk = k;      // (k ascends within a thread)
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d /= 2) {
        const int oc = __shfl_xor(bc, d, WAVE), okk = __shfl_xor(bk, d, WAVE);
        if (oc > bc || (oc == bc && okk < bk)) bc = oc, bk = okk;
    }
    if (lane == 0) best_count[wv] = bc, best_k[wv] = bk;
    __syncthreads();
    bc = best_count[0], bk = best_k[0];
#pragma unroll
    for (int i = 1; i < BLOCK / WAVE; ++i) {
        const int oc = best_count[i], okk = best_k[i];
        if (oc > bc || (oc == bc && okk < bk)) bc = oc, bk = okk;
    }
}

}  // namespace

#define FF_REQUIRE_RANSAC_SHAPE(name)                                                                                    \
    FF_REQUIRE(B > 0 && B <= MAX_BATCH, name ": B = %d (1 .. %d samples)", B, MAX_BATCH);                                   \
    FF_REQUIRE(N >= 1 && N <= MAX_ROWS, name ": N = %d (1 .. %d rows)", N, MAX_ROWS);                                    \
    FF_REQUIRE(K >= 1 && K <= MAX_HYP, name ": K = %d (1 .. %d hypotheses)", K, MAX_HYP)
