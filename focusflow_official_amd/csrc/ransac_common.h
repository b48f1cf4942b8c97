// What the two RANSAC checks of a video session share (epipolar.hip: fundamental matrices from 8 rows; homography.hip:
// homographies from 4), which is everything but the model: which rows are candidates, the frame normalisation, the workspace, the
// four launches (compaction; draws, elimination of an 8 x 9 system; scoring; argmax, verdict and flags), templates over a Model,
// and the host function that checks the arguments and enqueues them.  Both checks must see the same rows of a session in the
// same order, so these are spelled once.  Exact fp32: a file that includes this sets `#pragma clang fp contract(off)` first.
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

using ff::mix;

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

// num / den of a judge; a vanishing den measures nothing: 0 for an inlier (num = 0 too), else +inf
__device__ __forceinline__ float quotient(float num, float den, bool in) { return den > 0.f ? __fdiv_rn(num, den) : (in ? 0.f : __builtin_inff()); }

// ---- the three launches behind the compaction, once.  What a check brings is its Model:
//   SAMPLE                         the rows of a minimal sample (at most 8)
//   PLANAR                         (host) the check has a second verdict: planar_permille and the `planar` output are required
//   rows(sys, lane, j, x, y, xp, yp)   what draw j, the normalised row [x, y, x', y'], puts into this thread's 8 x 9 system
//   accept(good, model, px, py)    behind solve_8x9 (-> good): may refuse the model of the sample (px, py)[0 .. SAMPLE) or rewrite
//                                  it in place.  -> good
//   judge(m, p, t, d2) -> inlier   THE expression of the scoring pass and of the final flags; d2: the squared distance of row p
//                                  to model m in normalised units, +inf where there is none
//   to_pixels(g, fr, out)          the best model in pixel coordinates from g = m T, T = [[s, 0, -cx s], [0, s, -cy s], [0, 0, 1]]

// one thread per hypothesis: SAMPLE distinct ranks (Floyd), the system, elimination with full pivoting, back-substitution.  The
// system lives in LDS as [element][thread]: a pivot's row and column are run-time indices, which a register array would answer
// with scratch, and lane l of a wave reads bank l mod 64 whatever element it asks for
template <class Model>
__global__ void __launch_bounds__(WAVE) ransac_hypotheses_kernel(int N, int K, unsigned seed, const int* __restrict__ epoch, Workspace ws) {
    constexpr int S = Model::SAMPLE;
    __shared__ float sys[72 * WAVE];
    __shared__ int perm[9 * WAVE];
    const int b = blockIdx.y, lane = threadIdx.x, k = blockIdx.x * WAVE + lane;
    if (k >= K) return;      // (no barrier below: a thread works on its own column of the LDS arrays)
    const int M = ws.m[b];
    int* count = ws.counts + (long long)b * K + k;
    if (M < S) {
        *count = -1;
        return;
    }
    // the draws: Floyd's algorithm, S distinct ranks below M
    unsigned h = mix(seed + 0x9e3779b9u);
    h = mix(h ^ (unsigned)*epoch);
    h = mix(h ^ (unsigned)b);
    int pick[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const int n = M - S + j;
        int t = (int)(mix(h ^ (unsigned)(S * k + j)) % (unsigned)(n + 1));
        bool taken = false;
#pragma unroll
        for (int i = 0; i < j; ++i) taken |= pick[i] == t;
        pick[j] = taken ? n : t;
    }
    const float* planes = ws.planes + (long long)b * 4 * N;
    float px[S], py[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const float x = planes[pick[j]], y = planes[N + pick[j]], xp = planes[2 * N + pick[j]], yp = planes[3 * N + pick[j]];
        px[j] = x, py[j] = y;
        Model::rows(sys, lane, j, x, y, xp, yp);
    }
    float* model = ws.models + ((long long)b * K + k) * 9;
    const bool good = Model::accept(solve_8x9(sys, perm, lane, model), model, px, py);
    *count = good ? 0 : -1;
}

// one wave per hypothesis: lanes over the candidates, the inlier count by ballot and popcount.  counts in: 0 a model, -1
// degenerate; out: the inliers (0 for a degenerate hypothesis)
template <class Model>
__global__ void __launch_bounds__(SCORE_WAVES* WAVE) ransac_score_kernel(int N, int K, float t, Workspace ws) {
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
                float d2;
                in = Model::judge(f, make_float4(planes[r], planes[N + r], planes[2 * N + r], planes[3 * N + r]), t, d2);
            }
            inliers += __popcll(__ballot(in));
        }
    }
    if (lane == 0) *count = inliers;
}

// one block per sample: argmax over K (the lowest k of equal counts), the verdict - none for a sample that `hold` (null: no
// sample) names -, `planar` (null: the check has none), then per row status, dist2, valid and the culled table; the model; the
// epoch word
template <class Model>
__global__ void __launch_bounds__(BLOCK) ransac_select_kernel(const float4* __restrict__ matches, unsigned char* __restrict__ valid, int N, int K, Frame fr,
                                                              float t, float s2, int min_inliers, int permille, int planar_permille, int cull,
                                                              float2* __restrict__ pos, long long* __restrict__ ids, int* __restrict__ age,
                                                              float* __restrict__ model_out, float* __restrict__ dist2,
                                                              unsigned char* __restrict__ status, int* __restrict__ inliers, int* __restrict__ candidates,
                                                              unsigned char* __restrict__ ok_out, unsigned char* __restrict__ planar_out,
                                                              int* __restrict__ epoch, const unsigned char* __restrict__ hold, Workspace ws) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int bc, bk;
    best_hypothesis(ws.counts + (long long)b * K, K, bc, bk);
    const int M = ws.m[b];
    const bool held = hold && hold[b];      // (ff_epipolar_ransac_hold: this sample gets no verdict, whatever its hypotheses scored)
    const bool ok = !held && M >= Model::SAMPLE && bc >= min_inliers && 1000ll * bc >= (long long)permille * M;
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
                float d2;
                const bool in = Model::judge(f, normalise(m, fr), t, d2);
                d = __fdiv_rn(d2, s2);
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
        if (planar_out) planar_out[b] = ok && 1000ll * bc >= (long long)planar_permille * M;
        float g[9];      // (all zero without a verdict, and so is the model)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            g[3 * i] = f[3 * i] * fr.s;
            g[3 * i + 1] = f[3 * i + 1] * fr.s;
            g[3 * i + 2] = f[3 * i + 2] - (g[3 * i] * fr.cx + g[3 * i + 1] * fr.cy);
        }
        Model::to_pixels(g, fr, model_out + b * 9);
        if (b == 0) *epoch = *epoch + 1;      // (the hypotheses of this call read it in an earlier launch)
    }
}

inline int ws_or_0(int B, int N, int K) {      // ff_*_ws: 0 for a shape that the check refuses
    if (B <= 0 || B > MAX_BATCH || N < 1 || N > MAX_ROWS || K < 1 || K > MAX_HYP) return 0;
    return (int)ws_bytes(B, N, K);
}

// The host side of a check: its argument checks under the entry's `name`, then the four launches on `stream`.  A Model without
// PLANAR passes planar_permille 0 and planar null.
template <class Model>
int ransac(const char* name, const float* matches, unsigned char* valid, int B, int N, int H, int W, float threshold, int K, int min_inliers, int permille,
           int planar_permille, unsigned int seed, int* epoch, int cull, float* pos, long long* ids, int* age, float* model, float* dist2,
           unsigned char* status, int* inliers, int* candidates, unsigned char* ok, unsigned char* planar, void* ws, long long ws_size,
           const unsigned char* hold, void* stream) {
    FF_REQUIRE(B > 0 && B <= MAX_BATCH, "%s: B = %d (1 .. %d samples)", name, B, MAX_BATCH);
    FF_REQUIRE(N >= 1 && N <= MAX_ROWS, "%s: N = %d (1 .. %d rows)", name, N, MAX_ROWS);
    FF_REQUIRE(K >= 1 && K <= MAX_HYP, "%s: K = %d (1 .. %d hypotheses)", name, K, MAX_HYP);
    FF_REQUIRE(H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 24), "%s: H = %d, W = %d (1 .. 2^24: positions are fp32)", name, H, W);
    FF_REQUIRE(threshold >= 0.f && threshold < __builtin_inff(), "%s: threshold = %g (>= 0 and finite, no NaN)", name, (double)threshold);
    FF_REQUIRE(min_inliers >= 1, "%s: min_inliers = %d (at least 1: a degenerate hypothesis scores 0)", name, min_inliers);
    FF_REQUIRE(permille >= 0 && permille <= 1000, "%s: permille = %d (0 .. 1000)", name, permille);
    FF_REQUIRE(planar_permille >= 0 && planar_permille <= 1000, "%s: planar_permille = %d (0 .. 1000)", name, planar_permille);
    FF_REQUIRE(matches && valid && epoch && model && dist2 && status && inliers && candidates && ok && (planar || !Model::PLANAR) && ws, "%s: null pointer",
               name);
    FF_REQUIRE((pos && ids && age) || (!pos && !ids && !age), "%s: a track table is pos, ids and age: all three or none", name);
    FF_REQUIRE(((size_t)matches & 15) == 0 && ((size_t)pos & 7) == 0, "%s: matches must be 16-byte aligned, pos 8-byte aligned", name);
    FF_REQUIRE(((size_t)ws & 15) == 0 && ws_size >= (long long)ws_bytes(B, N, K), "%s: ws must be 16-byte aligned and hold %lld bytes, got %lld", name,
               (long long)ws_bytes(B, N, K), ws_size);
    const Frame fr = frame_of(H, W);
    const float t = (float)((double)threshold * (double)threshold * (double)fr.s * (double)fr.s), s2 = (float)((double)fr.s * (double)fr.s);
    const Workspace w = carve(ws, B, N, K);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const float4* m4 = reinterpret_cast<const float4*>(matches);
    epi_compact_kernel<<<B, BLOCK, 0, s>>>(m4, valid, N, fr, w);
    ransac_hypotheses_kernel<Model><<<dim3((K + WAVE - 1) / WAVE, B), WAVE, 0, s>>>(N, K, seed, epoch, w);
    ransac_score_kernel<Model><<<dim3((K + SCORE_WAVES - 1) / SCORE_WAVES, B), SCORE_WAVES * WAVE, 0, s>>>(N, K, t, w);
    ransac_select_kernel<Model><<<B, BLOCK, 0, s>>>(m4, valid, N, K, fr, t, s2, min_inliers, permille, planar_permille, cull, reinterpret_cast<float2*>(pos),
                                                    ids, age, model, dist2, status, inliers, candidates, ok, planar, epoch, hold, w);
    return ff::check_launch(name);
}

}  // namespace
