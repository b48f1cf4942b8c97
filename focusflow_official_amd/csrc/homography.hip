// Homography check of a video session (frames.FrameSequence(homography=...), geometry.HomographyCheck): a RANSAC over 4-point
// homographies (the DLT of Hartley & Zisserman, alg. 4.1, on frame-normalised coordinates) on the rows of a matches / valid
// pair, scored by the one-sided transfer error, with a verdict on whether ONE plane-induced map (a planar scene, or a camera
// that only rotates) explains the pair; and the dense residual of a flow field against that map.  Definitions:
// include/focusflow_hip.h; restated in numpy by tests/homography_ref.py.  Candidates, normalisation, draws' hash, workspace,
// compaction, elimination and argmax are those of the epipolar check (ransac_common.h), so both see the same rows of a session.
// Every step is exact (fp32, every operation rounded separately: no FMA), so the tests ask for equality.
//
//   epi_compact_kernel      (ransac_common.h) the candidate rows in row order as four planes, their number M
//   hom_hypotheses_kernel   one thread per hypothesis: 4 distinct ranks (Floyd), the 8 x 9 DLT system in LDS as [element][thread],
//                           elimination with full pivoting, back-substitution; the sign of w on its own four points
//   hom_score_kernel        one wave per hypothesis: lanes over the candidates, the inlier count by ballot and popcount
//   hom_select_kernel       one block per sample: argmax over K, the two verdicts (ok, planar), per row status, dist2, valid and
//                           the culled table; H; the epoch word
//   hom_residual_kernel     one thread per four pixels of a row: |(x + u, y + v) - pi(H (x, y, 1))|^2, a single pass over the flow
//
// Every output element is written by exactly one thread: no atomics, no allocation, no synchronisation; every launch goes to the
// caller's stream.
#pragma clang fp contract(off)
#include "ransac_common.h"

namespace {

// The one expression of the scoring pass and of the final flags: the one-sided transfer error times w^2, and w^2.
__device__ __forceinline__ void transfer(const float* h, const float4 p, float& num, float& den, float& w) {
    const float u = (h[0] * p.x + h[1] * p.y) + h[2];
    const float v = (h[3] * p.x + h[4] * p.y) + h[5];
    w = (h[6] * p.x + h[7] * p.y) + h[8];
    const float du = u - p.z * w, dv = v - p.w * w;
    num = du * du + dv * dv;
    den = w * w;
}

__global__ void __launch_bounds__(WAVE) hom_hypotheses_kernel(int N, int K, unsigned seed, const int* __restrict__ epoch, Workspace ws) {
    __shared__ float sys[72 * WAVE];
    __shared__ int perm[9 * WAVE];
    const int b = blockIdx.y, lane = threadIdx.x, k = blockIdx.x * WAVE + lane;
    if (k >= K) return;      // (no barrier below: a thread works on its own column of the LDS arrays)
    const int M = ws.m[b];
    int* count = ws.counts + (long long)b * K + k;
    if (M < 4) {
        *count = -1;
        return;
    }
    // the draws: Floyd's algorithm, 4 distinct ranks below M
    unsigned h = mix(seed + 0x9e3779b9u);
    h = mix(h ^ (unsigned)*epoch);
    h = mix(h ^ (unsigned)b);
    int pick[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = M - 4 + j;
        int t = (int)(mix(h ^ (unsigned)(4 * k + j)) % (unsigned)(n + 1));
        bool taken = false;
#pragma unroll
        for (int i = 0; i < j; ++i) taken |= pick[i] == t;
        pick[j] = taken ? n : t;
    }
    const float* planes = ws.planes + (long long)b * 4 * N;
    float px[4], py[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x = planes[pick[j]], y = planes[N + pick[j]], xp = planes[2 * N + pick[j]], yp = planes[3 * N + pick[j]];
        px[j] = x, py[j] = y;
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
    float* model = ws.models + ((long long)b * K + k) * 9;
    bool good = solve_8x9(sys, perm, lane, model);
    // w on the sample's own points: strictly of one sign, or three of them are collinear or the map folds the plane.  (This thread
    // wrote the nine values it reads back.)
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
    *count = good ? 0 : -1;
}

// counts in: 0 a model, -1 degenerate; out: the inliers (0 for a degenerate hypothesis)
__global__ void __launch_bounds__(SCORE_WAVES* WAVE) hom_score_kernel(int N, int K, float t, Workspace ws) {
    const int b = blockIdx.y, lane = threadIdx.x % WAVE, k = blockIdx.x * SCORE_WAVES + threadIdx.x / WAVE;
    if (k >= K) return;
    int* count = ws.counts + (long long)b * K + k;
    const int M = ws.m[b];
    int inliers = 0;
    if (*count == 0) {      // (uniform over the wave)
        const float* model = ws.models + ((long long)b * K + k) * 9;
        float h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = model[i];
        const float* planes = ws.planes + (long long)b * 4 * N;
        for (int r0 = 0; r0 < M; r0 += WAVE) {
            const int r = r0 + lane;
            bool in = false;
            if (r < M) {
                float num, den, w;
                transfer(h, make_float4(planes[r], planes[N + r], planes[2 * N + r], planes[3 * N + r]), num, den, w);
                in = w > 0.f && num <= t * den;
            }
            inliers += __popcll(__ballot(in));
        }
    }
    if (lane == 0) *count = inliers;
}

__global__ void __launch_bounds__(BLOCK) hom_select_kernel(const float4* __restrict__ matches, unsigned char* __restrict__ valid, int N, int K, Frame fr,
                                                           float t, float s2, int min_inliers, int permille, int planar_permille, int cull,
                                                           float2* __restrict__ pos, long long* __restrict__ ids, int* __restrict__ age,
                                                           float* __restrict__ Hout, float* __restrict__ dist2, unsigned char* __restrict__ status,
                                                           int* __restrict__ inliers, int* __restrict__ candidates, unsigned char* __restrict__ ok_out,
                                                           unsigned char* __restrict__ planar_out, int* __restrict__ epoch, Workspace ws) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int bc, bk;
    best_hypothesis(ws.counts + (long long)b * K, K, bc, bk);
    const int M = ws.m[b];
    const bool ok = M >= 4 && bc >= min_inliers && 1000ll * bc >= (long long)permille * M;
    float h[9];
    const float* model = ws.models + ((long long)b * K + bk) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = ok ? model[i] : 0.f;
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
                float num, den, w;
                transfer(h, normalise(m, fr), num, den, w);
                const bool in = w > 0.f && num <= t * den;
                if (w > 0.f) d = __fdiv_rn(den > 0.f ? __fdiv_rn(num, den) : (in ? 0.f : __builtin_inff()), s2);
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
        planar_out[b] = ok && 1000ll * bc >= (long long)planar_permille * M;
        // pixel coordinates: T^-1 Hn T with T = [[s, 0, -cx s], [0, s, -cy s], [0, 0, 1]] (all zero without a verdict)
        float g[9];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            g[3 * i] = h[3 * i] * fr.s;
            g[3 * i + 1] = h[3 * i + 1] * fr.s;
            g[3 * i + 2] = h[3 * i + 2] - (g[3 * i] * fr.cx + g[3 * i + 1] * fr.cy);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Hout[b * 9 + j] = __fdiv_rn(g[j], fr.s) + fr.cx * g[6 + j];
            Hout[b * 9 + 3 + j] = __fdiv_rn(g[3 + j], fr.s) + fr.cy * g[6 + j];
            Hout[b * 9 + 6 + j] = g[6 + j];
        }
        if (b == 0) *epoch = *epoch + 1;      // (the hypotheses of this call read it in an earlier launch)
    }
}

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

extern "C" int ff_homography_ws(int B, int N, int K) {
    if (B <= 0 || B > MAX_BATCH || N < 1 || N > MAX_ROWS || K < 1 || K > MAX_HYP) return 0;
    return (int)ws_bytes(B, N, K);
}

extern "C" int ff_homography_ransac(const float* matches, unsigned char* valid, int B, int N, int H, int W, float threshold, int K, int min_inliers,
                                    int permille, int planar_permille, unsigned int seed, int* epoch, int cull, float* pos, long long* ids, int* age,
                                    float* Hout, float* dist2, unsigned char* status, int* inliers, int* candidates, unsigned char* ok,
                                    unsigned char* planar, void* ws, long long ws_size, void* stream) {
    FF_REQUIRE_RANSAC_SHAPE("ff_homography_ransac");
    FF_REQUIRE(H > 0 && W > 0 && H <= (1 << 24) && W <= (1 << 24), "ff_homography_ransac: H = %d, W = %d (1 .. 2^24: positions are fp32)", H, W);
    FF_REQUIRE(threshold >= 0.f && threshold < __builtin_inff(), "ff_homography_ransac: threshold = %g (>= 0 and finite, no NaN)", (double)threshold);
    FF_REQUIRE(min_inliers >= 1, "ff_homography_ransac: min_inliers = %d (at least 1: a degenerate hypothesis scores 0)", min_inliers);
    FF_REQUIRE(permille >= 0 && permille <= 1000, "ff_homography_ransac: permille = %d (0 .. 1000)", permille);
    FF_REQUIRE(planar_permille >= 0 && planar_permille <= 1000, "ff_homography_ransac: planar_permille = %d (0 .. 1000)", planar_permille);
    FF_REQUIRE(matches && valid && epoch && Hout && dist2 && status && inliers && candidates && ok && planar && ws, "ff_homography_ransac: null pointer");
    FF_REQUIRE((pos && ids && age) || (!pos && !ids && !age), "ff_homography_ransac: a track table is pos, ids and age: all three or none");
    FF_REQUIRE(((size_t)matches & 15) == 0 && ((size_t)pos & 7) == 0, "ff_homography_ransac: matches must be 16-byte aligned, pos 8-byte aligned");
    FF_REQUIRE(((size_t)ws & 15) == 0 && ws_size >= (long long)ws_bytes(B, N, K),
               "ff_homography_ransac: ws must be 16-byte aligned and hold %lld bytes, got %lld", (long long)ws_bytes(B, N, K), ws_size);
    const Frame fr = frame_of(H, W);
    const float t = (float)((double)threshold * (double)threshold * (double)fr.s * (double)fr.s), s2 = (float)((double)fr.s * (double)fr.s);
    const Workspace w = carve(ws, B, N, K);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const float4* m4 = reinterpret_cast<const float4*>(matches);
    epi_compact_kernel<<<B, BLOCK, 0, s>>>(m4, valid, N, fr, w);
    hom_hypotheses_kernel<<<dim3((K + WAVE - 1) / WAVE, B), WAVE, 0, s>>>(N, K, seed, epoch, w);
    hom_score_kernel<<<dim3((K + SCORE_WAVES - 1) / SCORE_WAVES, B), SCORE_WAVES * WAVE, 0, s>>>(N, K, t, w);
    hom_select_kernel<<<B, BLOCK, 0, s>>>(m4, valid, N, K, fr, t, s2, min_inliers, permille, planar_permille, cull, reinterpret_cast<float2*>(pos), ids,
                                          age, Hout, dist2, status, inliers, candidates, ok, planar, epoch, w);
    return ff::check_launch("ff_homography_ransac");
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
