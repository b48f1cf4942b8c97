// AlternateCorrBlock (FF_RAFT_Core/corr.py:63-91): CorrBlock.__call__ (corr.py:29-50) without the all-pairs pyramid.
//
// By linearity, level l of the pyramid at fmap2 position p is <fmap1[q], pool_l(fmap2)[p]> / sqrt(C), pool_l the l-fold 2x2
// average pooling (floor semantics, as avg_pool2d).  The 81 taps of a level share their integer corners' grid: each output
// is a bilinear blend of four values of the 10 x 10 grid of integer-position dot products around the query.  So:
//   ff_corr_alt_prepare  (once per forward) pooled levels 1-3 of fmap2 and the lookup's operand form of every level:
//                        fp16 split pairs (ff_pack_split_f16's row format) for the split precisions, plain fp32 rows for
//                        the exact-fp32 one (level 0 and fmap1 are then the feature maps themselves);
//   ff_corr_alt_lookup   (per iteration) one block per 8 x 4 tile of queries of one image.  Per level: the tap chains of the
//                        32 queries (corr_lookup_dma.hip's arithmetic: bit-identical taps), the union of their windows clipped
//                        to the plane, ONE dense GEMM  D[union position][query] = <f2_l[pos], f1[q]>  on the matrix pipe
//                        (three-term split-f16 32x32x16 MFMAs, or exact 32x32x2 fp32 ones), D through LDS, and every query
//                        blends its own 9 x 9 outputs from it (the lookup kernel's blend order).
// Routes are decided on the device, per (tile, level): when the union is larger than the LDS buffer (discontinuous flow,
// wild coordinates) the tile is split into its four rows of 8 queries, and a row whose union is still too large into
// single queries (a window of at most 10 x 10 positions) - every query has a route, and nothing waits for the host.
//
// Operand rows are 1 KB (256 fp32 or 256 split pairs) and addressed with 64-bit offsets from a base per level: no batch has
// to fit a 4 GB buffer resource.  The A operand (union positions) is read straight from L2 into registers (union rows are
// contiguous runs of NHWC rows), the B operand (the tile's 32 fmap1 rows) is staged once per tile in LDS.
#pragma clang fp contract(off)
#include <cstdint>
#include "split_mfma.h"
#include "corr_alt_taps.h"

namespace {


constexpr int CH = 256;               // feature channels
constexpr int ROWB = 1024;            // bytes of one operand row
constexpr int TQX = 8, TQY = 4, TQ = TQX * TQY;
constexpr int CAP = 320;              // union positions the D buffer holds (smooth flow: 221 / 168 / 132 / 121 at levels 0-3)
constexpr int F1_PITCH = ROWB + 16;   // LDS row pitch of the fmap1 tile: consecutive rows 4 banks apart
constexpr int D_PITCH = TQ + 1;       // floats per D row
constexpr int OFF_F1 = 0;
constexpr int OFF_D = OFF_F1 + TQ * F1_PITCH;
constexpr int OFF_TAB = OFF_D + CAP * D_PITCH * 4;             // [32 queries][x0 x9 | y0 x9 | wx x9 | wy x9]
constexpr int OFF_WIN = OFF_TAB + TQ * 36 * 4;                 // clipped windows: 32 single queries, 4 rows, the tile
constexpr int NWIN = TQ + 4 + 1;
constexpr int OFF_PLAN = OFF_WIN + NWIN * 16;                  // work items [count, then (first, G, X0, Y0, BW, BH) x 32]
constexpr int LDS_BYTES = OFF_PLAN + (1 + 6 * TQ) * 4;
static_assert(2 * LDS_BYTES <= 160 * 1024, "two blocks per CU");

struct AltArgs {
    const char* f1;           // [B*Q][1 KB] split pairs or fp32 fmap1
    const char* f2[4];        // level l: [B*h_l*w_l][1 KB]
    const float* coords;      // [B*Q][2] x, y
    float* out;
    int* taps;                // optional [B*Q][4][2][9]
    long long out_ld;
    int h[4], w[4];
    float nm1x[4], nm1y[4], r2x[4], r2y[4];
    int tiles_x, tiles_y;
    float scale;
};


// One 32-position x 32-query block of D: rows = union positions p0 .. p0 + 31 (row-major over the BW-wide window at X0, Y0),
// columns = queries first + (col % G) of the tile.
template <bool SPLIT>
__device__ __forceinline__ void d_block(const AltArgs& a, char* sm, int lv, long long img_row0, int p0, int npos, int first, int G,
                                        int X0, int Y0, int BW, int lane) {
    const int r = lane & 31, hh = lane >> 5;
    const int p = min(p0 + r, npos - 1);
    const int py = p / BW, px = p - py * BW;
    const char* arow = a.f2[lv] + (size_t)(img_row0 + (long long)(Y0 + py) * a.w[lv] + (X0 + px)) * ROWB;
    const char* brow = sm + OFF_F1 + (first + (r & (G - 1))) * F1_PITCH;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if (SPLIT) {
        // 32-channel chunk c: [x0: 32 halfs | x1: 32 halfs]; k-slice s of the chunk: halfs 16 s + 8 hh .. + 7 of either term
#pragma unroll
        for (int c = 0; c < CH / 32; ++c)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int off = c * 128 + s * 32 + hh * 16;
                const f16x8 a0 = *reinterpret_cast<const f16x8*>(arow + off);
                const f16x8 a1 = *reinterpret_cast<const f16x8*>(arow + off + 64);
                const f16x8 b0 = *reinterpret_cast<const f16x8*>(brow + off);
                const f16x8 b1 = *reinterpret_cast<const f16x8*>(brow + off + 64);
                ff::mfma32_terms<3, true>(acc, a0, a1, b0, b1);      // a0 b0, a0 b1, a1 b0 (corr_build.hip's order)
            }
    } else {
        // exact fp32: the half-wave hh sums channels 128 hh .. 128 hh + 127, one channel per MFMA step (the order of k is free)
        const float* af = reinterpret_cast<const float*>(arow) + hh * 128;
        const float* bf = reinterpret_cast<const float*>(brow) + hh * 128;
#pragma unroll 4
        for (int i = 0; i < 32; ++i) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(af + 4 * i);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bf + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
        }
    }
    float* D = reinterpret_cast<float*>(sm + OFF_D);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = 8 * (i >> 2) + 4 * hh + (i & 3);
        if (p0 + row < npos) D[(p0 + row) * D_PITCH + r] = acc[i] * a.scale;
    }
}

template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void alt_lookup_kernel(const AltArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntile = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / ntile, tile = blockIdx.x - b * ntile;
    const int gx0 = (tile % a.tiles_x) * TQX, gy0 = (tile / a.tiles_x) * TQY;
    const int h0 = a.h[0], w0 = a.w[0];
    auto qactive = [&](int t) { return gx0 + (t & 7) < w0 && gy0 + (t >> 3) < h0; };
    auto qindex = [&](int t) { return ((long long)b * h0 + gy0 + (t >> 3)) * w0 + gx0 + (t & 7); };

    // the tile's fmap1 rows -> LDS (queries outside the image: zero rows)
    for (int i = tid; i < TQ * (ROWB / 16); i += 256) {
        const int t = i >> 6, pc = i & 63;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qactive(t)) v = *reinterpret_cast<const f32x4*>(a.f1 + (size_t)qindex(t) * ROWB + pc * 16);
        *reinterpret_cast<f32x4*>(sm + OFF_F1 + t * F1_PITCH + pc * 16) = v;
    }
    int* tab = reinterpret_cast<int*>(sm + OFF_TAB);
    int* win = reinterpret_cast<int*>(sm + OFF_WIN);
    int* plan = reinterpret_cast<int*>(sm + OFF_PLAN);
    const float* D = reinterpret_cast<const float*>(sm + OFF_D);

    for (int lv = 0; lv < 4; ++lv) {
        const int hl = a.h[lv], wl = a.w[lv];
        const float inv = 1.f / (float)(1 << lv);
        // ---- taps of the 32 queries: entry j = axis * 9 + offset index
        for (int i = tid; i < TQ * 18; i += 256) {
            const int t = i / 18, j = i - t * 18, ax = j / 9, o = j - ax * 9;
            const bool act = qactive(t);
            const float c = act ? a.coords[qindex(t) * 2 + ax] : 0.f;
            int i0;
            float wgt;
            tap(c, inv, (float)(o - 4), ax ? a.nm1y[lv] : a.nm1x[lv], ax ? a.r2y[lv] : a.r2x[lv], i0, wgt);
            tab[t * 36 + j] = i0;
            tab[t * 36 + 18 + j] = __float_as_int(wgt);
            if (a.taps && act) a.taps[(qindex(t) * 4 + lv) * 18 + j] = i0;
        }
        __syncthreads();
        // ---- windows clipped to the plane (wave 0; lanes 32-63 mirror 0-31): single queries, rows of 8, the tile
        if (wave == 0) {
            const int t = lane & 31;
            const int* e = tab + t * 36;
            int x0 = max(clampi(e[0]), 0), x1 = min(clampi(e[8]) + 1, wl - 1);
            int y0 = max(clampi(e[9]), 0), y1 = min(clampi(e[17]) + 1, hl - 1);
            if (!qactive(t) || x0 > x1 || y0 > y1) x0 = y0 = BIG, x1 = y1 = -BIG;      // empty: the identity of the union
            auto put = [&](int slot) { *reinterpret_cast<int4*>(win + slot * 4) = make_int4(x0, y0, x1, y1); };
            if (lane < 32) put(t);
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) {
                x0 = min(x0, __shfl_xor(x0, m));
                y0 = min(y0, __shfl_xor(y0, m));
                x1 = max(x1, __shfl_xor(x1, m));
                y1 = max(y1, __shfl_xor(y1, m));
                if (m == 4 && lane < 32 && (t & 7) == 0) put(TQ + (t >> 3));
            }
            if (lane == 0) put(TQ + 4);
        }
        __syncthreads();
        // ---- work items: the tile, else its rows, else single queries
        if (tid == 0) {
            int n = 0;
            auto area = [&](int slot) {
                const int4 v = *reinterpret_cast<const int4*>(win + slot * 4);
                return v.x > v.z ? 0 : (v.z - v.x + 1) * (v.w - v.y + 1);
            };
            auto push = [&](int first, int G, int slot) {
                const int4 v = *reinterpret_cast<const int4*>(win + slot * 4);
                int bw = v.x > v.z ? 0 : v.z - v.x + 1, bh = v.x > v.z ? 0 : v.w - v.y + 1;
                // (a single query's clipped window is at most 10 x 10: its taps are consecutive wherever they fall inside a plane;
                // the clamp only keeps the D buffer in bounds)
                if (bw > CAP) bw = CAP;
                if (bw * bh > CAP) bh = CAP / max(bw, 1);
                int* it = plan + 1 + 6 * n++;
                it[0] = first, it[1] = G, it[2] = v.x, it[3] = v.y, it[4] = bw, it[5] = bh;
            };
            if (area(TQ + 4) <= CAP) {
                push(0, TQ, TQ + 4);
            } else {
                for (int g = 0; g < 4; ++g) {
                    if (area(TQ + g) <= CAP) push(8 * g, 8, TQ + g);
                    else
                        for (int t = 8 * g; t < 8 * g + 8; ++t) push(t, 1, t);
                }
            }
            plan[0] = n;
        }
        __syncthreads();
        const int nitems = plan[0];
        for (int itn = 0; itn < nitems; ++itn) {
            const int* it = plan + 1 + 6 * itn;
            const int first = it[0], G = it[1], X0 = it[2], Y0 = it[3], BW = it[4], BH = it[5];
            const int npos = BW * BH;
            const long long img_row0 = (long long)b * hl * wl;
            for (int p0 = wave * 32; p0 < npos; p0 += 128) d_block<SPLIT>(a, sm, lv, img_row0, p0, npos, first, G, X0, Y0, BW, lane);
            __syncthreads();
            // ---- blend: item i -> query first + i / 81, output k = a * 9 + b (a: x offset, b: y offset)
            for (int i = tid; i < G * 81; i += 256) {
                const int col = i / 81, k = i - col * 81, t = first + col;
                if (!qactive(t)) continue;
                const int ia = k / 9, ib = k - ia * 9;
                const int* e = tab + t * 36;
                const int xa = clampi(e[ia]), yb = clampi(e[9 + ib]);
                const float wx = __int_as_float(e[18 + ia]), wy = __int_as_float(e[27 + ib]);
                auto dv = [&](int y, int x) {
                    const int dx = x - X0, dy = y - Y0;
                    return ((unsigned)dx < (unsigned)BW && (unsigned)dy < (unsigned)BH) ? D[(dy * BW + dx) * D_PITCH + col] : 0.f;
                };
                const float v00 = dv(yb, xa), v01 = dv(yb, xa + 1), v10 = dv(yb + 1, xa), v11 = dv(yb + 1, xa + 1);
                // corr_lookup_dma.hip's blend: weights (1 - wx, wx) x (1 - wy, wy), products, sum left to right
                const float ex = __fsub_rn(1.f, wx), sy = __fsub_rn(1.f, wy);
                const float t00 = __fmul_rn(v00, __fmul_rn(ex, sy)), t01 = __fmul_rn(v01, __fmul_rn(wx, sy));
                const float t10 = __fmul_rn(v10, __fmul_rn(ex, wy)), t11 = __fmul_rn(v11, __fmul_rn(wx, wy));
                a.out[qindex(t) * a.out_ld + lv * 81 + k] = __fadd_rn(__fadd_rn(__fadd_rn(t00, t01), t10), t11);
            }
            __syncthreads();
        }
    }
}

// ---- prepare: one thread = 4 channels of one 8 x 8 block of level-0 positions (its 4 x 4 / 2 x 2 / 1 pooled cells) ----
struct PrepArgs {
    const float* f1;
    const float* f2;
    char* f1s;                // SPLIT: split fmap1 rows
    char* lvl[4];             // SPLIT: split rows of levels 0-3; fp32: levels 1-3 (level 0 is fmap2 itself)
    int B, h[4], w[4], nbx, nby;
};

template <bool SPLIT>
__device__ __forceinline__ void put_row(char* base, long long row, int g, f32x4 v) {
    if (SPLIT) {
        f16x4 x0, x1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sv = v[e] * ff::WSPLIT;        // ff_pack_split_f16's arithmetic
            x0[e] = (_Float16)sv;
            x1[e] = (_Float16)(sv - (float)x0[e]);
        }
        char* c = base + (size_t)row * ROWB + (g >> 3) * 128 + (g & 7) * 8;
        *reinterpret_cast<f16x4*>(c) = x0;
        *reinterpret_cast<f16x4*>(c + 64) = x1;
    } else {
        *reinterpret_cast<f32x4*>(base + (size_t)row * ROWB + g * 16) = v;
    }
}

__device__ __forceinline__ f32x4 pool4(f32x4 p, f32x4 q, f32x4 r, f32x4 s) { return (((p + q) + r) + s) * 0.25f; }

template <bool SPLIT>
__global__ __launch_bounds__(256) void alt_prepare_kernel(const PrepArgs a) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    const int g = (int)(i & 63);
    const long long blk = i >> 6;
    const long long nb = (long long)a.nbx * a.nby;
    if (blk >= nb * a.B) return;
    const int b = (int)(blk / nb), rem = (int)(blk - (long long)b * nb);
    const int by = rem / a.nbx, bx = rem - by * a.nbx;
    const int h0 = a.h[0], w0 = a.w[0];
    auto row = [&](int l, int y, int x) { return ((long long)b * a.h[l] + y) * a.w[l] + x; };
    auto ld2 = [&](int y, int x) { return *reinterpret_cast<const f32x4*>(a.f2 + row(0, y, x) * CH + g * 4); };
    if (SPLIT) {
        for (int yy = 0; yy < 8; ++yy)
            for (int xx = 0; xx < 8; ++xx) {
                const int y = 8 * by + yy, x = 8 * bx + xx;
                if (y < h0 && x < w0) {
                    put_row<true>(a.lvl[0], row(0, y, x), g, ld2(y, x));
                    put_row<true>(a.f1s, row(0, y, x), g, *reinterpret_cast<const f32x4*>(a.f1 + row(0, y, x) * CH + g * 4));
                }
            }
    }
    f32x4 p1[4][4];
#pragma unroll
    for (int y1 = 0; y1 < 4; ++y1)
#pragma unroll
        for (int x1 = 0; x1 < 4; ++x1) {
            const int Y = 4 * by + y1, X = 4 * bx + x1;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (Y < a.h[1] && X < a.w[1]) {
                v = pool4(ld2(2 * Y, 2 * X), ld2(2 * Y, 2 * X + 1), ld2(2 * Y + 1, 2 * X), ld2(2 * Y + 1, 2 * X + 1));
                put_row<SPLIT>(a.lvl[1], row(1, Y, X), g, v);
            }
            p1[y1][x1] = v;
        }
    f32x4 p2[2][2];
#pragma unroll
    for (int y2 = 0; y2 < 2; ++y2)
#pragma unroll
        for (int x2 = 0; x2 < 2; ++x2) {
            const int Y = 2 * by + y2, X = 2 * bx + x2;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (Y < a.h[2] && X < a.w[2]) {
                v = pool4(p1[2 * y2][2 * x2], p1[2 * y2][2 * x2 + 1], p1[2 * y2 + 1][2 * x2], p1[2 * y2 + 1][2 * x2 + 1]);
                put_row<SPLIT>(a.lvl[2], row(2, Y, X), g, v);
            }
            p2[y2][x2] = v;
        }
    if (by < a.h[3] && bx < a.w[3]) put_row<SPLIT>(a.lvl[3], row(3, by, bx), g, pool4(p2[0][0], p2[0][1], p2[1][0], p2[1][1]));
}

}  // namespace

extern "C" int ff_corr_alt_prepare(const float* fmap1, const float* fmap2, int B, int h0, int w0, int C, int split, void* f1_split,
                                   void* const* levels, void* stream) {
    FF_REQUIRE(fmap1 && fmap2 && levels, "ff_corr_alt_prepare: null pointer");
    FF_REQUIRE(C == CH, "ff_corr_alt_prepare: C = %d (the kernels are built for 256 feature channels)", C);
    FF_REQUIRE(B >= 1 && (h0 >> 3) >= 2 && (w0 >> 3) >= 2, "ff_corr_alt_prepare: plane %dx%d too small (level 3 must be at least 2x2)", h0, w0);
    FF_REQUIRE(ff::aligned16(fmap1) && ff::aligned16(fmap2), "ff_corr_alt_prepare: feature maps not 16-byte aligned");
    PrepArgs a;
    a.f1 = fmap1;
    a.f2 = fmap2;
    a.f1s = static_cast<char*>(f1_split);
    for (int l = 0; l < 4; ++l) {
        a.h[l] = h0 >> l;
        a.w[l] = w0 >> l;
        a.lvl[l] = static_cast<char*>(levels[l]);
        FF_REQUIRE(l == 0 && !split ? true : (levels[l] != nullptr && ff::aligned16(levels[l])), "ff_corr_alt_prepare: level %d null or misaligned", l);
    }
    FF_REQUIRE(!split || (f1_split && ff::aligned16(f1_split)), "ff_corr_alt_prepare: split fmap1 rows null or misaligned");
    a.B = B;
    a.nbx = (w0 + 7) / 8;
    a.nby = (h0 + 7) / 8;
    const long long threads = (long long)B * a.nbx * a.nby * 64;
    const long long blocks = (threads + 255) / 256;
    FF_REQUIRE(blocks < (1ll << 31), "ff_corr_alt_prepare: grid too large");
    hipEvent_t ev0, ev1;          // null unless ff_launch_timing_begin(FF_TIME_ALT_PREPARE) is in effect
    ff::launch_timing_events(FF_TIME_ALT_PREPARE, &ev0, &ev1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (split) hipExtLaunchKernelGGL(alt_prepare_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, ev0, ev1, 0, a);
    else hipExtLaunchKernelGGL(alt_prepare_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, ev0, ev1, 0, a);
    return ff::check_launch("ff_corr_alt_prepare");
}

extern "C" int ff_corr_alt_lookup(const void* f1, const void* const* levels, int split, const float* coords, int B, int h0, int w0,
                                  float* out, int out_ld, int* taps, void* stream) {
    FF_REQUIRE(f1 && levels && coords && out, "ff_corr_alt_lookup: null pointer");
    FF_REQUIRE(B >= 1 && (h0 >> 3) >= 2 && (w0 >> 3) >= 2, "ff_corr_alt_lookup: level 3 is %dx%d; the sampler divides by (n-1)", h0 >> 3, w0 >> 3);
    FF_REQUIRE(out_ld >= 324, "ff_corr_alt_lookup: out_ld %d < 324", out_ld);
    FF_REQUIRE(ff::aligned16(f1), "ff_corr_alt_lookup: fmap1 rows misaligned");
    AltArgs a;
    a.f1 = static_cast<const char*>(f1);
    for (int l = 0; l < 4; ++l) {
        FF_REQUIRE(levels[l] != nullptr && ff::aligned16(levels[l]), "ff_corr_alt_lookup: level %d null or misaligned", l);
        a.f2[l] = static_cast<const char*>(levels[l]);
        a.h[l] = h0 >> l;
        a.w[l] = w0 >> l;
        a.nm1x[l] = (float)(a.w[l] - 1);
        a.nm1y[l] = (float)(a.h[l] - 1);
        const volatile float rx = 1.0f / a.nm1x[l], ry = 1.0f / a.nm1y[l];      // correctly rounded reciprocals (IEEE division)
        a.r2x[l] = rx + rx;
        a.r2y[l] = ry + ry;
    }
    a.coords = coords;
    a.out = out;
    a.out_ld = out_ld;
    a.taps = taps;
    a.tiles_x = (w0 + TQX - 1) / TQX;
    a.tiles_y = (h0 + TQY - 1) / TQY;
    a.scale = split ? 1.f / sqrtf((float)CH) / (ff::WSPLIT * ff::WSPLIT) : 1.f / sqrtf((float)CH);
    const long long blocks = (long long)B * a.tiles_x * a.tiles_y;
    FF_REQUIRE(blocks < (1ll << 31), "ff_corr_alt_lookup: grid too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipEvent_t ev0, ev1;          // null unless ff_launch_timing_begin(FF_TIME_ALT_LOOKUP) is in effect
    ff::launch_timing_events(FF_TIME_ALT_LOOKUP, &ev0, &ev1);
    if (split) {
        FF_ALLOW_DYNAMIC_LDS((&alt_lookup_kernel<true>), LDS_BYTES);
        hipExtLaunchKernelGGL(alt_lookup_kernel<true>, dim3((unsigned)blocks), dim3(256), LDS_BYTES, s, ev0, ev1, 0, a);
    } else {
        FF_ALLOW_DYNAMIC_LDS((&alt_lookup_kernel<false>), LDS_BYTES);
        hipExtLaunchKernelGGL(alt_lookup_kernel<false>, dim3((unsigned)blocks), dim3(256), LDS_BYTES, s, ev0, ev1, 0, a);
    }
    return ff::check_launch("ff_corr_alt_lookup");
}
