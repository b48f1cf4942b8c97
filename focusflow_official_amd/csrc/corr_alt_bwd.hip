// Backward of the on-the-fly correlation (corr_alt.hip's lookup): for all lookups of one recorded pass, the gradients of
// fmap1 and fmap2 - what CorrBlock's backward (scatter into the pyramid, pooling chain, two volume contractions) gives,
// without any Q x Q tensor.
//
// Per (tile of 8 x 4 queries, level l), the forward computed D[pos][q] = <f2_l[pos], f1[q]> / 16 over the union of the
// tile's windows and blended each query's 81 outputs from four corners of D.  Its adjoint: every upstream value dcorr_t[q][k]
// is scattered through the same corners and weights (corr_alt_taps.h: the forward's taps bit for bit) into an LDS buffer
//     A[pos][q] = sum_t sum_k dcorr_t[q][l*81 + k] w_k(pos) / 16,
// and then two GEMMs on the matrix pipe (exact fp32 32x32x2 MFMAs):
//     d f1[q]     += sum_pos A[pos][q] f2_l[pos]   (K = union positions; the tile owns its queries: accumulated in registers over
//                                                   every level and lookup, stored once - no atomics)
//     d f2_l[pos] += sum_q   A[pos][q] f1[q]       (K = the tile's 32 queries; fp32 atomics into linear level planes, each
//                                                   wave-instruction two 128-B runs of two 1 KB rows, as the accumulator holds them)
// The scatter for lookup t goes into the SAME A as lookup t-1 while its work item's union lies inside the window A holds
// (windows are grown by one position on every side where the buffer has room), so the iterations of a converging flow share
// one pair of GEMMs and one set of atomics.  Routes are decided on the device exactly as in the forward: the tile's union, else
// its four rows of 8, else single queries.  A last kernel folds the level planes into d fmap2 = d f2_0 + sum_l unpool_l(d f2_l)
// / 4^l (avg_pool2d's floor semantics: rows and columns the pooling dropped get nothing).
//
// The arithmetic is exact fp32 in every precision (the operands are fp32 rows: fmap1, fmap2 and ff_corr_alt_prepare's fp32
// levels 1-3): the coefficients A are sums of products of upstream gradients and weights, whose split-f16 form would need a
// third split operand per pass; DESIGN.md §4 gives what the exact form costs.
#pragma clang fp contract(off)
#include <cstdint>
#include "split_mfma.h"
#include "corr_alt_taps.h"

namespace {


constexpr int CH = 256;               // feature channels
constexpr int TQX = 8, TQY = 4, TQ = TQX * TQY;
constexpr int CAP = 320;              // union positions the A buffer holds (as the forward's D buffer)
constexpr int F1_PITCH = CH + 4;      // floats per LDS row of the fmap1 tile: consecutive rows 4 banks apart
constexpr int A_PITCH = TQ + 1;       // floats per A row
constexpr int OFF_F1 = 0;
constexpr int OFF_A = OFF_F1 + TQ * F1_PITCH * 4;
constexpr int OFF_TAB = OFF_A + CAP * A_PITCH * 4;             // [32 queries][x0 x9 | y0 x9 | wx x9 | wy x9]
constexpr int OFF_WIN = OFF_TAB + TQ * 36 * 4;                 // clipped windows: 32 single queries, 4 rows, the tile
constexpr int NWIN = TQ + 4 + 1;
constexpr int OFF_PLAN = OFF_WIN + NWIN * 16;                  // work items [count, then (first, G, X0, Y0, BW, BH) x 32]
constexpr int LDS_BYTES = OFF_PLAN + (1 + 6 * TQ) * 4;
static_assert(2 * LDS_BYTES <= 160 * 1024, "two blocks per CU");
constexpr int MAXT = 32;              // lookups per launch (the host splits longer passes)

struct BwdArgs {
    const float* f1;          // fmap1 [B*Q][256]
    const float* f2[4];       // fp32 levels [B*h_l*w_l][256] (level 0 = fmap2)
    const float* coords[MAXT];
    const float* dout[MAXT];  // [B*Q][dout_ld], channels 0..323
    float* df1;               // [B*Q][256]
    float* df2[4];            // zeroed fp32 level planes [B*h_l*w_l][256]
    long long dout_ld;
    int nt, accumulate;       // accumulate: add into df1 (a later launch of a split pass)
    int h[4], w[4];
    float nm1x[4], nm1y[4], r2x[4], r2y[4];
    int tiles_x, tiles_y;
};

__global__ __launch_bounds__(256, 2) void alt_lookup_bwd_kernel(const BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int ntile = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / ntile, tile = blockIdx.x - b * ntile;
    const int gx0 = (tile % a.tiles_x) * TQX, gy0 = (tile / a.tiles_x) * TQY;
    const int h0 = a.h[0], w0 = a.w[0];
    auto qactive = [&](int t) { return gx0 + (t & 7) < w0 && gy0 + (t >> 3) < h0; };
    auto qindex = [&](int t) { return ((long long)b * h0 + gy0 + (t >> 3)) * w0 + gx0 + (t & 7); };

    float* F1 = reinterpret_cast<float*>(sm + OFF_F1);
    float* A = reinterpret_cast<float*>(sm + OFF_A);
    int* tab = reinterpret_cast<int*>(sm + OFF_TAB);
    int* win = reinterpret_cast<int*>(sm + OFF_WIN);
    int* plan = reinterpret_cast<int*>(sm + OFF_PLAN);

    // the tile's fmap1 rows -> LDS (queries outside the image: zero rows); A zeroed once (every flush zeroes what it used)
    for (int i = tid; i < TQ * (CH / 4); i += 256) {
        const int t = i >> 6, pc = i & 63;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qactive(t)) v = *reinterpret_cast<const f32x4*>(a.f1 + qindex(t) * CH + pc * 4);
        *reinterpret_cast<f32x4*>(F1 + t * F1_PITCH + pc * 4) = v;
    }
    for (int i = tid; i < CAP * A_PITCH; i += 256) A[i] = 0.f;

    // d fmap1 of the tile: rows = its 32 queries, columns = channels 64 wave .. 64 wave + 63 (two 32 x 32 accumulators)
    f32x16 g1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) g1[j][i] = 0.f;

    for (int lv = 0; lv < 4; ++lv) {
        const int hl = a.h[lv], wl = a.w[lv];
        const float inv = 1.f / (float)(1 << lv);
        const long long img_row0 = (long long)b * hl * wl;
        const float* f2 = a.f2[lv];

        // both GEMMs over the window (X0, Y0, BW, BH) that A holds, then A's rows back to zero
        auto flush = [&](int X0, int Y0, int BW, int BH) {
            const int npos = BW * BH;
            // d f2_l[pos][c] = sum_q A[pos][q] f1[q][c]: 32 positions x 32 channels per accumulator, K = the 32 queries
            for (int p0 = wave * 32; p0 < npos; p0 += 128) {
                float av[16];
#pragma unroll
                for (int s = 0; s < 16; ++s) av[s] = A[(p0 + r) * A_PITCH + 2 * s + hh];     // (rows >= npos are zero)
                long long orow[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int p = p0 + 8 * (i >> 2) + 4 * hh + (i & 3);
                    const int py = p / max(BW, 1), px = p - py * BW;
                    orow[i] = p < npos ? img_row0 + (long long)(Y0 + py) * wl + (X0 + px) : -1;
                }
                for (int cb = 0; cb < CH / 32; ++cb) {
                    f32x16 acc;
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                    for (int s = 0; s < 16; ++s)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], F1[(2 * s + hh) * F1_PITCH + cb * 32 + r], acc, 0, 0, 0);
                    float* dst = a.df2[lv] + cb * 32 + r;
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (orow[i] >= 0 && acc[i] != 0.f) atomicAdd(dst + orow[i] * CH, acc[i]);
                }
            }
            // d f1[q][c] += sum_pos A[pos][q] f2_l[pos][c]: K = the window's positions, two at a time
            const int c0 = wave * 64 + r;
            for (int s = 0; 2 * s < npos; ++s) {
                const int p = 2 * s + hh;                      // (p < CAP: A's row p is zero beyond npos)
                const float av = A[p * A_PITCH + r];
                const int pc = min(p, npos - 1);
                const int py = pc / BW, px = pc - py * BW;
                const float* row = f2 + (size_t)(img_row0 + (long long)(Y0 + py) * wl + (X0 + px)) * CH;
                g1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, row[c0], g1[0], 0, 0, 0);
                g1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, row[c0 + 32], g1[1], 0, 0, 0);
            }
            __syncthreads();
            for (int i = tid; i < npos * A_PITCH; i += 256) A[i] = 0.f;
            __syncthreads();
        };

        int cx0 = 0, cy0 = 0, cbw = 0, cbh = 0;        // the window A holds (cbw == 0: none)
        for (int t = 0; t < a.nt; ++t) {
            // ---- taps of the 32 queries for lookup t (the forward's): entry j = axis * 9 + offset index
            for (int i = tid; i < TQ * 18; i += 256) {
                const int q = i / 18, j = i - q * 18, ax = j / 9, o = j - ax * 9;
                const float c = qactive(q) ? a.coords[t][qindex(q) * 2 + ax] : 0.f;
                int i0;
                float wgt;
                tap(c, inv, (float)(o - 4), ax ? a.nm1y[lv] : a.nm1x[lv], ax ? a.r2y[lv] : a.r2x[lv], i0, wgt);
                tab[q * 36 + j] = i0;
                tab[q * 36 + 18 + j] = __float_as_int(wgt);
            }
            __syncthreads();
            // ---- windows clipped to the plane (the forward's): single queries, rows of 8, the tile
            if (wave == 0) {
                const int q = lane & 31;
                const int* e = tab + q * 36;
                int x0 = max(clampi(e[0]), 0), x1 = min(clampi(e[8]) + 1, wl - 1);
                int y0 = max(clampi(e[9]), 0), y1 = min(clampi(e[17]) + 1, hl - 1);
                if (!qactive(q) || x0 > x1 || y0 > y1) x0 = y0 = BIG, x1 = y1 = -BIG;
                auto put = [&](int slot) { *reinterpret_cast<int4*>(win + slot * 4) = make_int4(x0, y0, x1, y1); };
                if (lane < 32) put(q);
#pragma unroll
                for (int m = 1; m < 32; m <<= 1) {
                    x0 = min(x0, __shfl_xor(x0, m));
                    y0 = min(y0, __shfl_xor(y0, m));
                    x1 = max(x1, __shfl_xor(x1, m));
                    y1 = max(y1, __shfl_xor(y1, m));
                    if (m == 4 && lane < 32 && (q & 7) == 0) put(TQ + (q >> 3));
                }
                if (lane == 0) put(TQ + 4);
            }
            __syncthreads();
            // ---- work items (the forward's): the tile, else its rows, else single queries
            if (tid == 0) {
                int n = 0;
                auto area = [&](int slot) {
                    const int4 v = *reinterpret_cast<const int4*>(win + slot * 4);
                    return v.x > v.z ? 0 : (v.z - v.x + 1) * (v.w - v.y + 1);
                };
                auto push = [&](int first, int G, int slot) {
                    const int4 v = *reinterpret_cast<const int4*>(win + slot * 4);
                    int bw = v.x > v.z ? 0 : v.z - v.x + 1, bh = v.x > v.z ? 0 : v.w - v.y + 1;
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
                            for (int q = 8 * g; q < 8 * g + 8; ++q) push(q, 1, q);
                    }
                }
                plan[0] = n;
            }
            __syncthreads();
            const int nitems = plan[0];
            const float* dout = a.dout[t];
            for (int itn = 0; itn < nitems; ++itn) {
                const int* it = plan + 1 + 6 * itn;
                const int first = it[0], G = it[1], X0 = it[2], Y0 = it[3], BW = it[4], BH = it[5];
                if (BW * BH == 0) continue;                    // no corner of these queries lies inside the plane
                // the route of this item: scatter into the window A holds, or flush that and start a new one
                if (cbw == 0 || X0 < cx0 || Y0 < cy0 || X0 + BW > cx0 + cbw || Y0 + BH > cy0 + cbh) {
                    if (cbw != 0) flush(cx0, cy0, cbw, cbh);
                    int nx0 = max(X0 - 1, 0), ny0 = max(Y0 - 1, 0);
                    int nx1 = min(X0 + BW, wl - 1), ny1 = min(Y0 + BH, hl - 1);
                    if ((nx1 - nx0 + 1) * (ny1 - ny0 + 1) > CAP) nx0 = X0, ny0 = Y0, nx1 = X0 + BW - 1, ny1 = Y0 + BH - 1;
                    cx0 = nx0, cy0 = ny0, cbw = nx1 - nx0 + 1, cbh = ny1 - ny0 + 1;
                }
                // ---- scatter: item i -> query first + i / 81, output k = ia * 9 + ib (the forward's blend, transposed)
                for (int i = tid; i < G * 81; i += 256) {
                    const int col = i / 81, k = i - col * 81, q = first + col;
                    if (!qactive(q)) continue;
                    const float g = dout[qindex(q) * a.dout_ld + lv * 81 + k] * 0.0625f;     // (1 / sqrt(256): exact)
                    if (g == 0.f) continue;
                    const int ia = k / 9, ib = k - ia * 9;
                    const int* e = tab + q * 36;
                    const int xa = clampi(e[ia]), yb = clampi(e[9 + ib]);
                    const float wx = __int_as_float(e[18 + ia]), wy = __int_as_float(e[27 + ib]);
                    const float ex = __fsub_rn(1.f, wx), sy = __fsub_rn(1.f, wy);
                    auto add = [&](int y, int x, float v) {
                        if ((unsigned)(x - X0) < (unsigned)BW && (unsigned)(y - Y0) < (unsigned)BH)
                            atomicAdd(A + ((y - cy0) * cbw + (x - cx0)) * A_PITCH + q, v);
                    };
                    add(yb, xa, __fmul_rn(g, __fmul_rn(ex, sy)));
                    add(yb, xa + 1, __fmul_rn(g, __fmul_rn(wx, sy)));
                    add(yb + 1, xa, __fmul_rn(g, __fmul_rn(ex, wy)));
                    add(yb + 1, xa + 1, __fmul_rn(g, __fmul_rn(wx, wy)));
                }
                __syncthreads();
            }
        }
        if (cbw != 0) flush(cx0, cy0, cbw, cbh);
    }

    // ---- d fmap1: the tile owns its rows
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = 8 * (i >> 2) + 4 * hh + (i & 3);
            if (!qactive(q)) continue;
            float* dst = a.df1 + qindex(q) * CH + wave * 64 + 32 * j + r;
            *dst = a.accumulate ? *dst + g1[j][i] : g1[j][i];
        }
}

// ---- fold: d fmap2[pix] = d f2_0[pix] + sum_{l >= 1} d f2_l[pix >> l] / 4^l (in place on level 0); one thread = 4 channels
struct FoldArgs {
    float* d0;
    const float* dl[4];
    int B, h[4], w[4];
};

__global__ __launch_bounds__(256) void alt_fold_kernel(const FoldArgs a) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    const long long npix = (long long)a.B * a.h[0] * a.w[0];
    if (i >= npix * (CH / 4)) return;
    const long long pix = i >> 6;
    const int g = (int)(i & 63);
    const int x = (int)(pix % a.w[0]);
    const long long by = pix / a.w[0];
    const int y = (int)(by % a.h[0]), b = (int)(by / a.h[0]);
    f32x4 v = *reinterpret_cast<const f32x4*>(a.d0 + pix * CH + g * 4);
    float s = 0.25f;
#pragma unroll
    for (int l = 1; l < 4; ++l, s *= 0.25f) {
        const int yl = y >> l, xl = x >> l;
        if (yl < a.h[l] && xl < a.w[l]) v += *reinterpret_cast<const f32x4*>(a.dl[l] + (((long long)b * a.h[l] + yl) * a.w[l] + xl) * CH + g * 4) * s;
    }
    *reinterpret_cast<f32x4*>(a.d0 + pix * CH + g * 4) = v;
}

}  // namespace

extern "C" int ff_corr_alt_lookup_bwd(const float* fmap1, const float* const* levels, const float* const* coords_list,
                                      const float* const* dout_list, int T, int dout_ld, int B, int h0, int w0, float* d_fmap1,
                                      float* const* d_levels, void* stream) {
    FF_REQUIRE(fmap1 && levels && coords_list && dout_list && d_fmap1 && d_levels, "ff_corr_alt_lookup_bwd: null pointer");
    FF_REQUIRE(T >= 1, "ff_corr_alt_lookup_bwd: T = %d (no lookup has a gradient: the caller's gradients are zero)", T);
    FF_REQUIRE(B >= 1 && (h0 >> 3) >= 2 && (w0 >> 3) >= 2, "ff_corr_alt_lookup_bwd: level 3 is %dx%d; the sampler divides by (n-1)", h0 >> 3, w0 >> 3);
    FF_REQUIRE(dout_ld >= 324, "ff_corr_alt_lookup_bwd: dout_ld %d < 324", dout_ld);
    FF_REQUIRE(ff::aligned16(fmap1) && ff::aligned16(d_fmap1), "ff_corr_alt_lookup_bwd: fmap1 / d_fmap1 misaligned");
    for (int t = 0; t < T; ++t)
        FF_REQUIRE(coords_list[t] && dout_list[t], "ff_corr_alt_lookup_bwd: lookup %d: null coordinates or gradient", t);
    BwdArgs a;
    a.f1 = fmap1;
    a.df1 = d_fmap1;
    for (int l = 0; l < 4; ++l) {
        FF_REQUIRE(levels[l] && d_levels[l] && ff::aligned16(levels[l]) && ff::aligned16(d_levels[l]),
                   "ff_corr_alt_lookup_bwd: level %d null or misaligned", l);
        a.f2[l] = levels[l];
        a.df2[l] = d_levels[l];
        a.h[l] = h0 >> l;
        a.w[l] = w0 >> l;
        a.nm1x[l] = (float)(a.w[l] - 1);
        a.nm1y[l] = (float)(a.h[l] - 1);
        const volatile float rx = 1.0f / a.nm1x[l], ry = 1.0f / a.nm1y[l];      // ff_corr_alt_lookup's reciprocals
        a.r2x[l] = rx + rx;
        a.r2y[l] = ry + ry;
    }
    a.dout_ld = dout_ld;
    a.tiles_x = (w0 + TQX - 1) / TQX;
    a.tiles_y = (h0 + TQY - 1) / TQY;
    const long long blocks = (long long)B * a.tiles_x * a.tiles_y;
    FF_REQUIRE(blocks < (1ll << 31), "ff_corr_alt_lookup_bwd: grid too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    FF_ALLOW_DYNAMIC_LDS((&alt_lookup_bwd_kernel), LDS_BYTES);
    // passes longer than MAXT lookups: one launch per MAXT, the later ones adding into d_fmap1 (the level planes accumulate anyway)
    for (int t0 = 0; t0 < T; t0 += MAXT) {
        a.nt = T - t0 < MAXT ? T - t0 : MAXT;
        a.accumulate = t0 > 0;
        for (int t = 0; t < a.nt; ++t) {
            a.coords[t] = coords_list[t0 + t];
            a.dout[t] = dout_list[t0 + t];
        }
        hipEvent_t ev0, ev1;      // null unless ff_launch_timing_begin(FF_TIME_ALT_LOOKUP_BWD) is in effect
        ff::launch_timing_events(FF_TIME_ALT_LOOKUP_BWD, &ev0, &ev1);
        hipExtLaunchKernelGGL(alt_lookup_bwd_kernel, dim3((unsigned)blocks), dim3(256), LDS_BYTES, s, ev0, ev1, 0, a);
        const int rc = ff::check_launch("ff_corr_alt_lookup_bwd");
        if (rc != FF_OK) return rc;
    }
    FoldArgs f;
    f.d0 = d_levels[0];
    f.B = B;
    for (int l = 0; l < 4; ++l) {
        f.dl[l] = d_levels[l];
        f.h[l] = h0 >> l;
        f.w[l] = w0 >> l;
    }
    const long long fblocks = ((long long)B * h0 * w0 * (CH / 4) + 255) / 256;
    FF_REQUIRE(fblocks < (1ll << 31), "ff_corr_alt_lookup_bwd: fold grid too large");
    hipLaunchKernelGGL(alt_fold_kernel, dim3((unsigned)fblocks), dim3(256), 0, s, f);
    return ff::check_launch("ff_corr_alt_lookup_bwd (fold)");
}
