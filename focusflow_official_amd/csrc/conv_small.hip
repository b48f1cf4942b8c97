// Direct 3x3 convolution for 1 or 2 output channels (flow head conv2 256 -> 2, update.py:13-14; SA's 2 -> 1
// spatial map; FF-PWC's flow estimators): on a 64-wide MFMA tile such a conv wastes 97 % of the matrix work
// (41 us for 0.23 GFLOP at 48x64x8).  Two kernels, both exact fp32, chosen by ff::conv2d_fwd_small:
//
//   conv_small_kernel (the run kernel; inputs of fewer than 128 channels, and every shape under FF_SMALL_TILE=0): a dot
//   product on the vector ALU.  One wave = a run of RUN output pixels of one image row; lane = one group of 4 input
//   channels (Cin <= 256 per pass, more passes for wider inputs); the 3x3 weights of the lane's channels stay in registers
//   for the run; the input window slides along x, so each new pixel costs 3 coalesced float4 loads (1 KB per wave) instead
//   of 9; per pixel and output channel the 64 partial sums are folded with xor-shuffles.
//
//   conv_small_tile_kernel (the tile kernel; 128 channels or more): a block per 6 x 8 output tile reads the tile and its
//   halo once, forms per-input-pixel partial products on the fp32 MFMA and sums them over the 3x3 neighbourhood through
//   LDS - described at the kernel.  The flow head takes 12.9 us on it, 24.6 us on the run kernel (profiles/conv_small_trace.txt).
#include "ff_common.h"

namespace {

constexpr int RUN = 8;

struct SArgs {
    FFConvParams p;
    int Cin, runs_x;
};

__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b, float acc) {
    acc = fmaf(a[0], b[0], acc); acc = fmaf(a[1], b[1], acc); acc = fmaf(a[2], b[2], acc); return fmaf(a[3], b[3], acc);
}

// The epilogue of one output pixel (both kernels): bias, out_scale, ch_scale / ch_shift, act, res + act_res, the store, and
// the coordinate step of FF_EP_COORDS.  mine[] = the pixel's sums over all taps and channels.  The operands it reads from
// memory are loaded by load_ep, which the tile kernel calls ahead of its slab exchange (a load issued after the sums would
// add its whole latency to the block's critical path).
template <int COUT>
struct EpOps {
    float bias[COUT], res[COUT], c1[2];
};

template <int COUT>
__device__ __forceinline__ EpOps<COUT> load_ep(const FFConvParams& p, int b, int y, int x) {
    const long long m = ((long long)b * p.H + y) * p.W + x;
    EpOps<COUT> e;
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
        e.bias[c] = p.bias ? p.bias[c] : 0.f;
        e.res[c] = p.res ? p.res[m * p.res_ld + c] : 0.f;
    }
    e.c1[0] = e.c1[1] = 0.f;
    if constexpr (COUT == 2) {
        if (p.ep_mode == FF_EP_COORDS) { e.c1[0] = p.ep_a[m * 2]; e.c1[1] = p.ep_a[m * 2 + 1]; }
    }
    return e;
}

template <int COUT>
__device__ __forceinline__ void finish_pixel(const FFConvParams& p, int b, int y, int x, float (&mine)[COUT], const EpOps<COUT>& e) {
    const long long m = ((long long)b * p.H + y) * p.W + x;
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
        float v = mine[c] + e.bias[c];
        v *= p.out_scale;
        if (p.ch_scale) v = v * p.ch_scale[c] + p.ch_shift[c];
        v = ff::apply_act(v, p.act);
        if (p.res) v = ff::apply_act(v + e.res[c], p.act_res);
        p.y[m * p.y_ld + c] = v;
        mine[c] = v;
    }
    if constexpr (COUT == 2) {
        if (p.ep_mode == FF_EP_COORDS) {      // raft.py:223 coords1 = coords1 + delta_flow, :219 flow = coords1 - coords0 (ff_coords_step's roundings)
            float* c1 = const_cast<float*>(p.ep_a) + m * 2;
            const float cx = __fadd_rn(e.c1[0], mine[0]), cy = __fadd_rn(e.c1[1], mine[1]);
            c1[0] = cx;
            c1[1] = cy;
            *reinterpret_cast<f32x4*>(const_cast<float*>(p.ep_b) + m * 4) = (f32x4){__fsub_rn(cx, (float)x), __fsub_rn(cy, (float)y), 0.f, 0.f};
        }
    }
}

template <int COUT>
__global__ __launch_bounds__(256) void conv_small_kernel(const SArgs a) {
    const FFConvParams& p = a.p;
    const int lane = threadIdx.x & 63;
    const long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // (b, y, run)
    const long long ntask = (long long)p.B * p.H * a.runs_x;
    if (task >= ntask) return;
    const int run = (int)(task % a.runs_x);
    const int y = (int)((task / a.runs_x) % p.H);
    const int b = (int)(task / ((long long)a.runs_x * p.H));
    const int x0 = run * RUN;
    const int H = p.H, W = p.W, K = 9 * a.Cin;

    float mine[COUT];                        // lane i (< RUN) collects pixel x0 + i
#pragma unroll
    for (int c = 0; c < COUT; ++c) mine[c] = 0.f;

    // channel passes: lane's 4 channels at cpos = pass*256 + lane*4 of the concatenated input
    for (int cbase = 0; cbase < a.Cin; cbase += 256) {
        const int cpos = cbase + lane * 4;
        const bool cok = cpos < a.Cin;
        // which segment holds cpos (segments are multiples of 4 channels, so a float4 never straddles two)
        const float* xp = p.x[0];            // lanes past the last channel load a valid dummy (segment 0, channel 0)
        int ld = p.x_ld[0], cs = 0;
        if (cok) {
            const int c0 = p.x_c[0], c01 = p.x_c[0] + p.x_c[1];
            cs = cpos;
            if (cs < c0) { xp = p.x[0]; ld = p.x_ld[0]; }
            else if (cs < c01) { xp = p.x[1]; ld = p.x_ld[1]; cs -= c0; }
            else { xp = p.x[2]; ld = p.x_ld[2]; cs -= c01; }
        }
        f32x4 w[COUT][9];
#pragma unroll
        for (int c = 0; c < COUT; ++c)
#pragma unroll
            for (int t = 0; t < 9; ++t)
                w[c][t] = cok ? *reinterpret_cast<const f32x4*>(p.w + (long long)c * K + t * a.Cin + cpos) : (f32x4){0.f, 0.f, 0.f, 0.f};
        // no load under a branch (the compiler would wait for each before issuing the next): out-of-image taps read a
        // clamped pixel and are zeroed by a select
        auto load = [&](int yy, int xx) {
            const bool ok = cok && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const int yc = min(max(yy, 0), H - 1), xc = min(max(xx, 0), W - 1);
            const f32x4 v = *reinterpret_cast<const f32x4*>(xp + ((long long)(b * H + yc) * W + xc) * ld + cs);
            return ok ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
        };
        f32x4 col[3][3];                     // col[slot][dy]: window columns x-1, x, x+1 rotate through 3 slots
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) { col[0][dy] = load(y - 1 + dy, x0 - 1); col[1][dy] = load(y - 1 + dy, x0); }
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) col[(i + 2) % 3][dy] = load(y - 1 + dy, x0 + i + 1);
#pragma unroll
            for (int c = 0; c < COUT; ++c) {
                float s = 0.f;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) s = dot4(col[(i + dx) % 3][dy], w[c][dy * 3 + dx], s);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);      // fold the 64 lanes right away
                if (lane == i) mine[c] += s;
            }
        }
    }
    const int x = x0 + lane;
    if (lane < RUN && x < W) finish_pixel<COUT>(p, b, y, x, mine, load_ep<COUT>(p, b, y, x));
}

// ---- the tile kernel (conv_small_tile_kernel): the same convolution for inputs of 128 channels or more.
// A block owns TH x TW = 6 x 8 output pixels and reads their (TH + 2) x (TW + 2) = 80 input pixels once (1.67 x the tile,
// the shared halo out of one L2; the run kernel above reads every pixel 3.75 times).  For every input pixel q it forms
//     P[q][n] = sum_ch x[q][ch] * w[n][ch],   n = cout * 9 + tap   (9 or 18 columns; the packed rows ARE w[n][Cin])
// and an output pixel is the sum of its nine P[q + tap][cout * 9 + tap].  P is a [80 x Cin] x [Cin x 18] product in exact
// fp32: columns 0 .. 15 on v_mfma_f32_16x16x4_f32 (an fmaf chain, one rounding per product - the arithmetic class of the
// run kernel - and the sum over the channels needs no fold across lanes), columns 16 and 17 of the two-channel head as
// fmaf chains on the vector ALU beside the MFMAs (a second MFMA for 2 of 16 columns would double the matrix time).  The 80
// pixels are 5 groups of 16 (the A rows: lane = pixel l & 15, k = l >> 4; the B columns: lane = n, k = l >> 4).  A lane's
// k are 4 consecutive channels (one float4 load -> 4 MFMAs), so one load instruction reads 64 consecutive bytes of each
// of 16 pixels.  The four waves split the channels: a pass is 256 channels, wave w takes 64 of them (4 float4 per pixel
// and lane, 256 consecutive bytes per pixel); its weights (4 float4, and 8 for columns 16 / 17) stay in registers for the
// pass: loaded once per block and pass.  All loads of a pass are issued before its first MFMA.  Each wave writes its P
// slab to LDS; after one barrier a thread per output pixel sums 9 taps x 4 slabs in a fixed order (taps outside the image
// are left out: the zero padding) and runs the epilogue.  An in-image NaN / Inf reaches exactly the outputs that see it.
// The flow head (8 x 48 x 64, 256 channels) is 512 blocks, two per CU (196 VGPRs, 25 KB of LDS): while one block waits for
// its loads the other computes.  6 x 16 tiles - one block per CU, 1.5 x reads - measured 13.8 us there against 12.9 us.
constexpr int TH = 6, TW = 8, HALO_W = TW + 2, NPIX = (TH + 2) * HALO_W, NGRP = NPIX / 16, SLAB_LD = 20;
static_assert(NPIX % 16 == 0, "the halo tile is whole groups of 16 pixels");

struct TArgs {
    FFConvParams p;
    int Cin, tiles_x, tiles_y;
};

template <int COUT>
__global__ __launch_bounds__(256) void conv_small_tile_kernel(const TArgs a) {
    __shared__ float slab[4][NPIX][SLAB_LD];
    constexpr int NCOL = COUT == 2 ? 16 : 9, NEXT = COUT == 2 ? 2 : 0;      // columns on the MFMA, columns on the vector ALU
    const FFConvParams& p = a.p;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pi = lane & 15, kq = lane >> 4;
    // Blocks i, i + 8, i + 16 ... are observed to share an XCD and its L2: give each of the 8 classes a contiguous range of
    // tiles (the flow head: one image per class), so that the halo two neighbouring tiles share is fetched into one L2
    // once.  A bijection for every grid size; placement changes the speed only.
    const int nblk = gridDim.x, q8 = nblk / 8, r8 = nblk % 8, cls = blockIdx.x % 8;
    const int tile = (cls < r8 ? cls * (q8 + 1) : r8 * (q8 + 1) + (cls - r8) * q8) + blockIdx.x / 8;
    const int tx = tile % a.tiles_x, ty = (tile / a.tiles_x) % a.tiles_y, b = tile / (a.tiles_x * a.tiles_y);
    const int y0 = ty * TH, x0 = tx * TW, H = p.H, W = p.W, Cin = a.Cin;

    int pix[NGRP];                           // the lane's input pixel of each group, clamped into the image (< 2^30)
#pragma unroll
    for (int g = 0; g < NGRP; ++g) {
        const int q = g * 16 + pi, iy = y0 - 1 + q / HALO_W, ix = x0 - 1 + q % HALO_W;
        pix[g] = (b * H + min(max(iy, 0), H - 1)) * W + min(max(ix, 0), W - 1);
    }
    f32x4 acc[NGRP];                         // P[pixel g * 16 + kq * 4 + r][column pi] in acc[g][r]
    float ext[NGRP][NEXT > 0 ? NEXT : 1];    // this lane's 4-channel share of P[pixel g * 16 + pi][column 16 + e]
#pragma unroll
    for (int g = 0; g < NGRP; ++g) {
        acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < NEXT; ++e) ext[g][e] = 0.f;
    }

    // No value that comes from a load passes through a select (the compiler turns such a select into a branch around the
    // load and waits for each load by itself): a pixel outside the image reads a clamped one and its P is never summed;
    // a column past the last reads the last one and is never stored; a lane whose channels lie past Cin reads the first
    // four weights as its "activations" (finite wherever the result is) against weights multiplied by 0.
    const int c0 = p.x_c[0], c01 = p.x_c[0] + p.x_c[1];
    for (int cbase = wv * 64; cbase < Cin; cbase += 256) {      // this wave's 64 channels of each pass (wave-uniform)
        const float* xp[4];
        long long ld[4];
        f32x4 bw[4], wx[4][NEXT > 0 ? NEXT : 1];
        float keep[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cpos = cbase + j * 16 + kq * 4;
            const bool cok = cpos < Cin;
            // which segment holds cpos (segments are multiples of 4 channels, so a float4 never straddles two)
            const int seg = cpos < c0 ? 0 : (cpos < c01 ? 1 : 2);
            const int cs = cpos - (seg == 0 ? 0 : (seg == 1 ? c0 : c01));
            xp[j] = cok ? (seg == 0 ? p.x[0] : (seg == 1 ? p.x[1] : p.x[2])) + cs : p.w;
            ld[j] = cok ? (seg == 0 ? p.x_ld[0] : (seg == 1 ? p.x_ld[1] : p.x_ld[2])) : 0;
            keep[j] = cok ? 1.f : 0.f;
            const float* wc = p.w + (cok ? cpos : 0);
            bw[j] = *reinterpret_cast<const f32x4*>(wc + (long long)min(pi, NCOL - 1) * Cin);
#pragma unroll
            for (int e = 0; e < NEXT; ++e) wx[j][e] = *reinterpret_cast<const f32x4*>(wc + (long long)(16 + e) * Cin);
        }
        f32x4 xa[NGRP][4];
#pragma unroll
        for (int g = 0; g < NGRP; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) xa[g][j] = *reinterpret_cast<const f32x4*>(xp[j] + pix[g] * ld[j]);
        // every load first, then the groups in the order their loads return: the scheduler would otherwise interleave all
        // groups (independent accumulators) and wait for the last load before the first MFMA.  Two groups at a time, so
        // that no MFMA waits for the one before it (issue 32 cycles, dependent 40).
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bw[j] *= keep[j];
#pragma unroll
            for (int e = 0; e < NEXT; ++e) wx[j][e] *= keep[j];
        }
#pragma unroll
        for (int g0 = 0; g0 < NGRP; g0 += 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int g = g0; g < g0 + 2 && g < NGRP; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[g][j][t], bw[j][t], acc[g], 0, 0, 0);
#pragma unroll
                for (int g = g0; g < g0 + 2 && g < NGRP; ++g)
#pragma unroll
                    for (int e = 0; e < NEXT; ++e) ext[g][e] = dot4(xa[g][j], wx[j][e], ext[g][e]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the thread's output pixel in the epilogue; what the epilogue reads from memory is asked for now, ahead of the slab
    // writes, the barrier and the LDS sums
    const int oy = threadIdx.x / TW, ox = threadIdx.x % TW, y = y0 + oy, x = x0 + ox;
    const bool has_px = oy < TH && y < H && x < W;
    EpOps<COUT> eo = {};
    if (has_px) eo = load_ep<COUT>(p, b, y, x);
#pragma unroll
    for (int g = 0; g < NGRP; ++g) {
        if (pi < NCOL) {
#pragma unroll
            for (int r = 0; r < 4; ++r) slab[wv][g * 16 + kq * 4 + r][pi] = acc[g][r];
        }
#pragma unroll
        for (int e = 0; e < NEXT; ++e) {     // the four lanes of a pixel (kq = 0 .. 3) hold its four channel shares
            float s = ext[g][e];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (kq == 0) slab[wv][g * 16 + pi][16 + e] = s;
        }
    }
    __syncthreads();
    if (has_px) {
        float mine[COUT];
#pragma unroll
        for (int c = 0; c < COUT; ++c) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const bool in = (unsigned)(y - 1 + t / 3) < (unsigned)H && (unsigned)(x - 1 + t % 3) < (unsigned)W;      // zero padding
#pragma unroll
                for (int w4 = 0; w4 < 4; ++w4) {
                    const float v = slab[w4][(oy + t / 3) * HALO_W + ox + t % 3][c * 9 + t];
                    s += in ? v : 0.f;
                }
            }
            mine[c] = s;
        }
        finish_pixel<COUT>(p, b, y, x, mine, eo);
    }
}

}  // namespace

namespace ff {
// FF_OK if launched, 1 if the shape is not this kernel's (fp32 rows, 3x3, stride 1, pad 1, Cout <= 2, groups 1)
int conv2d_fwd_small(const FFConvParams& p, int cin, hipStream_t s) {
    const int dlh = p.dil_h ? p.dil_h : 1, dlw = p.dil_w ? p.dil_w : 1;
    if (p.w_format != FF_W_F32 || p.Cout > 2 || p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad_h != 1 || p.pad_w != 1 ||
        dlh != 1 || dlw != 1 || p.groups != 1)
        return 1;
    // The tile kernel takes every input of 128 channels or more (any segments, any ld, any multiple of 4 channels; a last
    // pass of fewer than 256 channels runs with zeros): the flow head, FF-PWC's densely connected flow estimators.
    // Narrower inputs - SA's 2 -> 1 map - would leave most of its four waves without channels and keep the run kernel.
    // FF_SMALL_TILE=0: A/B switch, the run kernel for every shape.
    static const bool tile_enabled = !(getenv("FF_SMALL_TILE") && atoi(getenv("FF_SMALL_TILE")) == 0);
    if (tile_enabled && cin >= 128) {
        TArgs t;
        t.p = p;
        t.Cin = cin;
        t.tiles_x = (p.W + TW - 1) / TW;
        t.tiles_y = (p.H + TH - 1) / TH;
        const unsigned blocks = (unsigned)((long long)p.B * t.tiles_y * t.tiles_x);       // < 2^30 pixels (ff_conv2d_fwd)
        if (p.Cout == 1) conv_small_tile_kernel<1><<<blocks, 256, 0, s>>>(t);
        else conv_small_tile_kernel<2><<<blocks, 256, 0, s>>>(t);
        return check_launch("ff_conv2d_fwd(small, tile)");
    }
    SArgs a;
    a.p = p;
    a.Cin = cin;
    a.runs_x = (p.W + RUN - 1) / RUN;
    const long long tasks = (long long)p.B * p.H * a.runs_x;
    const unsigned blocks = (unsigned)((tasks + 3) / 4);
    if (p.Cout == 1) conv_small_kernel<1><<<blocks, 256, 0, s>>>(a);
    else conv_small_kernel<2><<<blocks, 256, 0, s>>>(a);
    return check_launch("ff_conv2d_fwd(small)");
}
}  // namespace ff

// ---------------------------------------------------------------------------------------------------------------------
// nn.ConvTranspose2d(Cin, Cout <= 2, kernel 4, stride 2, padding 1) - FF-PWC's netUpflow / netUpfeat
// (ff_pwcnet.py:243-244) - without the zero-dilated copy of the input and without a matrix tile: on the MFMA path the
// 640 -> 2 layer at 56 x 128 took 257 us (a 4x larger, three-quarters-zero input and 62 of 64 tile columns empty).
// Written as the equivalent forward convolution over the dilated input D (D[2i][2j] = x[i][j], 4 x 4 kernel Wf = the
// flipped, transposed parameter, pad 2): out[oy][ox] = sum_{a,b} D[oy-2+a][ox-2+b] Wf[a][b]; D is non-zero only at even
// coordinates, so an output pixel sees 2 x 2 taps: a = oy mod 2 (+2), input row (oy - 2 + a) / 2, likewise in x.
// One wave = a run of 8 output pixels of one output row (6 input columns x 2 input rows); lane = 4 input channels
// (256 channels per pass); the 2 x 4 taps of the row parity stay in registers; exact fp32.
namespace {

struct DArgs {
    const float* x; int x_ld;
    const float* w;          // [Cout][16 * Cin] fp32 rows, k = (a * 4 + b) * Cin + ci  (ff_pack_conv_weight of Wf)
    const float* bias;
    float* y; int y_ld;
    int B, H, W, Cin, runs_x;
};

template <int COUT>
__global__ __launch_bounds__(256) void deconv4x4s2_small_kernel(const DArgs a) {
    const int lane = threadIdx.x & 63;
    const int Ho = 2 * a.H, Wo = 2 * a.W;
    const long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // (b, oy, run)
    if (task >= (long long)a.B * Ho * a.runs_x) return;
    const int run = (int)(task % a.runs_x);
    const int oy = (int)((task / a.runs_x) % Ho);
    const int b = (int)(task / ((long long)a.runs_x * Ho));
    const int ox0 = run * RUN, n0 = ox0 >> 1;               // RUN = 8 outputs = input columns n0 - 1 .. n0 + 4
    const int a0 = oy & 1;                                   // kernel rows a0, a0 + 2 -> input rows iy0, iy0 + 1
    const int iy0 = (oy - 2 + a0) >> 1;                      // arithmetic shift: -1 for oy = 0
    const int K = 16 * a.Cin;

    float mine[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) mine[c] = 0.f;
    for (int cbase = 0; cbase < a.Cin; cbase += 256) {
        const int cpos = cbase + lane * 4;
        const bool cok = cpos < a.Cin;
        f32x4 w[COUT][2][4];                                  // [co][row tap a0 + 2 r][b]
#pragma unroll
        for (int c = 0; c < COUT; ++c)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int bb = 0; bb < 4; ++bb)
                    w[c][r][bb] = cok ? *reinterpret_cast<const f32x4*>(a.w + (long long)c * K + ((a0 + 2 * r) * 4 + bb) * a.Cin + cpos)
                                      : (f32x4){0.f, 0.f, 0.f, 0.f};
        auto load = [&](int iy, int ix) {                     // no load under a branch: clamp, then select
            const bool ok = cok && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const int yc = min(max(iy, 0), a.H - 1), xc = min(max(ix, 0), a.W - 1);
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + ((long long)(b * a.H + yc) * a.W + xc) * a.x_ld + (cok ? cpos : 0));
            return ok ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
        };
        f32x4 col[6][2];                                       // input columns n0 - 1 + j, rows iy0 + r
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int r = 0; r < 2; ++r) col[j][r] = load(iy0 + r, n0 - 1 + j);
#pragma unroll
        for (int i = 0; i < RUN; ++i) {                       // ox = ox0 + i: b0 = i & 1, input columns (ox - 2 + b0) / 2 (+1)
            const int b0 = i & 1, j0 = ((i - 2 + b0) >> 1) + 1;   // column slot of the first tap: (ox - 2 + b0) / 2 - (n0 - 1)
#pragma unroll
            for (int c = 0; c < COUT; ++c) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int t = 0; t < 2; ++t) s = dot4(col[j0 + t][r], w[c][r][b0 + 2 * t], s);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if (lane == i) mine[c] += s;
            }
        }
    }
    const int ox = ox0 + lane;
    if (lane < RUN && ox < Wo) {
        const long long m = ((long long)b * Ho + oy) * Wo + ox;
#pragma unroll
        for (int c = 0; c < COUT; ++c) a.y[m * a.y_ld + c] = mine[c] + (a.bias ? a.bias[c] : 0.f);
    }
}

}  // namespace

extern "C" int ff_deconv4x4s2_small(const float* x, int x_ld, int B, int H, int W, int Cin, const float* w, const float* bias,
                                    int Cout, float* y, int y_ld, void* stream) {
    FF_REQUIRE(x && w && y && B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 4 == 0 && (Cout == 1 || Cout == 2),
               "ff_deconv4x4s2_small: Cin must be a multiple of 4, Cout 1 or 2");
    FF_REQUIRE(x_ld >= Cin && x_ld % 4 == 0 && y_ld >= Cout && ff::aligned16(x) && ff::aligned16(w), "ff_deconv4x4s2_small: ld/alignment");
    DArgs a;
    a.x = x; a.x_ld = x_ld; a.w = w; a.bias = bias; a.y = y; a.y_ld = y_ld;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin;
    a.runs_x = (2 * W + RUN - 1) / RUN;
    const long long tasks = (long long)B * 2 * H * a.runs_x;
    const unsigned blocks = (unsigned)((tasks + 3) / 4);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Cout == 1) deconv4x4s2_small_kernel<1><<<blocks, 256, 0, s>>>(a);
    else deconv4x4s2_small_kernel<2><<<blocks, 256, 0, s>>>(a);
    return ff::check_launch("ff_deconv4x4s2_small");
}
