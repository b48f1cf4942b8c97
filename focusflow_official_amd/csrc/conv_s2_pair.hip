// The entry of a stride-2 residual block as ONE launch (extractor.py:26-46, stages 2 and 3 of every encoder branch): from one
// fp32 NHWC input x
//     A = conv3x3(x), stride 2, pad 1        (conv1)
//     D = conv1x1(x), stride 2, pad 0        (downsample[0]: the shortcut)
// in(2y, 2x) is tap (1, 1) of the 3x3: the shortcut is one more tap step over rows the block already holds.  The generic route
// ran the two as im2col launches that each read x, re-split every activation once per tap and could not deliver InstanceNorm
// statistics (two ff_norm_stats passes re-read both outputs).
//   * a block owns a 4 x 16 output tile of one image and EVERY output channel of both convolutions, so the 9 x 33 input patch
//     is staged once per 32-channel chunk: 16-byte buffer loads (the descriptor zero-fills the padding and the ragged edges:
//     positions outside the image are given an offset beyond the tensor), split to (x0, x1) in registers, written to LDS once;
//   * LDS image: one row per patch position, 144-byte pitch, [x0 | x1 | pad]; the columns of a patch row de-interleaved (17
//     even ones, then 16 odd ones), so the 16 pixels of an output row read 16 consecutive LDS rows for every tap.  Conflict-free
//     ds_read_b128 in conv_patch.hip's way: the 16-byte k-groups of a term sit in the order 0, 2, 1, 3 and lane i handles pixel
//     PI16(i) of its row;
//   * Cout / 16 waves (6 or 8); a wave computes its 16 channels for all 64 pixels of both outputs (8 accumulator tiles) and takes
//     its weights straight into registers in fragment order (ff_pack_frag16, as conv_dma.hip's main loop): no weights in LDS,
//     the next tap's loads in flight behind the current tap's MFMAs;
//   * ten tap steps per chunk: nine into A's accumulators, the centre tap's rows again with the shortcut's weights into D's;
//     v_mfma_f32_16x16x32_f16 with A = weights, B = 16 pixels, terms in ff::mfma16_terms' order (split_mfma.h: w0 x0, w1 x0, w0 x1);
//   * a lane's accumulator holds four consecutive channels of one pixel: the epilogue - acc / 64 + bias, optional per-channel
//     scale and shift (folded eval BatchNorm), activation, as separately rounded operations - leaves as 16-byte buffer stores;
//   * statistics (optional per output): every lane reduces what it stores to {pivot, sum(v - pivot), sum((v - pivot)^2), n} per
//     channel, the 16 lanes of a channel group merge re-centred on one pivot (conv_patch.hip's merge), one entry per tile:
//     [B][tiles][Cout][4] for ff_norm_stats_finish.
// hipcc-flags: -ffp-contract=off
#include <algorithm>
#include "split_mfma.h"

namespace {

constexpr int TH = 4, TW = 16;                  // output tile
constexpr int PH = 2 * TH + 1, PW = 2 * TW + 1; // input patch: 9 x 33
constexpr int NEV = TW + 1;                     // even patch columns come first in a row of the LDS image
constexpr int NPOS = PH * PW;
constexpr int PITCH = 144;
constexpr int LDS_BYTES = NPOS * PITCH;         // 42768: three 6-wave blocks (96 registers) or two 8-wave blocks per CU
constexpr unsigned OOB = 0x80000000u;           // every tensor is below 2 GiB: an offset no descriptor covers

struct SArgs {
    FFConvS2Pair p;
    int Ho, Wo, tiles_x, tiles_y, ncin;         // ncin = Cin / 32
    unsigned x_bytes, y_bytes[2];               // what the descriptors cover
};

template <int TERMS, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(NW == 8 ? 4 : 5, NW == 8 ? 4 : 5))) void conv_s2_pair_kernel(const SArgs a) {
    constexpr int NT = NW * 64, NITEM = NPOS * 8, NJ = (NITEM + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    const FFConvS2Pair& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, g16 = lane >> 4;
    const int tx = blockIdx.x, ty = blockIdx.y, b = blockIdx.z;
    const int ox0 = tx * TW, oy0 = ty * TH, ix0 = 2 * ox0 - 1, iy0 = 2 * oy0 - 1;
    const int H = p.H, W = p.W, ncin = a.ncin;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, a.x_bytes, 0x00020000);

    // ---- the loader's items: (patch position, 16-byte piece of its 32-channel chunk) in the order of the memory
    unsigned goff[NJ];
    int loff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = tid + j * NT, pos = i >> 3, q = i & 7;
        const int r = pos / PW, c = pos - r * PW;
        const int iy = iy0 + r, ix = ix0 + c;
        const bool ok = i < NITEM && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        goff[j] = ok ? ((unsigned)((b * H + iy) * W + ix) * (unsigned)p.x_ld) * 4u + q * 16 : OOB;
        const int idx = (c & 1) ? NEV + (c >> 1) : (c >> 1);
        loff[j] = (r * PW + idx) * PITCH + ff::KG16(q >> 1) * 16 + (q & 1) * 8;
    }

    // ---- this wave's weights: [Cout / 16][K chunks][term][lane][16 B]; the 3x3 rows are [tap][Cin]
    const __amdgpu_buffer_rsrc_t rwa = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w3_frag), 0, NW * 9 * ncin * 2048, 0x00020000);
    const __amdgpu_buffer_rsrc_t rwd = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w1_frag), 0, NW * ncin * 2048, 0x00020000);
    const int wbase_a = lane * 16 + wave * 9 * ncin * 2048, wbase_d = lane * 16 + wave * ncin * 2048;

    f32x4 acc_a[TH], acc_d[TH];
#pragma unroll
    for (int py = 0; py < TH; ++py) acc_a[py] = acc_d[py] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int pxl = ff::PI16(i16);
    const char* bp = smem + pxl * PITCH + ff::KG16(g16) * 16;

    auto load_w = [&](const __amdgpu_buffer_rsrc_t r, int off, f32x4 (&wv)[2]) { ff::load_w_frag<TERMS>(r, off, 0, wv); };
    auto tap_step = [&](const char* xp, const f32x4 (&wv)[2], f32x4 (&acc)[TH]) {      // one tap of one chunk over the tile's four rows
        // (ff::mfma16_terms' order written out: this kernel reads the x1 fragment BETWEEN the first term and the other two, which
        // the shared step - all operands before the first MFMA - schedules differently)
        const f16x8 w0 = __builtin_bit_cast(f16x8, wv[0]);
        f16x8 w1;
        if (TERMS == 3) w1 = __builtin_bit_cast(f16x8, wv[1]);
#pragma unroll
        for (int py = 0; py < TH; ++py) {
            const f16x8 xa = *reinterpret_cast<const f16x8*>(xp + py * (2 * PW * PITCH));
            acc[py] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, xa, acc[py], 0, 0, 0);
            if (TERMS == 3) {
                const f16x8 xb = *reinterpret_cast<const f16x8*>(xp + py * (2 * PW * PITCH) + 64);
                acc[py] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, xa, acc[py], 0, 0, 0);
                acc[py] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, xb, acc[py], 0, 0, 0);
            }
            if (py == 1) __builtin_amdgcn_sched_barrier(0);     // at most two rows' operands live at a time
        }
    };
    auto tap_off = [](int s) {                            // tap s = (ky, kx): patch row ky, de-interleaved column of kx
        const int ky = (s * 11) >> 5, kx = s - 3 * ky;
        return (ky * PW + (kx == 0 ? 0 : (kx == 1 ? NEV : 1))) * PITCH;
    };

    for (int kc = 0; kc < ncin; ++kc) {
        f32x4 wc[2], wn[2];
        {
            f32x4 val[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) val[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, goff[j] + kc * 128, 0, 0));
            load_w(rwa, wbase_a + kc * 2048, wc);
            if (kc) __syncthreads();                      // everybody has read the previous chunk
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j == NJ - 1 && tid + j * NT >= NITEM) continue;
                f16x4 h0, h1;
                ff::split_pair4(val[j], h0, h1);
                *reinterpret_cast<f16x4*>(smem + loff[j]) = h0;
                if (TERMS == 3) *reinterpret_cast<f16x4*>(smem + loff[j] + 64) = h1;
            }
        }
        __syncthreads();
        // ten steps, the next step's weights in flight behind the current step's MFMAs
#pragma unroll 1
        for (int s = 0; s < 8; ++s) {
            load_w(rwa, wbase_a + ((s + 1) * ncin + kc) * 2048, wn);
            tap_step(bp + tap_off(s), wc, acc_a);
            wc[0] = wn[0];
            wc[1] = wn[1];
        }
        load_w(rwd, wbase_d + kc * 2048, wn);
        tap_step(bp + tap_off(8), wc, acc_a);
        tap_step(bp + tap_off(4), wn, acc_d);             // the shortcut: the centre tap's rows again
    }

    // ---- epilogue: lane (i16, g16) holds channels 16 wave + 4 g16 .. + 3 of pixel (oy0 + py, ox0 + PI16(i16))
    const int Cout = NW * 16, ch = wave * 16 + g16 * 4;
    const int ox = ox0 + pxl;
    const int nparts = a.tiles_x * a.tiles_y, part = ty * a.tiles_x + tx;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.y[o], 0, a.y_bytes[o], 0x00020000);
        const f32x4 bias = p.bias[o] ? *reinterpret_cast<const f32x4*>(p.bias[o] + ch) : (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 cs = {1.f, 1.f, 1.f, 1.f}, ct = {0.f, 0.f, 0.f, 0.f};
        if (p.scale[o]) {
            cs = *reinterpret_cast<const f32x4*>(p.scale[o] + ch);
            ct = *reinterpret_cast<const f32x4*>(p.shift[o] + ch);
        }
        f32x4 out[TH];
        bool ok[TH];
#pragma unroll
        for (int py = 0; py < TH; ++py) {
            f32x4 v = (o == 0 ? acc_a[py] : acc_d[py]) * ff::SPLIT_INV + bias;
            if (p.scale[o]) v = v * cs + ct;
            if (p.act[o] == FF_ACT_RELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] < 0.f ? 0.f : v[r];      // (torch.relu: a NaN stays a NaN, ff::apply_act)
            }
            out[py] = v;
            const int oy = oy0 + py;
            ok[py] = oy < a.Ho && ox < a.Wo;
            const unsigned yoff = ok[py] ? ((unsigned)((b * a.Ho + oy) * a.Wo + ox) * (unsigned)p.y_ld[o] + ch) * 4u : OOB;      // (a pixel outside the plane: dropped by the descriptor)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ry, yoff, 0, 0);
        }
        if (p.stats_part[o]) {
            // entry [image][tile][channel]: a wave's four lanes with i16 == 0 write 256 contiguous bytes
            f32x4* e = reinterpret_cast<f32x4*>(p.stats_part[o]) + ((long long)b * nparts + part) * Cout + ch;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float st_p = 0.f, st_s1 = 0.f, st_s2 = 0.f, st_n = 0.f;
#pragma unroll
                for (int py = 0; py < TH; ++py) {
                    if (!ok[py]) continue;
                    if (st_n == 0.f) st_p = out[py][r];                       // the pivot: the lane's first value inside the plane
                    const float d = out[py][r] - st_p;
                    st_s1 += d;
                    st_s2 = fmaf(d, d, st_s2);
                    st_n += 1.f;
                }
                // the other lanes of the 16 hold the same channel over other pixels: folded in re-centred on this lane's pivot
                //   sum(v - p) = s + n d,  sum((v - p)^2) = q + 2 d s + n d^2   for entries around p + d
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {
                    const float p2 = __shfl_xor(st_p, m), s2 = __shfl_xor(st_s1, m), q2 = __shfl_xor(st_s2, m), n2 = __shfl_xor(st_n, m);
                    const float pv = st_n > 0.f ? st_p : p2, d = p2 - pv;
                    st_s1 = st_s1 + s2 + n2 * d;
                    st_s2 = st_s2 + q2 + 2.f * d * s2 + n2 * d * d;
                    st_n += n2;
                    st_p = pv;
                }
                if (i16 == 0) e[r] = (f32x4){st_p, st_s1, st_s2, st_n};
            }
        }
    }
}

bool overlap(const void* a, long long na, const void* b, long long nb) {
    const char *x = static_cast<const char*>(a), *y = static_cast<const char*>(b);
    return x < y + nb && y < x + na;
}

template <int TERMS>
void launch(const SArgs& a, hipStream_t s) {
    const dim3 grid(a.tiles_x, a.tiles_y, a.p.B);
    if (a.p.Cout == 96) conv_s2_pair_kernel<TERMS, 6><<<grid, 384, 0, s>>>(a);
    else conv_s2_pair_kernel<TERMS, 8><<<grid, 512, 0, s>>>(a);
}

}  // namespace

// statistics entries per (image, channel) of an H x W input: one per 4 x 16 output tile
extern "C" int ff_conv_s2_pair_stats_parts(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    return ((Ho + TH - 1) / TH) * ((Wo + TW - 1) / TW);
}

extern "C" int ff_conv_s2_pair_fwd(const FFConvS2Pair* pp, void* stream) {
    FF_REQUIRE(pp, "ff_conv_s2_pair_fwd: null argument");
    const FFConvS2Pair& p = *pp;
    FF_REQUIRE(p.k[0] == 3 && p.stride[0] == 2 && p.pad[0] == 1 && p.k[1] == 1 && p.stride[1] == 2 && p.pad[1] == 0,
               "ff_conv_s2_pair_fwd: kernel / stride / pad (%d, %d, %d) + (%d, %d, %d): this entry runs a 3x3 stride-2 pad-1 convolution with a 1x1 stride-2 pad-0 shortcut",
               p.k[0], p.stride[0], p.pad[0], p.k[1], p.stride[1], p.pad[1]);
    FF_REQUIRE(p.w_format == FF_W_F16X3 || p.w_format == FF_W_F16, "ff_conv_s2_pair_fwd: w_format %d (a split weight format; fp32 rows take ff_conv2d_fwd)", p.w_format);
    FF_REQUIRE(p.B > 0 && p.B < 65536 && p.H > 0 && p.W > 0, "ff_conv_s2_pair_fwd: B %d, H %d, W %d", p.B, p.H, p.W);
    FF_REQUIRE(p.Cin > 0 && p.Cin % 32 == 0, "ff_conv_s2_pair_fwd: Cin = %d (a multiple of 32)", p.Cin);
    FF_REQUIRE(p.Cout == 96 || p.Cout == 128, "ff_conv_s2_pair_fwd: Cout = %d (96 or 128; other widths take ff_conv2d_fwd)", p.Cout);
    FF_REQUIRE(p.x && p.w3_frag && p.w1_frag && ff::aligned16(p.w3_frag) && ff::aligned16(p.w1_frag), "ff_conv_s2_pair_fwd: null input / weights, or weights not 16-byte aligned");
    FF_REQUIRE(p.x_ld >= p.Cin && p.x_ld % 4 == 0 && ff::aligned16(p.x), "ff_conv_s2_pair_fwd: input: leading dimension %d (>= Cin, a multiple of 4) / 16-byte alignment", p.x_ld);
    SArgs a;
    a.p = p;
    a.Ho = (p.H - 1) / 2 + 1;
    a.Wo = (p.W - 1) / 2 + 1;
    a.tiles_x = (a.Wo + TW - 1) / TW;
    a.tiles_y = (a.Ho + TH - 1) / TH;
    a.ncin = p.Cin / 32;
    FF_REQUIRE(a.tiles_y < 65536, "ff_conv_s2_pair_fwd: H %d", p.H);
    const long long xb = (((long long)p.B * p.H * p.W - 1) * p.x_ld + p.Cin) * 4;
    FF_REQUIRE(xb < (1ll << 31), "ff_conv_s2_pair_fwd: a tensor of 2 GiB or more");
    a.x_bytes = (unsigned)xb;
    long long yb[2];
    for (int o = 0; o < 2; ++o) {
        FF_REQUIRE(p.y[o] && p.y_ld[o] >= p.Cout && p.y_ld[o] % 4 == 0 && ff::aligned16(p.y[o]),
                   "ff_conv_s2_pair_fwd: output %d: null, leading dimension %d (>= Cout, a multiple of 4) or not 16-byte aligned", o, p.y_ld[o]);
        yb[o] = (((long long)p.B * a.Ho * a.Wo - 1) * p.y_ld[o] + p.Cout) * 4;
        FF_REQUIRE(yb[o] < (1ll << 31), "ff_conv_s2_pair_fwd: a tensor of 2 GiB or more");
        a.y_bytes[o] = (unsigned)yb[o];
        FF_REQUIRE(!overlap(p.y[o], yb[o], p.x, xb), "ff_conv_s2_pair_fwd: output %d aliases the input", o);
        FF_REQUIRE(p.act[o] == FF_ACT_NONE || p.act[o] == FF_ACT_RELU, "ff_conv_s2_pair_fwd: act %d (FF_ACT_NONE or FF_ACT_RELU)", p.act[o]);
        FF_REQUIRE(!p.bias[o] || ff::aligned16(p.bias[o]), "ff_conv_s2_pair_fwd: bias %d not 16-byte aligned", o);
        FF_REQUIRE(!p.scale[o] || (p.shift[o] && ff::aligned16(p.scale[o]) && ff::aligned16(p.shift[o])), "ff_conv_s2_pair_fwd: scale without shift / alignment (output %d)", o);
        FF_REQUIRE(!p.stats_part[o] || ff::aligned16(p.stats_part[o]), "ff_conv_s2_pair_fwd: stats_part %d not 16-byte aligned", o);
    }
    FF_REQUIRE(!overlap(p.y[0], yb[0], p.y[1], yb[1]), "ff_conv_s2_pair_fwd: the two outputs alias");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.w_format == FF_W_F16X3) launch<3>(a, s);
    else launch<1>(a, s);
    return ff::check_launch("ff_conv_s2_pair_fwd");
}
