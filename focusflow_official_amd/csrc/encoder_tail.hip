// The output stage of a Condition Control Encoder as ONE launch (parallel_fusion.py:237-242): behind stage 3 both encoders end in
//     m4 = m + B4 x + b4 ,  x4 = x + A4 m + a4          fusion4   (128 channels, both directions)
//     m5 = Wm m4 + bm    ,  x5 = Wx x4 + bx             mask_conv2 / conv2   (128 -> 256)
//     out = x5 + A5 m5 + a5                              fusion5   (256 channels, one direction)
// with no activation and no norm in between, i.e. out = W [x | m] + b: one 1x1 convolution 256 -> 256 whose weight the host
// composes from the ten parameters (cce.py: float64, rounded once).  The generic route ran it as four conv_split launches at
// 1/8 resolution that write and re-read three intermediate tensors; here every input byte is read once and only the result is
// written.
//   * a block owns one tile of 64 consecutive pixels of the flat [B HW] pixel axis; 256 threads load their (pixel, 4 channel)
//     items of both tensors with 16-byte buffer loads (the descriptor's size bounds a partial last tile: reads beyond it return
//     zero, stores are dropped) and write the split pair (x0, x1) to LDS once - the operand image [8 K chunks][64 pixels][128 B];
//   * LAZY INPUTS as in fusion_pair.hip: with scale / shift tables (ff_norm_coeffs) and the residual given, the loader evaluates
//     relu(xres + relu(fma(x, scale, shift))) itself - ff_norm_apply's operations, bit for bit - so the feature encoder's two
//     normalisation passes behind stage 3 disappear.  A tile may straddle images (HW % 64 != 0): the tables are then indexed per
//     item;
//   * wave w computes output channels 64 w .. 64 w + 63 (four 16-channel tiles) for all 64 pixels: 64 accumulator registers.
//     The composed weight (256 KB in fragment order, ff_pack_frag16; L2-resident) comes chunk by chunk straight into registers,
//     the next chunk's loads in flight behind the current chunk's MFMAs (32 registers per buffer);
//   * matrix form and LDS image are conv_dma.hip's / fusion_pair.hip's: v_mfma_f32_16x16x32_f16, A = weights, B = 16 pixels, LDS
//     row = one pixel's 32-channel chunk [x0 | x1], its eight 16-byte slots XOR-swizzled by (pixel >> 1) & 7, lanes mapped to pixels
//     through PI16.  Terms in ff::mfma16_terms' order (split_mfma.h: w0 x0, w1 x0, w0 x1), K in ascending chunks;
//   * a lane's accumulator holds four consecutive output channels of one pixel: the epilogue - acc / 64 + bias as separately
//     rounded operations - leaves as 16-byte stores straight from the registers (a wave's four stores fill 256 consecutive bytes
//     of each of its 16 pixels).
// hipcc-flags: -ffp-contract=off
#include <algorithm>
#include "split_mfma.h"

namespace {

constexpr int C = 128;      // channels per input branch
constexpr int COUT = 256;
constexpr int TP = 64;      // pixels per tile
constexpr int NKC = 2 * C / 32;     // K chunks of 32 channels over the segments [x | m]
constexpr int PLANE = TP * 128;     // one K chunk of the operand image
constexpr int LDS_BYTES = NKC * PLANE;

struct TArgs {
    FFEncoderTail p;
    unsigned npix;          // B * HW
};

template <int TERMS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void encoder_tail_kernel(const TArgs a) {
    constexpr int G = C / 4;            // 4-channel groups per pixel and branch: 32
    constexpr int PSTEP = 256 / G;      // pixels per pass of the loader: 8
    constexpr int NI = TP / PSTEP;      // items per thread and tensor: 8
    constexpr int NPG = TP / 16;        // 16-pixel groups of a tile
    constexpr int NTW = COUT / 16 / 4;  // 16-channel output tiles per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FFEncoderTail& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, g16 = lane >> 4;
    const int grp = tid % G, pl = tid / G;
    const unsigned pix0 = blockIdx.x * (unsigned)TP;
    const unsigned in_bytes = a.npix * (unsigned)(C * 4), out_bytes = a.npix * (unsigned)(COUT * 4);     // < 2^31 (checked by the host)

    // ---- this wave's weights: chunk 0 is on its way while the tile is loaded
    const int tile0 = wave * NTW;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w_frag), 0, (COUT / 16) * NKC * 2048, 0x00020000);
    f32x4 wa[NTW][2], wb[NTW][2];
    auto load_w = [&](int kc, f32x4 (&w)[NTW][2]) {          // [COUT / 16][NKC][term][lane][16 B]
#pragma unroll
        for (int v = 0; v < NTW; ++v) {       // (not ff::load_w_frag: with the offset as one shared value the compiler groups lane * 16 + 1024 differently - other address code)
            w[v][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, lane * 16 + ((tile0 + v) * NKC + kc) * 2048, 0, 0));
            if (TERMS == 3) w[v][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, lane * 16 + ((tile0 + v) * NKC + kc) * 2048 + 1024, 0, 0));
        }
    };
    load_w(0, wa);

    // ---- load phase: one branch's items (and a lazy branch's residuals) in flight together; the value the stage reads is x, or
    // in_act(fma(x, scale, shift)), or relu(xres + that) (ff_norm_apply's operations); its split pair goes to the operand image
    const bool one_image = p.HW % TP == 0;          // a tile lies inside one image: one pair of coefficient vectors per thread
    const unsigned voff = pix0 * (unsigned)(C * 4) + tid * 16;
#pragma unroll
    for (int br = 0; br < 2; ++br) {
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x[br]), 0, in_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.xres[br] ? p.xres[br] : p.x[br]), 0, in_bytes, 0x00020000);
        f32x4 val[NI], rsd[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            val[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, voff + j * (256 * 16), 0, 0));
            if (p.xres[br]) rsd[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, voff + j * (256 * 16), 0, 0));
        }
        if (p.scale[br]) {
            f32x4 sc, sh;
            if (one_image) {
                const int bimg = (int)(pix0 / (unsigned)p.HW);
                sc = *reinterpret_cast<const f32x4*>(p.scale[br] + (long long)bimg * C + grp * 4);
                sh = *reinterpret_cast<const f32x4*>(p.shift[br] + (long long)bimg * C + grp * 4);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                if (!one_image) {
                    const int bimg = min((int)((pix0 + j * PSTEP + pl) / (unsigned)p.HW), p.B - 1);     // (pixels beyond the last image: any table row; their results are not stored)
                    sc = *reinterpret_cast<const f32x4*>(p.scale[br] + (long long)bimg * C + grp * 4);
                    sh = *reinterpret_cast<const f32x4*>(p.shift[br] + (long long)bimg * C + grp * 4);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float o = fmaf(val[j][r], sc[r], sh[r]);
                    o = ff::apply_act(o, p.in_act);
                    if (p.xres[br]) { o += rsd[j][r]; o = o < 0.f ? 0.f : o; }
                    val[j][r] = o;
                }
            }
        }
        // operand image: row = pixel, K chunk br * 4 + grp / 8, slot swizzle by (pixel >> 1) & 7
        const int cc = (grp * 4) & 31, kcw = br * (C / 32) + ((grp * 4) >> 5);
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            f16x4 h0, h1;
            ff::split_pair4(val[j], h0, h1);
            const int px = j * PSTEP + pl, sw = (px >> 1) & 7;
            char* row = smem + kcw * PLANE + px * 128 + (cc & 7) * 2;
            *reinterpret_cast<f16x4*>(row + (((cc >> 3) ^ sw) << 4)) = h0;
            if (TERMS == 3) *reinterpret_cast<f16x4*>(row + (((4 + (cc >> 3)) ^ sw) << 4)) = h1;
        }
    }
    __syncthreads();

    // ---- the 256 x 256 convolution: this wave's NTW channel tiles over all pixel groups
    f32x4 acc[NTW][NPG];
#pragma unroll
    for (int v = 0; v < NTW; ++v)
#pragma unroll
        for (int g = 0; g < NPG; ++g) acc[v][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int pxl = ff::PI16(i16), swl = (pxl >> 1) & 7;             // ((16 g + pxl) >> 1) & 7 == (pxl >> 1) & 7
    const char* fa = smem + pxl * 128 + ((g16 ^ swl) << 4);
    const char* fb = smem + pxl * 128 + (((4 + g16) ^ swl) << 4);
    auto chunk = [&](int kc, const f32x4 (&w)[NTW][2]) {
#pragma unroll
        for (int g = 0; g < NPG; ++g) {
            const f16x8 xa = *reinterpret_cast<const f16x8*>(fa + kc * PLANE + g * 2048);
            const f16x8 xb = TERMS == 3 ? *reinterpret_cast<const f16x8*>(fb + kc * PLANE + g * 2048) : xa;
#pragma unroll
            for (int v = 0; v < NTW; ++v) ff::mfma16_terms<TERMS>(acc[v][g], w[v][0], w[v][1], xa, xb);
        }
    };
#pragma unroll
    for (int kc = 0; kc < NKC; kc += 2) {
        load_w(kc + 1, wb);
        chunk(kc, wa);
        if (kc + 2 < NKC) load_w(kc + 2, wa);
        chunk(kc + 1, wb);
    }

    // ---- out = acc / 64 + bias: lane (i16, g16) holds channels 16 (tile0 + v) + 4 g16 .. + 3 of pixel 16 g + PI16(i16)
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, out_bytes, 0x00020000);
    const float xinv = ff::SPLIT_INV;
    const unsigned yoff = (pix0 + pxl) * (unsigned)(COUT * 4) + (tile0 * 16 + g16 * 4) * 4;
#pragma unroll
    for (int v = 0; v < NTW; ++v) {
        const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + (tile0 + v) * 16 + g16 * 4);
#pragma unroll
        for (int g = 0; g < NPG; ++g) {
            const f32x4 t = acc[v][g] * xinv + bias;
            // (vector offset only, as in fusion_pair.hip: no scalar offset register, and a pixel beyond the tensor is dropped by the descriptor)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t), ry, yoff + g * (16 * COUT * 4) + v * 64, 0, 0);
        }
    }
}

}  // namespace

extern "C" int ff_encoder_tail_fwd(const FFEncoderTail* pp, void* stream) {
    FF_REQUIRE(pp, "ff_encoder_tail_fwd: null argument");
    const FFEncoderTail& p = *pp;
    FF_REQUIRE(p.C == C && p.Cout == COUT, "ff_encoder_tail_fwd: C = %d, Cout = %d (the stage is 128 + 128 -> 256 channels; other widths take ff_conv2d_fwd)", p.C, p.Cout);
    FF_REQUIRE(p.B > 0 && p.HW > 0, "ff_encoder_tail_fwd: B %d, HW %d", p.B, p.HW);
    FF_REQUIRE((long long)p.B * p.HW * COUT * 4 < (1ll << 31), "ff_encoder_tail_fwd: a tensor of 2 GiB or more");
    FF_REQUIRE(p.w_format == FF_W_F16X3 || p.w_format == FF_W_F16, "ff_encoder_tail_fwd: w_format %d (a split weight format)", p.w_format);
    FF_REQUIRE(p.in_act >= FF_ACT_NONE && p.in_act <= FF_ACT_TANH, "ff_encoder_tail_fwd: bad in_act %d", p.in_act);
    FF_REQUIRE(p.y && p.w_frag && p.bias && p.y_ld == COUT && ff::aligned16(p.y) && ff::aligned16(p.w_frag) && ff::aligned16(p.bias),
               "ff_encoder_tail_fwd: output / weights / bias: null, not contiguous NHWC (leading dimension == 256) or not 16-byte aligned");
    for (int i = 0; i < 2; ++i) {
        FF_REQUIRE(p.x[i], "ff_encoder_tail_fwd: null tensor (branch %d)", i);
        FF_REQUIRE(p.x_ld[i] == C && ff::aligned16(p.x[i]), "ff_encoder_tail_fwd: contiguous NHWC inputs (leading dimension == 128) / 16-byte alignment (branch %d)", i);
        FF_REQUIRE(!p.xres[i] || (p.scale[i] && p.xres_ld[i] == C && ff::aligned16(p.xres[i])),
                   "ff_encoder_tail_fwd: xres needs scale / shift, leading dimension == 128, 16-byte alignment (branch %d)", i);
        FF_REQUIRE(!p.scale[i] || (p.shift[i] && ff::aligned16(p.scale[i]) && ff::aligned16(p.shift[i])), "ff_encoder_tail_fwd: scale without shift / alignment (branch %d)", i);
        FF_REQUIRE((const float*)p.y != p.x[i] && (const float*)p.y != p.xres[i], "ff_encoder_tail_fwd: the output aliases an input");
    }
    TArgs a;
    a.p = p;
    a.npix = (unsigned)p.B * (unsigned)p.HW;
    const unsigned blocks = (a.npix + TP - 1) / TP;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.w_format == FF_W_F16X3) {
        FF_ALLOW_DYNAMIC_LDS((&encoder_tail_kernel<3>), LDS_BYTES);
        encoder_tail_kernel<3><<<blocks, 256, LDS_BYTES, s>>>(a);
    } else {
        FF_ALLOW_DYNAMIC_LDS((&encoder_tail_kernel<1>), LDS_BYTES);
        encoder_tail_kernel<1><<<blocks, 256, LDS_BYTES, s>>>(a);
    }
    return ff::check_launch("ff_encoder_tail_fwd");
}
