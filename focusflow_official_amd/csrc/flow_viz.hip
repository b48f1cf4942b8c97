// Flow images out of a video session (frames.FrameSequence(render=...)), and ops.flow_to_image / flow_viz.flow_to_image on their
// own: the Middlebury colour wheel (Baker et al., ICCV 2007) as the reference's core/utils/flow_viz.py::flow_to_image applies it.
// The definition - the reference's own dtype chain, fp32 up to the wheel index and fp64 behind it - is in
// include/focusflow_hip.h; tests/flow_viz_ref.py restates it in numpy and tests/golden/flow_viz.npz ties that to the reference.
//
//   ff_flow_rad_max    the per-sample maximum of the clipped flow's magnitude over the frame: the scale of the colours
//   ff_flow_to_image   fp32 field in, uint8 colours out, any layout by element strides, an occlusion plane painted over them
//
// Every step is rounded on its own (no FMA: a fused multiply-add anywhere in the chain changes bytes), fp32 division is the
// correctly rounded one, and the two fp32 square roots are taken in fp64 and rounded once, which is the correctly rounded fp32
// root (53 >= 2 * 24 + 2 bits).  The one step with latitude is the angle: atan2 in fp64, rounded once to fp32, is the correctly
// rounded fp32 value in all but rare cases, where numpy's own atan2f may be the one that is an ulp off.
//
// Traffic is 8 B in and 3 B out per pixel (5.7 MB at 540 x 960): both launches are bound by latency, not by HBM, and the ~40 fp64
// operations per pixel behind the index do not show.  What does is the shape of the stores: three bytes per pixel written by one
// lane each leave most of every write transaction empty, so for a dense (B,H,W,3) destination a lane colours FOUR consecutive
// pixels and writes their 12 bytes as three dwords, the lanes of a wave 768 consecutive bytes.  The pixels are numbered through
// the whole tensor, so rows whose 3 W is no multiple of 4 need no care of their own: only the last 1 .. 3 pixels of the tensor
// are written bytewise.  Any other destination (planes, a strided view) takes one pixel per lane and byte stores: for planes
// the lanes of a wave then write 64 consecutive bytes per channel.
//
// The maximum: non-negative floats order as their bit patterns, so the blocks of a sample meet in an unsigned atomicMax on the
// bits, which is exact and independent of the order.  The words are cleared by a memset node that ff_flow_rad_max enqueues in
// front of its kernel: a captured graph that is replayed on a frame with smaller motion starts from 0, not from the last maximum.
#pragma clang fp contract(off)
#include <climits>
#include <cmath>
#include "frame_field.h"

namespace {

constexpr int THREADS = 256;
constexpr int NCOLS = 55;
constexpr int MAX_BLOCKS_PER_SAMPLE = 256;      // of the reduction: that many atomics per sample at the most

using ff::Field;

__device__ __forceinline__ bool finite(float x) { return (__float_as_uint(x) & 0x7fffffffu) < 0x7f800000u; }
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }

// (u, v) of a pixel -> the clipped components and their magnitude; false: the vector is left out (non-finite u, v or magnitude)
__device__ __forceinline__ bool clipped(float u, float v, float clip, float& uc, float& vc, float& r) {
    uc = u;
    vc = v;
    if (clip >= 0.f) {      // np.clip(flow, 0, clip): below to 0 as well
        uc = fminf(fmaxf(u, 0.f), clip);
        vc = fminf(fmaxf(v, 0.f), clip);
    }
    r = sqrt_rn(__fadd_rn(__fmul_rn(uc, uc), __fmul_rn(vc, vc)));
    return finite(u) && finite(v) && finite(r);
}

// make_colorwheel, entry k as r | g << 8 | b << 16.  floor(255 i / n) in integers is the reference's floor of the fp64 quotient.
__device__ __forceinline__ unsigned wheel_entry(int k) {
    int r, g, b;
    if (k < 15) { r = 255; g = 255 * k / 15; b = 0; }                                        // RY
    else if (k < 21) { r = 255 - 255 * (k - 15) / 6; g = 255; b = 0; }                       // YG
    else if (k < 25) { r = 0; g = 255; b = 255 * (k - 21) / 4; }                             // GC
    else if (k < 36) { r = 0; g = 255 - 255 * (k - 25) / 11; b = 255; }                      // CB
    else if (k < 49) { r = 255 * (k - 36) / 13; g = 0; b = 255; }                            // BM
    else { r = 255; g = 0; b = 255 - 255 * (k - 49) / 6; }                                   // MR
    return (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16;
}

// The definition behind the maximum: the colour of a vector as r | g << 8 | b << 16.  `wheel`: the 55 entries in LDS.
__device__ __forceinline__ unsigned colour(float uc, float vc, float den, const unsigned* wheel) {
    const float un = __fdiv_rn(uc, den), vn = __fdiv_rn(vc, den);
    const float rad = sqrt_rn(__fadd_rn(__fmul_rn(un, un), __fmul_rn(vn, vn)));
    const float a = __fdiv_rn((float)atan2(-(double)vn, -(double)un), 3.14159274101257324f);      // (float) pi
    const float fk = __fmul_rn(__fdiv_rn(__fadd_rn(a, 1.f), 2.f), (float)(NCOLS - 1));
    const int k0 = min(max((int)floorf(fk), 0), NCOLS - 1);      // (0 .. 54 already; the clamp is a guard for the table)
    const int k1 = k0 + 1 == NCOLS ? 0 : k0 + 1;
    const double f = (double)fk - (double)k0;
    const unsigned w0 = wheel[k0], w1 = wheel[k1];
    unsigned rgb = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double c0 = (double)(w0 >> (8 * c) & 255u) / 255.0, c1 = (double)(w1 >> (8 * c) & 255u) / 255.0;
        double col = (1.0 - f) * c0 + f * c1;
        col = rad <= 1.f ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
        rgb |= (unsigned)(int)floor(255.0 * col) << (8 * c);
    }
    return rgb;
}

// grid (blocks per sample, B): every block reduces its share of sample b's frame and meets the others in one atomicMax
__global__ void __launch_bounds__(THREADS) rad_max_kernel(Field f, int H, int W, float clip, unsigned* __restrict__ rad_max) {
    __shared__ float part[THREADS / 64];
    const int b = blockIdx.y;
    const float* base = f.p + b * f.ld_b;
    const unsigned npix = (unsigned)H * (unsigned)W;
    float m = 0.f;
    for (unsigned i = blockIdx.x * THREADS + threadIdx.x; i < npix; i += gridDim.x * THREADS) {
        const unsigned y = i / (unsigned)W, x = i - y * (unsigned)W;
        const float* px = base + (long long)y * f.ld_row + (long long)x * f.ld_col;
        float uc, vc, r;
        if (clipped(px[0], px[f.ld_c], clip, uc, vc, r)) m = fmaxf(m, r);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) m = fmaxf(m, part[w]);
        atomicMax(rad_max + b, __float_as_uint(m));      // (m >= +0: the bits order as the values)
    }
}

struct Image {      // the uint8 destination by element (= byte) strides; the occlusion plane likewise (p null: none)
    unsigned char* p;
    long long ld_b, ld_row, ld_col, ld_c;
};
struct Plane {
    const unsigned char* p;
    long long ld_b, ld_row, ld_col;
};

// The colour of pixel (b, y, x) in the order of the destination's channels: byte 0 | byte 1 << 8 | byte 2 << 16.
__device__ __forceinline__ unsigned pixel(const Field& f, const Plane& occ, const float* __restrict__ rad_max, float den_fixed, float clip,
                                          unsigned paint, int swap_rb, int b, int y, int x, const unsigned* wheel) {
    if (occ.p && occ.p[b * occ.ld_b + (long long)y * occ.ld_row + (long long)x * occ.ld_col]) return paint;      // (in the destination's order already)
    const float* px = f.p + b * f.ld_b + (long long)y * f.ld_row + (long long)x * f.ld_col;
    float uc, vc, r;
    if (!clipped(px[0], px[f.ld_c], clip, uc, vc, r)) return 0u;
    const float den = rad_max ? __fadd_rn(rad_max[b], 1e-5f) : den_fixed;
    const unsigned rgb = colour(uc, vc, den, wheel);
    return swap_rb ? (rgb >> 16 & 255u) | (rgb & 0xff00u) | (rgb & 255u) << 16 : rgb;
}

__device__ __forceinline__ void fill_wheel(unsigned* wheel) {
    if (threadIdx.x < NCOLS) wheel[threadIdx.x] = wheel_entry(threadIdx.x);
    __syncthreads();
}

// any destination: one pixel per lane, three byte stores
__global__ void __launch_bounds__(THREADS) to_image_kernel(Field f, Plane occ, const float* __restrict__ rad_max, float den_fixed, float clip,
                                                           unsigned paint, int swap_rb, int H, int W, unsigned npix, Image dst) {
    __shared__ unsigned wheel[NCOLS];
    fill_wheel(wheel);
    for (unsigned i = blockIdx.x * THREADS + threadIdx.x; i < npix; i += gridDim.x * THREADS) {
        const unsigned row = i / (unsigned)W;                           // b H + y
        const int x = (int)(i - row * (unsigned)W), b = (int)(row / (unsigned)H), y = (int)(row - (unsigned)b * (unsigned)H);
        const unsigned c = pixel(f, occ, rad_max, den_fixed, clip, paint, swap_rb, b, y, x, wheel);
        unsigned char* o = dst.p + b * dst.ld_b + (long long)y * dst.ld_row + (long long)x * dst.ld_col;
        o[0] = (unsigned char)c;
        o[dst.ld_c] = (unsigned char)(c >> 8);
        o[2 * dst.ld_c] = (unsigned char)(c >> 16);
    }
}

// a contiguous, 4-byte aligned (B,H,W,3) destination: pixels 4 t .. 4 t + 3 of the whole tensor per lane, written as three dwords
__global__ void __launch_bounds__(THREADS) to_image_dense_kernel(Field f, Plane occ, const float* __restrict__ rad_max, float den_fixed, float clip,
                                                                 unsigned paint, int swap_rb, int H, int W, unsigned npix,
                                                                 unsigned char* __restrict__ dst) {
    __shared__ unsigned wheel[NCOLS];
    fill_wheel(wheel);
    const unsigned quads = (npix + 3) / 4;
    for (unsigned t = blockIdx.x * THREADS + threadIdx.x; t < quads; t += gridDim.x * THREADS) {
        const unsigned i0 = 4 * t;
        const unsigned row = i0 / (unsigned)W;
        int x = (int)(i0 - row * (unsigned)W), b = (int)(row / (unsigned)H), y = (int)(row - (unsigned)b * (unsigned)H);
        unsigned c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = i0 + j < npix ? pixel(f, occ, rad_max, den_fixed, clip, paint, swap_rb, b, y, x, wheel) : 0u;
            if (++x == W) {
                x = 0;
                if (++y == H) { y = 0; ++b; }
            }
        }
        unsigned char* o = dst + 12ll * t;
        if (i0 + 4 <= npix) {
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
            o4[0] = c[0] | c[1] << 24;
            o4[1] = c[1] >> 8 | c[2] << 16;
            o4[2] = c[2] >> 16 | c[3] << 8;
        } else {      // the last 1 .. 3 pixels of the tensor
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (i0 + j < npix) {
                    o[3 * j] = (unsigned char)c[j];
                    o[3 * j + 1] = (unsigned char)(c[j] >> 8);
                    o[3 * j + 2] = (unsigned char)(c[j] >> 16);
                }
        }
    }
}

}  // namespace

// what the two entries ask beyond the frame's place in its field
#define FF_REQUIRE_VIZ_LIMITS(name)                                                                                                         \
    FF_REQUIRE(B <= 65535, name ": B = %d (at most 65535: a grid dimension)", B);                                                           \
    FF_REQUIRE((long long)B * H * W <= (1ll << 30), name ": B H W = %d x %d x %d (at most 2^30 pixels)", B, H, W);                          \
    FF_REQUIRE(ld_b >= 0 && ld_c >= 0 && ld_row >= 0 && ld_col >= 0, name ": a negative stride of the field");                             \
    FF_REQUIRE(!(clip != clip), name ": clip is a NaN (negative: no clipping)")

extern "C" int ff_flow_rad_max(const float* flow, long long ld_b, long long ld_c, long long ld_row, long long ld_col, int B, int left, int top,
                               int H, int W, int Hp, int Wp, float clip, float* rad_max, void* stream) {
    FF_REQUIRE_FRAME_IN_FIELD("ff_flow_rad_max");
    FF_REQUIRE_VIZ_LIMITS("ff_flow_rad_max");
    FF_REQUIRE(flow && rad_max, "ff_flow_rad_max: null pointer");
    FF_REQUIRE(((size_t)rad_max & 3) == 0, "ff_flow_rad_max: rad_max must be 4-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(rad_max, 0, sizeof(float) * (size_t)B, s);
    if (e != hipSuccess) return ff::fail(FF_EHIP, "ff_flow_rad_max: hipMemsetAsync: %s", hipGetErrorString(e));
    const Field f = ff::frame_field(flow, ld_b, ld_c, ld_row, ld_col, left, top);
    const long long npix = (long long)H * W;
    // (four pixels per thread before a sample gets a second block: the blocks of a sample meet in an atomic)
    const unsigned blocks = (unsigned)std::min<long long>((npix + 4 * THREADS - 1) / (4 * THREADS), MAX_BLOCKS_PER_SAMPLE);
    rad_max_kernel<<<dim3(blocks, (unsigned)B), THREADS, 0, s>>>(f, H, W, clip, reinterpret_cast<unsigned*>(rad_max));
    return ff::check_launch("ff_flow_rad_max");
}

extern "C" int ff_flow_to_image(const float* flow, long long ld_b, long long ld_c, long long ld_row, long long ld_col, int B, int left, int top,
                                int H, int W, int Hp, int Wp, const float* rad_max, double max_flow, float clip, const unsigned char* occluded,
                                long long occ_ld_b, long long occ_ld_row, long long occ_ld_col, int occ_r, int occ_g, int occ_b, int swap_rb,
                                unsigned char* dst, long long dst_ld_b, long long dst_ld_row, long long dst_ld_col, long long dst_ld_c,
                                void* stream) {
    FF_REQUIRE_FRAME_IN_FIELD("ff_flow_to_image");
    FF_REQUIRE_VIZ_LIMITS("ff_flow_to_image");
    FF_REQUIRE(flow && dst, "ff_flow_to_image: null pointer (flow or dst)");
    FF_REQUIRE(rad_max || (max_flow > 0.0 && std::isfinite(max_flow)),
               "ff_flow_to_image: max_flow = %g without rad_max (a device maximum, or a finite max_flow > 0)", max_flow);
    FF_REQUIRE(swap_rb == 0 || swap_rb == 1, "ff_flow_to_image: swap_rb = %d (0 = R,G,B destination, 1 = B,G,R destination)", swap_rb);
    FF_REQUIRE((occ_r | occ_g | occ_b) >= 0 && (occ_r | occ_g | occ_b) <= 255, "ff_flow_to_image: occluded colour (%d, %d, %d): 0 .. 255 each", occ_r,
               occ_g, occ_b);
    FF_REQUIRE(occ_ld_b >= 0 && occ_ld_row >= 0 && occ_ld_col >= 0, "ff_flow_to_image: a negative stride of the occlusion plane");
    FF_REQUIRE(dst_ld_b >= 0 && dst_ld_row >= 0 && dst_ld_col >= 0 && dst_ld_c >= 0, "ff_flow_to_image: a negative stride of the destination");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Field f = ff::frame_field(flow, ld_b, ld_c, ld_row, ld_col, left, top);
    const Plane occ = {occluded, occ_ld_b, occ_ld_row, occ_ld_col};
    const float den_fixed = rad_max ? 0.f : (float)(max_flow + 1e-5);
    const unsigned paint = swap_rb ? (unsigned)occ_b | (unsigned)occ_g << 8 | (unsigned)occ_r << 16
                                   : (unsigned)occ_r | (unsigned)occ_g << 8 | (unsigned)occ_b << 16;
    const unsigned npix = (unsigned)((long long)B * H * W);
    const bool dense = dst_ld_c == 1 && dst_ld_col == 3 && dst_ld_row == 3ll * W && (B == 1 || dst_ld_b == 3ll * W * H) && ((size_t)dst & 3) == 0;
    if (dense) {
        const unsigned quads = (npix + 3) / 4;
        to_image_dense_kernel<<<(quads + THREADS - 1) / THREADS, THREADS, 0, s>>>(f, occ, rad_max, den_fixed, clip, paint, swap_rb, H, W, npix, dst);
    } else {
        const Image im = {dst, dst_ld_b, dst_ld_row, dst_ld_col, dst_ld_c};
        to_image_kernel<<<(npix + THREADS - 1) / THREADS, THREADS, 0, s>>>(f, occ, rad_max, den_fixed, clip, paint, swap_rb, H, W, npix, im);
    }
    return ff::check_launch("ff_flow_to_image");
}
