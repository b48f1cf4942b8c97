// The two ends of a video session (frames.FrameSequence): a decoder's uint8 frame in, key-point matches out.
//
//   ff_frame_ingest      uint8 frame, any layout given by element strides -> the contiguous fp32 (B,3,Hp,Wp) R,G,B tensor
//                        the models take, replicate-padded: x.permute(...).float() + InputPadder.pad (utils.py:5-19,
//                        F.pad(mode="replicate")).  uint8 -> fp32 is exact, so the result has the torch route's bits.
//   ff_pad_replicate     the same padding for a one-channel mask, uint8 or fp32 (evaluate.py pads its masks with the images)
//   ff_keypoint_matches  the detector's points (ff_good_features) and the flow at them -> [x, y, x + u, y + v] and a
//                        validity byte: what a tracking consumer reads instead of the dense field
//
// Every output element is written by exactly one thread from values it loads itself: no atomics, no LDS, no ordering
// between threads.  One launch each on the caller's stream, no allocation, no synchronisation.
#include <climits>
#include "frame_field.h"

namespace {

constexpr int THREADS = 256;

// dst[b][c][y][x] = (float) src[b sb + cmap(c) sc + clamp(y - top, 0, H-1) sy + clamp(x - left, 0, W-1) sx]
// One thread per destination pixel, all channels: a wave reads 64 neighbouring pixels of a row (HWC: 192 consecutive bytes)
// and writes 256 consecutive bytes per channel plane.
template <typename T>
__global__ void __launch_bounds__(THREADS) pad_convert_kernel(const T* __restrict__ src, long long sb, long long sy, long long sx, long long sc,
                                                              int channels, int swap_rb, int H, int W, int left, int top, int Hp, int Wp,
                                                              float* __restrict__ dst, long long npix) {
    const long long plane = (long long)Hp * Wp;
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < npix; i += (long long)gridDim.x * THREADS) {
        const long long b = i / plane;
        const int p = (int)(i - b * plane);
        const int y = p / Wp, x = p - y * Wp;
        const int yy = min(max(y - top, 0), H - 1), xx = min(max(x - left, 0), W - 1);
        const T* px = src + b * sb + (long long)yy * sy + (long long)xx * sx;
        float* out = dst + b * channels * plane + p;
        for (int c = 0; c < channels; ++c) {
            const int cs = swap_rb ? channels - 1 - c : c;
            out[c * plane] = (float)px[cs * sc];
        }
    }
}

// one thread per (b, n) row
__global__ void __launch_bounds__(THREADS) matches_kernel(const int* __restrict__ points, const int* __restrict__ count, int N,
                                                          ff::Field flow, int H, int W, float4* __restrict__ matches,
                                                          unsigned char* __restrict__ valid, int rows) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= rows) return;
    const int b = r / N, n = r - b * N;
    float4 m = make_float4(-1.f, -1.f, -1.f, -1.f);
    unsigned char ok = 0;
    const int x = points[2 * (long long)r], y = points[2 * (long long)r + 1];
    // (a row of the count whose point lies outside the frame is not the detector's: it is written as an empty row, never read through)
    if (n < count[b] && x >= 0 && x < W && y >= 0 && y < H) {
        const float* f = flow.p + b * flow.ld_b + (long long)y * flow.ld_row + (long long)x * flow.ld_col;
        const float u = f[0], v = f[flow.ld_c];
        const float tx = (float)x + u, ty = (float)y + v;
        m = make_float4((float)x, (float)y, tx, ty);
        ok = tx >= 0.f && tx <= (float)(W - 1) && ty >= 0.f && ty <= (float)(H - 1);      // (NaN: 0)
    }
    matches[r] = m;
    valid[r] = ok;
}

inline unsigned grid_for(long long n) { return (unsigned)std::min<long long>((n + THREADS - 1) / THREADS, 65535); }

template <typename T>
int launch_pad(const char* what, const T* src, long long sb, long long sy, long long sx, long long sc, int channels, int swap_rb, int B, int H,
               int W, int left, int top, int Hp, int Wp, float* dst, void* stream) {
    const long long npix = (long long)B * Hp * Wp;
    pad_convert_kernel<T><<<grid_for(npix), THREADS, 0, static_cast<hipStream_t>(stream)>>>(src, sb, sy, sx, sc, channels, swap_rb, H, W, left, top, Hp,
                                                                                           Wp, dst, npix);
    return ff::check_launch(what);
}

}  // namespace

extern "C" int ff_frame_ingest(const unsigned char* src, long long ld_b, long long ld_row, long long ld_col, long long ld_c, int swap_rb, int B,
                               int H, int W, int left, int top, int Hp, int Wp, float* dst, void* stream) {
    FF_REQUIRE(src && dst, "ff_frame_ingest: null pointer (src or dst)");
    FF_REQUIRE_FRAME_IN_FIELD("ff_frame_ingest");
    FF_REQUIRE((long long)Hp * Wp <= INT_MAX / 4, "ff_frame_ingest: Hp x Wp = %d x %d is too large a plane", Hp, Wp);
    FF_REQUIRE(swap_rb == 0 || swap_rb == 1, "ff_frame_ingest: swap_rb = %d (0 = R,G,B source, 1 = B,G,R source)", swap_rb);
    return launch_pad("ff_frame_ingest", src, ld_b, ld_row, ld_col, ld_c, 3, swap_rb, B, H, W, left, top, Hp, Wp, dst, stream);
}

extern "C" int ff_pad_replicate(const void* src, int src_is_u8, long long ld_b, long long ld_row, long long ld_col, int B, int H, int W, int left,
                                int top, int Hp, int Wp, float* dst, void* stream) {
    FF_REQUIRE(src && dst, "ff_pad_replicate: null pointer (src or dst)");
    FF_REQUIRE_FRAME_IN_FIELD("ff_pad_replicate");
    FF_REQUIRE((long long)Hp * Wp <= INT_MAX / 4, "ff_pad_replicate: Hp x Wp = %d x %d is too large a plane", Hp, Wp);
    FF_REQUIRE(src_is_u8 == 0 || src_is_u8 == 1, "ff_pad_replicate: src_is_u8 = %d (0 = fp32 source, 1 = uint8 source)", src_is_u8);
    if (src_is_u8)
        return launch_pad("ff_pad_replicate", static_cast<const unsigned char*>(src), ld_b, ld_row, ld_col, 0, 1, 0, B, H, W, left, top, Hp, Wp, dst,
                          stream);
    FF_REQUIRE(((size_t)src & 3) == 0, "ff_pad_replicate: src alignment (fp32)");
    return launch_pad("ff_pad_replicate", static_cast<const float*>(src), ld_b, ld_row, ld_col, 0, 1, 0, B, H, W, left, top, Hp, Wp, dst, stream);
}

extern "C" int ff_keypoint_matches(const int* points, const int* count, int N, const float* flow_up, long long ld_b, long long ld_c, long long ld_row,
                                   long long ld_col, int B, int left, int top, int H, int W, int Hp, int Wp, float* matches, unsigned char* valid,
                                   void* stream) {
    FF_REQUIRE(points && count && flow_up && matches && valid, "ff_keypoint_matches: null pointer");
    FF_REQUIRE(B > 0 && N > 0 && (long long)B * N <= INT_MAX / 4, "ff_keypoint_matches: B = %d, N = %d (both > 0, B N < 2^29)", B, N);
    FF_REQUIRE_FRAME_IN_FIELD("ff_keypoint_matches");
    FF_REQUIRE(((size_t)matches & 15) == 0, "ff_keypoint_matches: matches must be 16-byte aligned");
    const int rows = B * N;
    matches_kernel<<<(rows + THREADS - 1) / THREADS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        points, count, N, ff::frame_field(flow_up, ld_b, ld_c, ld_row, ld_col, left, top), H, W, reinterpret_cast<float4*>(matches), valid, rows);
    return ff::check_launch("ff_keypoint_matches");
}
