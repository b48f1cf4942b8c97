// Forward-backward consistency of a video session (frames.FrameSequence(fb=...)): the round trip of a start point through the
// forward flow and the backward flow sampled at its target, against the criterion of UnFlow (Meister et al. 2018).
// Definitions: include/focusflow_hip.h; restated in numpy by tests/fb_ref.py.  Every step is exact (fp32, every operation
// rounded separately: no FMA), so the tests ask for equality.
//
//   ff_fb_dense     every pixel of the frame is a start point: the squared round-trip error and the occlusion map
//   ff_fb_matches   the rows of a matches / valid pair are the start points: error and status per row, valid cleared where the
//                   row is inconsistent, and the slots of such rows die in an optional track table
//
// Both kernels write every element from exactly one thread: no atomics, no allocation, no synchronisation; every launch goes
// to the caller's stream.
//
// The dense kernel is bound by memory, and what bounds it is the gather: per pixel 8 B of forward flow in, eight taps of the
// backward flow, 5 B out.  ONE pixel per thread, every access 4 bytes (1 byte for the map) per lane: a flow is smooth, so the taps of
// the 64 neighbouring pixels of a wave are neighbours too and each gather instruction stays on a few lines, exactly like the
// two coalesced streams.  Wider accesses were built and measured and lost (profiles/fb_dense_variants.txt): the window offset
// `left` and an odd W leave either the frame's rows or the outputs' rows off 16-byte alignment, so one side has to be strided,
// and four pixels per lane - whether aligned to the padded field's columns for 16-byte loads, or to the outputs for 16-byte
// stores - spread every gather instruction of a wave over four times the addresses: 1.6x and 2.1x the time at 1080 x 1920.
#pragma clang fp contract(off)
#include <climits>
#include "frame_field.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_ROWS = 4096;      // N of ff_fb_matches: the slots of a track table, the points of a detector

using ff::Field;

// The definition.  (X, Y) -> (xt, yt) is the forward step, `bw` the backward field, b the sample.  -> inconsistent; err2 by
// reference (+inf where the target lies outside the frame: the backward field is not read then).
__device__ __forceinline__ bool round_trip(float X, float Y, float xt, float yt, const Field& bw, int b, int H, int W, float alpha, float beta,
                                           float& err2) {
    const bool inside = xt >= 0.f && xt <= (float)(W - 1) && yt >= 0.f && yt <= (float)(H - 1);      // (NaN: false)
    if (!inside) {
        err2 = __builtin_inff();
        return true;
    }
    float ub, vb;
    ff::bilinear_uv(bw, b, xt, yt, H, W, ub, vb);      // (the read ff_tracks_advance moves its tracks by)
    const float du = __fsub_rn(__fadd_rn(xt, ub), X), dv = __fsub_rn(__fadd_rn(yt, vb), Y);
    err2 = __fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv));
    const float fu = __fsub_rn(xt, X), fv = __fsub_rn(yt, Y);
    const float mf = __fadd_rn(__fmul_rn(fu, fu), __fmul_rn(fv, fv));
    const float mb = __fadd_rn(__fmul_rn(ub, ub), __fmul_rn(vb, vb));
    const float bound = __fadd_rn(__fmul_rn(alpha, __fadd_rn(mf, mb)), beta);
    return !(err2 <= bound);      // (a NaN anywhere: inconsistent)
}

// one thread per pixel; I: the type the flat index and its two divisions are done in (unsigned wherever B H W allows: a 64-bit
// division costs as much as the rest of the pixel)
template <typename I>
__global__ void __launch_bounds__(THREADS) fb_dense_kernel(Field fw, Field bw, int H, int W, I npix, float alpha, float beta,
                                                           float* __restrict__ err2, unsigned char* __restrict__ occluded) {
    for (I i = blockIdx.x * (I)THREADS + threadIdx.x; i < npix; i += (I)gridDim.x * THREADS) {
        const I row = i / (I)W;                           // b H + y
        const int x = (int)(i - row * (I)W), b = (int)(row / (I)H), y = (int)(row - (I)b * (I)H);
        const float* f = fw.p + b * fw.ld_b + (long long)y * fw.ld_row + (long long)x * fw.ld_col;
        const float X = (float)x, Y = (float)y;
        float e;
        const bool bad = round_trip(X, Y, __fadd_rn(X, f[0]), __fadd_rn(Y, f[fw.ld_c]), bw, b, H, W, alpha, beta, e);
        err2[i] = e;
        occluded[i] = bad ? 1 : 0;
    }
}

// one thread per row (b, n)
__global__ void __launch_bounds__(THREADS) fb_matches_kernel(const float4* __restrict__ matches, unsigned char* __restrict__ valid, int N,
                                                             Field bw, int H, int W, float alpha, float beta, float2* __restrict__ pos,
                                                             long long* __restrict__ ids, int* __restrict__ age, float* __restrict__ err2,
                                                             unsigned char* __restrict__ status, int rows) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= rows) return;
    const float4 m = matches[r];
    const unsigned char ok = valid[r];
    float e = -1.f;
    unsigned char st = 0;
    if (!(m.x < 0.f)) {                                   // a row: a no-row holds x = -1
        if (!ok) {
            e = __builtin_inff();
            st = 2;
        } else {
            st = round_trip(m.x, m.y, m.z, m.w, bw, r / N, H, W, alpha, beta, e) ? 3 : 1;
        }
    }
    err2[r] = e;
    status[r] = st;
    valid[r] = st == 1;
    if (st == 3 && pos) {
        pos[r] = make_float2(-1.f, -1.f);
        ids[r] = -1;
        age[r] = 0;
    }
}

}  // namespace

// what the two entries ask beyond the frame's place in its field
#define FF_REQUIRE_FB_LIMITS(name)                                                                                          \
    FF_REQUIRE(H <= (1 << 24) && W <= (1 << 24), name ": H = %d, W = %d (at most 2^24: positions are fp32)", H, W);         \
    FF_REQUIRE(alpha >= 0.f && beta >= 0.f, name ": alpha = %g, beta = %g (both >= 0, no NaN)", (double)alpha, (double)beta)

extern "C" int ff_fb_dense(const float* fw, long long fw_ld_b, long long fw_ld_c, long long fw_ld_row, long long fw_ld_col, const float* bw,
                           long long bw_ld_b, long long bw_ld_c, long long bw_ld_row, long long bw_ld_col, int B, int left, int top, int H, int W,
                           int Hp, int Wp, float alpha, float beta, float* err2, unsigned char* occluded, void* stream) {
    FF_REQUIRE_FRAME_IN_FIELD("ff_fb_dense");      // (first: the outputs of an empty frame have no address, and the refusal should name the frame)
    FF_REQUIRE_FB_LIMITS("ff_fb_dense");
    FF_REQUIRE(fw && bw && err2 && occluded, "ff_fb_dense: null pointer");
    const long long npix = (long long)B * H * W;
    const unsigned grid = (unsigned)std::min<long long>((npix + THREADS - 1) / THREADS, 1 << 20);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Field f = ff::frame_field(fw, fw_ld_b, fw_ld_c, fw_ld_row, fw_ld_col, left, top);
    const Field back = ff::frame_field(bw, bw_ld_b, bw_ld_c, bw_ld_row, bw_ld_col, left, top);
    if (npix <= (1ll << 31))      // (an index below 2^31 plus the loop's step of at most 2^28 fits an unsigned)
        fb_dense_kernel<unsigned><<<grid, THREADS, 0, s>>>(f, back, H, W, (unsigned)npix, alpha, beta, err2, occluded);
    else
        fb_dense_kernel<long long><<<grid, THREADS, 0, s>>>(f, back, H, W, npix, alpha, beta, err2, occluded);
    return ff::check_launch("ff_fb_dense");
}

extern "C" int ff_fb_matches(const float* matches, unsigned char* valid, int N, const float* bw, long long bw_ld_b, long long bw_ld_c,
                             long long bw_ld_row, long long bw_ld_col, int B, int left, int top, int H, int W, int Hp, int Wp, float alpha,
                             float beta, float* pos, long long* ids, int* age, float* err2, unsigned char* status, void* stream) {
    FF_REQUIRE(N >= 1 && N <= MAX_ROWS, "ff_fb_matches: N = %d (1 .. %d rows)", N, MAX_ROWS);
    FF_REQUIRE_FRAME_IN_FIELD("ff_fb_matches");
    FF_REQUIRE_FB_LIMITS("ff_fb_matches");
    FF_REQUIRE(matches && valid && bw && err2 && status, "ff_fb_matches: null pointer");
    FF_REQUIRE((pos && ids && age) || (!pos && !ids && !age), "ff_fb_matches: a track table is pos, ids and age: all three or none");
    FF_REQUIRE((long long)B * N <= INT_MAX / 4, "ff_fb_matches: B = %d with N = %d (B N < 2^29)", B, N);
    FF_REQUIRE(((size_t)matches & 15) == 0 && ((size_t)pos & 7) == 0, "ff_fb_matches: matches must be 16-byte aligned, pos 8-byte aligned");
    const int rows = B * N;
    fb_matches_kernel<<<(rows + THREADS - 1) / THREADS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const float4*>(matches), valid, N, ff::frame_field(bw, bw_ld_b, bw_ld_c, bw_ld_row, bw_ld_col, left, top), H, W, alpha, beta,
        reinterpret_cast<float2*>(pos), ids, age, err2, status, rows);
    return ff::check_launch("ff_fb_matches");
}
