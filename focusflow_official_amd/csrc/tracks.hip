// Key-point tracks of a video session (tracks.TrackTable, frames.FrameSequence(tracks=...)): a table of N slots per sample that
// follows points from frame to frame and gives each a persistent id.  Definitions: include/focusflow_hip.h; restated in
// numpy by tests/tracks_ref.py.  Every step is exact, so the tests ask for equality.
//
//   ff_tracks_replenish  the detector's points (ff_good_features) fill the free slots, unless a live track lies nearer than
//                        min_distance (fp64, every operation rounded separately)
//   ff_tracks_mask       the live positions rasterised as the 0 / 255 plane FF-RAFT reads for its first frame
//   ff_tracks_advance    every live slot moves by the flow sampled bilinearly at its sub-pixel position (fp32, every
//                        operation rounded separately: no FMA), leaves a match row, ages or dies
//
// Nothing is ordered between blocks inside a launch (the L2s of the XCDs are not coherent with each other, DESIGN section 6
// "Key points on the device"): replenish keeps a sample inside ONE block, whose LDS and barriers order it, the other two
// kernels write every element from exactly one thread, and a kernel boundary publishes.  No atomics, no allocation, no
// synchronisation; every launch goes to the caller's stream.
#pragma clang fp contract(off)
#include <climits>
#include "frame_field.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_SLOTS = 4096;               // N and M
constexpr int RB = 1024;                      // the replenish block: sixteen waves of 64
constexpr int PER = MAX_SLOTS / RB;           // consecutive slots (detections) a thread owns in the two prefix sums
constexpr int CHUNK = 8;                      // positions a detection loads from LDS before it looks at them (MAX_SLOTS % CHUNK == 0)

// Exclusive prefix sum of one int per thread over the RB threads of the block; `total` = the sum of all.  Shuffles inside a
// wave of 64, the sixteen wave sums through LDS.  Both barriers are inside: `wave_sums` may be reused at once.
__device__ __forceinline__ int block_exclusive_scan(int v, int* wave_sums, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < RB / 64; ++k) {
        const int s = wave_sums[k];
        base += k < wave ? s : 0;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

// One block per sample.  LDS: the positions of the live slots (NaN for a dead one: it is near nothing) 32 KB, the list of
// free slots 8 KB, one byte per detection 4 KB.
__global__ void __launch_bounds__(RB) replenish_kernel(float2* __restrict__ pos, long long* __restrict__ ids, int* __restrict__ age,
                                                       long long* __restrict__ next_id, int N, const int2* __restrict__ points,
                                                       const int* __restrict__ count, int M, int H, int W, int min_distance,
                                                       int* __restrict__ born, int* __restrict__ live) {
    __shared__ float2 s_pos[MAX_SLOTS];
    __shared__ unsigned short s_free[MAX_SLOTS];      // s_free[q] = the q-th free slot, ascending
    __shared__ unsigned char s_open[MAX_SLOTS];       // detection j is inside the frame, below the count and not blocked
    __shared__ int s_wave[RB / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    pos += (long long)b * N;
    ids += (long long)b * N;
    age += (long long)b * N;
    points += (long long)b * M;
    const long long first_id = next_id[b];
    const int cnt = min(max(count[b], 0), M);

    const int n_pad = (N + CHUNK - 1) / CHUNK * CHUNK;      // (the walk below reads whole chunks: the rest of the last one is dead too)
    for (int s = t; s < n_pad; s += RB) s_pos[s] = (s < N && ids[s] >= 0) ? pos[s] : make_float2(__builtin_nanf(""), __builtin_nanf(""));
    __syncthreads();

    // one thread per detection walks the table.  A slot whose fp32 |dx| or |dy| reaches min_distance + 1 cannot block: fp32
    // subtraction is off by a factor within 1 +- 2^-24, so the exact |dx| then exceeds min_distance.  Only the few slots that
    // pass this go through the fp64 definition.  The positions come CHUNK at a time, so that their LDS reads are in flight
    // together.  What bounds the walk is the vector instructions of this one compute unit, about four per track-detection pair.
    const double md2 = (double)min_distance * (double)min_distance;
    const float reach = (float)(min_distance + 1);
    for (int j = t; j < M; j += RB) {
        bool open = false;
        if (j < cnt) {
            const int2 p = points[j];
            if (p.x >= 0 && p.x < W && p.y >= 0 && p.y < H) {
                const float xf = (float)p.x, yf = (float)p.y;
                const double xd = (double)p.x, yd = (double)p.y;
                bool blocked = false;
                for (int s0 = 0; s0 < n_pad; s0 += CHUNK) {
                    float2 q[CHUNK];
#pragma unroll
                    for (int k = 0; k < CHUNK; ++k) q[k] = s_pos[s0 + k];      // (one address for the whole wave: a broadcast)
#pragma unroll
                    for (int k = 0; k < CHUNK; ++k)
                        if (fabsf(q[k].x - xf) < reach && fabsf(q[k].y - yf) < reach) {
                            const double dx = (double)q[k].x - xd, dy = (double)q[k].y - yd;
                            blocked |= dx * dx + dy * dy < md2;
                        }
                }
                open = !blocked;
            }
        }
        s_open[j] = open;
    }
    __syncthreads();

    // rank of every open detection among the open ones, and of every free slot among the free ones: thread t owns the PER
    // consecutive items PER t .. PER t + PER - 1 of both, so the order of the items is the order of the threads
    int mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int j = PER * t + k;
        mine += j < M ? (int)s_open[j] : 0;
    }
    int n_open, n_free;
    const int rank0 = block_exclusive_scan(mine, s_wave, n_open);
    mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int s = PER * t + k;
        mine += (s < N && ids[s] < 0) ? 1 : 0;
    }
    int q = block_exclusive_scan(mine, s_wave, n_free);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int s = PER * t + k;
        if (s < N && ids[s] < 0) s_free[q++] = (unsigned short)s;
    }
    __syncthreads();      // (the last read of ids lies before this barrier, the first write behind it)

    const int taken = min(n_open, n_free);
    int r = rank0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int j = PER * t + k;
        if (j < M && s_open[j]) {
            if (r < taken) {
                const int s = s_free[r];
                const int2 p = points[j];
                ids[s] = first_id + r;
                pos[s] = make_float2((float)p.x, (float)p.y);
                age[s] = 0;
            }
            ++r;
        }
    }
    if (t == 0) {
        next_id[b] = first_id + taken;
        born[b] = taken;
        live[b] = N - n_free + taken;
    }
}

__global__ void __launch_bounds__(THREADS) zero_kernel(float4* __restrict__ dst, long long n4, float* __restrict__ tail, int ntail) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * THREADS) dst[i] = z;
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0.f;
}

// one thread per slot; two tracks on one pixel store the same value
__global__ void __launch_bounds__(THREADS) mask_scatter_kernel(const float2* __restrict__ pos, const long long* __restrict__ ids, int N, int H,
                                                               int W, float* __restrict__ mask, int rows) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= rows || ids[r] < 0) return;
    const float2 p = pos[r];
    // (fmaxf / fminf drop a NaN: the conversion below always sees a number inside the frame)
    const int x = (int)fminf(fmaxf(floorf(__fadd_rn(p.x, 0.5f)), 0.f), (float)(W - 1));
    const int y = (int)fminf(fmaxf(floorf(__fadd_rn(p.y, 0.5f)), 0.f), (float)(H - 1));
    mask[(long long)(r / N) * H * W + (long long)y * W + x] = 255.f;
}

// one thread per (b, slot)
__global__ void __launch_bounds__(THREADS) advance_kernel(float2* __restrict__ pos, long long* __restrict__ ids, int* __restrict__ age, int N,
                                                          ff::Field flow, int H, int W, float4* __restrict__ matches,
                                                          unsigned char* __restrict__ valid, long long* __restrict__ ids_out,
                                                          int* __restrict__ age_out, int rows) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= rows) return;
    const long long id = ids[r];
    const int a = age[r];
    float4 m = make_float4(-1.f, -1.f, -1.f, -1.f);
    unsigned char ok = 0;
    if (id >= 0) {
        const float2 p = pos[r];
        float u, v;      // (the invariant of a live slot puts the position inside the frame; the read holds its taps there whatever the table holds)
        ff::bilinear_uv(flow, r / N, p.x, p.y, H, W, u, v);
        const float tx = __fadd_rn(p.x, u), ty = __fadd_rn(p.y, v);
        m = make_float4(p.x, p.y, tx, ty);
        ok = tx >= 0.f && tx <= (float)(W - 1) && ty >= 0.f && ty <= (float)(H - 1);      // (NaN: 0)
        pos[r] = ok ? make_float2(tx, ty) : make_float2(-1.f, -1.f);
        ids[r] = ok ? id : -1;
        age[r] = ok ? a + 1 : 0;
    }
    matches[r] = m;
    valid[r] = ok;
    ids_out[r] = id >= 0 ? id : -1;
    age_out[r] = id >= 0 ? a : 0;
}

}  // namespace

// (ff_tracks_advance has a field as well: FF_REQUIRE_FRAME_IN_FIELD says the first line again there, which costs nothing)
#define FF_REQUIRE_TRACK_FRAME(name)                                                                                              \
    FF_REQUIRE(N >= 1 && N <= MAX_SLOTS, name ": N = %d (1 .. %d slots)", N, MAX_SLOTS);                                          \
    FF_REQUIRE(B > 0 && H > 0 && W > 0, name ": B = %d, H = %d, W = %d (all > 0)", B, H, W);                                      \
    FF_REQUIRE(H <= (1 << 24) && W <= (1 << 24), name ": H = %d, W = %d (at most 2^24: positions are fp32)", H, W);               \
    FF_REQUIRE((long long)B * N <= INT_MAX / 4, name ": B = %d with N = %d (B N < 2^29)", B, N)

extern "C" int ff_tracks_replenish(float* pos, long long* ids, int* age, long long* next_id, int N, const int* points, const int* count, int M,
                                   int B, int H, int W, int min_distance, int* born, int* live, void* stream) {
    FF_REQUIRE(pos && ids && age && next_id && points && count && born && live, "ff_tracks_replenish: null pointer");
    FF_REQUIRE_TRACK_FRAME("ff_tracks_replenish");
    FF_REQUIRE(M >= 1 && M <= MAX_SLOTS, "ff_tracks_replenish: M = %d (1 .. %d detections)", M, MAX_SLOTS);
    FF_REQUIRE(min_distance >= 0 && min_distance <= 32, "ff_tracks_replenish: min_distance = %d (0 .. 32)", min_distance);
    FF_REQUIRE(((size_t)pos & 7) == 0 && ((size_t)points & 7) == 0, "ff_tracks_replenish: pos and points must be 8-byte aligned");
    replenish_kernel<<<B, RB, 0, static_cast<hipStream_t>(stream)>>>(reinterpret_cast<float2*>(pos), ids, age, next_id, N,
                                                                     reinterpret_cast<const int2*>(points), count, M, H, W, min_distance, born, live);
    return ff::check_launch("ff_tracks_replenish");
}

extern "C" int ff_tracks_mask(const float* pos, const long long* ids, int N, int B, int H, int W, float* mask, void* stream) {
    FF_REQUIRE(pos && ids && mask, "ff_tracks_mask: null pointer");
    FF_REQUIRE_TRACK_FRAME("ff_tracks_mask");
    FF_REQUIRE((long long)H * W <= INT_MAX / 4, "ff_tracks_mask: H x W = %d x %d is too large a plane", H, W);
    FF_REQUIRE(((size_t)pos & 7) == 0 && ((size_t)mask & 15) == 0, "ff_tracks_mask: pos must be 8-byte aligned, mask 16-byte aligned");
    const long long n = (long long)B * H * W, n4 = n / 4;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((n4 + THREADS - 1) / THREADS, 65535));
    zero_kernel<<<grid, THREADS, 0, s>>>(reinterpret_cast<float4*>(mask), n4, mask + 4 * n4, (int)(n - 4 * n4));
    const int rows = B * N;
    mask_scatter_kernel<<<(rows + THREADS - 1) / THREADS, THREADS, 0, s>>>(reinterpret_cast<const float2*>(pos), ids, N, H, W, mask, rows);
    return ff::check_launch("ff_tracks_mask");
}

extern "C" int ff_tracks_advance(float* pos, long long* ids, int* age, int N, const float* flow_up, long long ld_b, long long ld_c,
                                 long long ld_row, long long ld_col, int B, int left, int top, int H, int W, int Hp, int Wp, float* matches,
                                 unsigned char* valid, long long* ids_out, int* age_out, void* stream) {
    FF_REQUIRE(pos && ids && age && flow_up && matches && valid && ids_out && age_out, "ff_tracks_advance: null pointer");
    FF_REQUIRE_TRACK_FRAME("ff_tracks_advance");
    FF_REQUIRE_FRAME_IN_FIELD("ff_tracks_advance");
    FF_REQUIRE(((size_t)pos & 7) == 0 && ((size_t)matches & 15) == 0, "ff_tracks_advance: pos must be 8-byte aligned, matches 16-byte aligned");
    const int rows = B * N;
    advance_kernel<<<(rows + THREADS - 1) / THREADS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<float2*>(pos), ids, age, N, ff::frame_field(flow_up, ld_b, ld_c, ld_row, ld_col, left, top), H, W,
        reinterpret_cast<float4*>(matches), valid, ids_out, age_out, rows);
    return ff::check_launch("ff_tracks_advance");
}
