// Shi-Tomasi key points on the device: the `goodfeature` mask type (scripts/maskGenerate.py:11-30,
// cv.goodFeaturesToTrack(img, 500, 0.01, 10); block size 3, Sobel aperture 3, minimum eigenvalue).
//
// Per sample of a (B,C,H,W) fp32 image in [0,255], C = 1 or 3:
//   gray    every channel -> rintf, clamped to 0..255; three channels (R,G,B) -> (4899 R + 9617 G + 1868 B + 8192) >> 14
//   dx, dy  3x3 Sobel of gray, reflect-101 borders: integers in [-1020, 1020]
//   a b c   sums of dx^2, dx dy, dy^2 over the 3x3 block, reflect-101 applied to the PRODUCT planes (a box filter over
//           them), not by differentiating a reflected image: below 2^24, exact in int32
//   lambda  ((a + c) - sqrt((a - c)^2 + 4 b^2)) / 2 in fp64: the radicand is an exact integer below 2^53 and sqrt is
//           correctly rounded, so lambda has the same bits as a host evaluation; it is never negative (a c >= b^2)
//   keep    lambda > max(lambda) * quality_level (one fp64 multiply, maximum per sample)
//   cand    kept, not on the outermost ring, and >= every in-image 3x3 neighbour (a larger neighbour is itself kept)
//   order   descending lambda, ties by ascending y W + x
//   greedy  walk in that order, accept unless an accepted point has dx^2 + dy^2 < min_distance^2, stop at max_corners
//
// The walk is evaluated without a sort.  A candidate is REJECTED iff an accepted candidate lies inside its disc, and
// ACCEPTED iff every stronger candidate inside its disc is rejected; both are statements about final states, so
// rounds that read states while other waves write them can only decide late, never wrongly: whatever a wave reads as
// accepted / rejected stays so.  The strongest undecided candidate is decided in every round, so the rounds end.  Six
// rounds run over all compute units (kp_round_kernel), the rest inside one block per sample (kp_resolve_kernel), which
// then ranks the accepted points against each other (through LDS; beyond 4096 of them, after a bitwise search for the
// cut-off key of the max_corners strongest), and writes mask, points and count.
//
// Ten launches on the caller's stream, no allocation, no synchronisation; every data-dependent loop is inside a kernel.
#include <climits>
#include "ff_common.h"

namespace {

constexpr int TW = 32, TH = 8;                       // lambda tile of one 256-thread block
constexpr int GW = TW + 4, GH = TH + 4;              // gray with a 2-pixel halo
constexpr int PW = TW + 2, PH = TH + 2;              // products with a 1-pixel halo
constexpr int RESOLVE_THREADS = 1024;
constexpr int MAX_MIN_DISTANCE = 32;
constexpr int WIDE_ROUNDS = 6;                       // uniform noise and its box means at 384x512 and 544x960 need six
constexpr int RANK_LDS = 4096;                       // accepted points ranked through LDS (48 KB) up to this many
enum : unsigned char { NONE = 0, UNDECIDED = 1, ACCEPTED = 2, REJECTED = 3 };

struct Header {                    // per sample, 16 bytes
    unsigned long long max_bits;   // max lambda as its bit pattern (non-negative doubles order as integers)
    int ncand;
    int pad;
};

struct Ws {
    Header* hdr;            // [B]
    double* lam;            // [B][Q]
    int* cand;              // [B][Q] candidate pixels, arbitrary order
    int* work;              // [B][Q] scratch list of the resolve kernel
    unsigned char* state;   // [B][Q]
};

__host__ __device__ inline long long ws_bytes_per_sample(long long Q) { return (sizeof(Header) + Q * 17 + 15) & ~15ll; }

inline Ws carve(void* ws, int B, long long Q) {
    Ws w;
    char* p = static_cast<char*>(ws);
    w.hdr = reinterpret_cast<Header*>(p);
    p += (long long)B * sizeof(Header);
    w.lam = reinterpret_cast<double*>(p);
    p += (long long)B * Q * 8;
    w.cand = reinterpret_cast<int*>(p);
    p += (long long)B * Q * 4;
    w.work = reinterpret_cast<int*>(p);
    p += (long long)B * Q * 4;
    w.state = reinterpret_cast<unsigned char*>(p);
    return w;
}

__device__ __forceinline__ int reflect101(int i, int n) {      // valid for -n < i < 2n - 1; clamped beyond (ragged tiles)
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ int to_u8(float v) { return (int)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// (a, b) stronger than (c, d) in the walk's order: larger lambda, then lower index
__device__ __forceinline__ bool stronger(double la, int ia, double lb, int ib) { return la > lb || (la == lb && ia < ib); }

__global__ void kp_init_kernel(Header* __restrict__ hdr, unsigned char* __restrict__ state, float* __restrict__ mask, int* __restrict__ points,
                               int* __restrict__ count, int B, long long n, long long npts) {
    const long long i0 = blockIdx.x * 256ll + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long i = i0; i < n; i += step) {
        state[i] = NONE;
        mask[i] = 0.f;
    }
    if (points)
        for (long long i = i0; i < npts; i += step) points[i] = -1;
    if (i0 < B) {
        hdr[i0] = Header{0ull, 0, 0};
        if (count) count[i0] = 0;
    }
}

__global__ void __launch_bounds__(256) kp_lambda_kernel(const float* __restrict__ image, int channels, long long ld_b, long long ld_c, long long ld_row,
                                                        int H, int W, double* __restrict__ lam, Header* __restrict__ hdr) {
    __shared__ short gray[GH][GW];
    __shared__ int pa[PH][PW], pb[PH][PW], pc[PH][PW];
    __shared__ unsigned long long wave_max[4];
    const int b = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, t = threadIdx.x;
    const float* img = image + (long long)b * ld_b;
    for (int i = t; i < GH * GW; i += 256) {
        const int gy = i / GW, gx = i - gy * GW;
        const int y = reflect101(y0 - 2 + gy, H), x = reflect101(x0 - 2 + gx, W);
        const float* px = img + (long long)y * ld_row + x;
        int g;
        if (channels == 3)
            g = (4899 * to_u8(px[0]) + 9617 * to_u8(px[ld_c]) + 1868 * to_u8(px[2 * ld_c]) + 8192) >> 14;
        else
            g = to_u8(px[0]);
        gray[gy][gx] = (short)g;
    }
    __syncthreads();
    for (int i = t; i < PH * PW; i += 256) {
        const int py = i / PW, px = i - py * PW;
        const int y = y0 - 1 + py, x = x0 - 1 + px;
        int a = 0, bb = 0, c = 0;
        if (y <= H && x <= W) {      // (further out only feeds outputs beyond the image)
            // the product plane's value at (y, x) is the product at the reflected position, whose own 3x3 lies inside the
            // gray tile: the reflection moves by at most one pixel inwards
            const int gy = reflect101(y, H) - (y0 - 2), gx = reflect101(x, W) - (x0 - 2);
            const int tl = gray[gy - 1][gx - 1], tc = gray[gy - 1][gx], tr = gray[gy - 1][gx + 1];
            const int ml = gray[gy][gx - 1], mr = gray[gy][gx + 1];
            const int bl = gray[gy + 1][gx - 1], bc = gray[gy + 1][gx], br = gray[gy + 1][gx + 1];
            const int dx = (tr + 2 * mr + br) - (tl + 2 * ml + bl);
            const int dy = (bl + 2 * bc + br) - (tl + 2 * tc + tr);
            a = dx * dx;
            bb = dx * dy;
            c = dy * dy;
        }
        pa[py][px] = a;
        pb[py][px] = bb;
        pc[py][px] = c;
    }
    __syncthreads();
    const int ty = t / TW, tx = t - ty * TW;
    const int y = y0 + ty, x = x0 + tx;
    unsigned long long bits = 0;
    if (y < H && x < W) {
        int a = 0, bb = 0, c = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a += pa[ty + j][tx + i];
                bb += pb[ty + j][tx + i];
                c += pc[ty + j][tx + i];
            }
        const double s = (double)(a + c), d = (double)(a - c), e = (double)bb;
        const double l = (s - sqrt(d * d + 4.0 * e * e)) * 0.5;
        lam[(long long)b * H * W + (long long)y * W + x] = l;
        bits = (unsigned long long)__double_as_longlong(l);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(bits, d);
        bits = o > bits ? o : bits;
    }
    if ((t & 63) == 0) wave_max[t >> 6] = bits;
    __syncthreads();
    if (t == 0) {
        unsigned long long m = wave_max[0];
        for (int k = 1; k < 4; ++k) m = wave_max[k] > m ? wave_max[k] : m;
        if (m) atomicMax(&hdr[b].max_bits, m);
    }
}

__global__ void __launch_bounds__(256) kp_candidates_kernel(const double* __restrict__ lam, Header* __restrict__ hdr, int* __restrict__ cand,
                                                            unsigned char* __restrict__ state, int H, int W, double quality) {
    const int b = blockIdx.y, Q = H * W;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Q) return;
    const int y = p / W, x = p - y * W;
    if (y < 1 || y > H - 2 || x < 1 || x > W - 2) return;
    const double* l = lam + (long long)b * Q;
    const double thr = __longlong_as_double((long long)hdr[b].max_bits) * quality;
    const double v = l[p];
    if (!(v > thr)) return;
    bool top = true;
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
        for (int i = -1; i <= 1; ++i) top = top && l[p + j * W + i] <= v;      // (the ring test above keeps these inside the image)
    if (!top) return;
    const int slot = atomicAdd(&hdr[b].ncand, 1);      // < Q
    cand[(long long)b * Q + slot] = p;
    state[(long long)b * Q + p] = UNDECIDED;
}

// States are shared between the waves of a round while it runs, so they are read and written as relaxed atomics.  Nothing
// relies on when a store becomes visible inside a launch: a stale read (from the compute unit's L1, or from another XCD's
// L2) shows an older state, which only defers a decision, and what a launch stored is published by the kernel boundary.
// The wide rounds therefore read at workgroup scope (ordinary cached loads); the resolve kernel is one block on one
// compute unit and reads at device scope, past its L1, so that each of its rounds sees the round before.
template <bool WIDE>
__device__ __forceinline__ int ld_state(const unsigned char* s) {
    if (WIDE) return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_state(unsigned char* s, unsigned char v) { __hip_atomic_store(s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One wave (all 64 lanes) looks at the disc of candidate p and decides it if the states it reads allow; lane 0 writes.
// Four positions per lane and step: their state loads are issued together, then the lambda loads of the undecided ones.
template <bool WIDE>
__device__ __forceinline__ void decide(int p, const double* __restrict__ lam, unsigned char* state, int H, int W, int md) {
    const int lane = threadIdx.x & 63;
    const int y = p / W, x = p - y * W, r = md - 1, side = max(2 * r + 1, 0);      // (min_distance 0: an empty disc)
    const double v = lam[p];
    bool hit = false, blocked = false;
    for (int k0 = lane; k0 < side * side; k0 += 256) {      // (wave-uniform trip count)
        int q[4], s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u;
            const int j = k / side, dy = j - r, dx = k - j * side - r;
            const int yy = y + dy, xx = x + dx;
            const bool in = k < side * side && dx * dx + dy * dy < md * md && (dx != 0 || dy != 0) && yy >= 0 && yy < H && xx >= 0 && xx < W;
            q[u] = in ? yy * W + xx : p;
            s[u] = in ? ld_state<WIDE>(state + q[u]) : (int)NONE;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            hit = hit || s[u] == ACCEPTED;
            if (s[u] == UNDECIDED) blocked = blocked || stronger(lam[q[u]], q[u], v, p);
        }
    }
    const bool any_hit = __any(hit), any_blocked = __any(blocked);
    if (lane == 0) {
        if (any_hit) st_state(state + p, REJECTED);
        else if (!any_blocked) st_state(state + p, ACCEPTED);
    }
}

// one round over all compute units: one wave per candidate (four per block)
__global__ void __launch_bounds__(256) kp_round_kernel(const double* __restrict__ lam, const Header* __restrict__ hdr, const int* __restrict__ cand,
                                                       unsigned char* state, int H, int W, int md) {
    const int b = blockIdx.y, Q = H * W;
    const int n = hdr[b].ncand;
    const int wave = threadIdx.x >> 6;
    unsigned char* st = state + (long long)b * Q;
    for (int c = blockIdx.x * 4 + wave; c < n; c += gridDim.x * 4) {      // (wave-uniform: only this wave writes st[p] during this launch)
        const int p = cand[(long long)b * Q + c];
        if (__builtin_amdgcn_readfirstlane(ld_state<true>(st + p)) == UNDECIDED) decide<true>(p, lam + (long long)b * Q, st, H, W, md);
    }
}

// sum of one int per thread over the block (every thread gets it)
__device__ __forceinline__ int block_sum(int v, int* acc) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();      // (the previous result has been read)
    if (threadIdx.x == 0) *acc = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(acc, v);
    __syncthreads();
    return *acc;
}

__global__ void __launch_bounds__(RESOLVE_THREADS) kp_resolve_kernel(const double* __restrict__ lam_all, const Header* __restrict__ hdr, int* __restrict__ cand_all,
                                                                     int* __restrict__ work_all, unsigned char* state_all, int H, int W, int md,
                                                                     int max_corners, float* __restrict__ mask, int* __restrict__ points,
                                                                     int* __restrict__ count) {
    __shared__ int n_list, acc;
    __shared__ double key_l[RANK_LDS];
    __shared__ int key_p[RANK_LDS];
    const int b = blockIdx.x, Q = H * W, t = threadIdx.x, wave = t >> 6;
    const double* lam = lam_all + (long long)b * Q;
    int* cand = cand_all + (long long)b * Q;
    int* work = work_all + (long long)b * Q;
    unsigned char* st = state_all + (long long)b * Q;
    const int n = hdr[b].ncand;
    // 1. the remaining rounds (every round decides at least the strongest undecided candidate: at most n of them)
    for (int round = 0; round <= n; ++round) {
        if (t == 0) n_list = 0;
        __syncthreads();
        for (int c = t; c < n; c += RESOLVE_THREADS) {
            const int p = cand[c];
            if (ld_state<false>(st + p) == UNDECIDED) work[atomicAdd(&n_list, 1)] = p;
        }
        __syncthreads();
        const int nw = n_list;      // (block-uniform)
        if (nw == 0) break;
        for (int k = wave; k < nw; k += RESOLVE_THREADS / 64) decide<false>(work[k], lam, st, H, W, md);
        __threadfence();
        __syncthreads();
    }
    // 2. the accepted points -> work[0 .. na)
    __syncthreads();
    if (t == 0) n_list = 0;
    __syncthreads();
    for (int c = t; c < n; c += RESOLVE_THREADS) {
        const int p = cand[c];
        if (ld_state<false>(st + p) == ACCEPTED) work[atomicAdd(&n_list, 1)] = p;
    }
    __syncthreads();
    const int na = n_list;
    const int K = min(na, max_corners);
    // 3. up to RANK_LDS accepted points (the rule at a minimum distance of a few pixels leaves hundreds): their keys go to
    //    LDS, every point counts the stronger ones - its place in the walk - and the first max_corners write themselves
    if (na <= RANK_LDS) {      // (block-uniform)
        for (int k = t; k < na; k += RESOLVE_THREADS) {
            const int p = work[k];
            key_p[k] = p;
            key_l[k] = lam[p];
        }
        __syncthreads();
        for (int k = t; k < na; k += RESOLVE_THREADS) {
            const int p = key_p[k];
            const double v = key_l[k];
            int rank = 0;
            for (int j = 0; j < na; ++j) rank += stronger(key_l[j], key_p[j], v, p);
            if (rank >= max_corners) continue;
            mask[(long long)b * Q + p] = 255.f;
            if (points) {
                int* row = points + ((long long)b * max_corners + rank) * 2;
                row[0] = p % W;
                row[1] = p / W;
            }
        }
        if (t == 0 && count) count[b] = K;
        return;
    }
    // 3'. more than that (min_distance 0 or 1 on a busy image): the cut-off key of the K strongest, i.e. the largest T with
    //    #{lambda >= T} >= K, bit by bit, then among lambda == T the index U of the last one kept
    unsigned long long T = 0;
    int U = INT_MAX;
    if (K < na) {      // (block-uniform)
        for (int bit = 62; bit >= 0; --bit) {
            const unsigned long long trial = T | (1ull << bit);
            int c = 0;
            for (int k = t; k < na; k += RESOLVE_THREADS) c += (unsigned long long)__double_as_longlong(lam[work[k]]) >= trial;
            if (block_sum(c, &acc) >= K) T = trial;
        }
        int above = 0;
        for (int k = t; k < na; k += RESOLVE_THREADS) above += (unsigned long long)__double_as_longlong(lam[work[k]]) > T;
        const int need = K - block_sum(above, &acc);      // >= 1 of the points with lambda == T
        U = 0;      // the largest U with #{lambda == T, index < U} < need is the need-th smallest index
        for (int bit = 30; bit >= 0; --bit) {
            const int trial = U | (1 << bit);
            int c = 0;
            for (int k = t; k < na; k += RESOLVE_THREADS) {
                const int p = work[k];
                c += (unsigned long long)__double_as_longlong(lam[p]) == T && p < trial;
            }
            if (block_sum(c, &acc) < need) U = trial;
        }
    }
    // 4. the kept points -> cand[0 .. K) (the candidate list is no longer needed), then their ranks
    __syncthreads();
    if (t == 0) n_list = 0;
    __syncthreads();
    for (int k = t; k < na; k += RESOLVE_THREADS) {
        const int p = work[k];
        const unsigned long long bits = (unsigned long long)__double_as_longlong(lam[p]);
        if (bits > T || (bits == T && p <= U)) cand[atomicAdd(&n_list, 1)] = p;
    }
    __threadfence_block();
    __syncthreads();
    for (int k = t; k < K; k += RESOLVE_THREADS) {
        const int p = cand[k];
        const double v = lam[p];
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const int q = cand[j];
            rank += stronger(lam[q], q, v, p);
        }
        const int y = p / W, x = p - y * W;
        mask[(long long)b * Q + p] = 255.f;
        if (points) {
            int* row = points + ((long long)b * max_corners + rank) * 2;
            row[0] = x;
            row[1] = y;
        }
    }
    if (t == 0 && count) count[b] = K;
}

}  // namespace

extern "C" int ff_good_features_ws(int B, int H, int W) {
    if (B <= 0 || H < 3 || W < 3 || H > 32767 || W > 32767) return 0;
    const long long Q = (long long)H * W;
    if (Q > INT_MAX / 32) return 0;
    const long long bytes = (long long)B * ws_bytes_per_sample(Q);
    return bytes <= INT_MAX ? (int)bytes : 0;
}

extern "C" int ff_good_features(const float* image, int channels, long long ld_b, long long ld_c, long long ld_row, int B, int H, int W,
                                int max_corners, double quality_level, int min_distance, void* ws, float* mask, int* points, int* count,
                                void* stream) {
    FF_REQUIRE(image && ws && mask && B > 0, "ff_good_features: bad argument (null pointer or B = %d)", B);
    FF_REQUIRE(channels == 1 || channels == 3, "ff_good_features: channels = %d (1 = gray or 3 = R,G,B)", channels);
    FF_REQUIRE(H >= 3 && W >= 3, "ff_good_features: H = %d, W = %d (a 3x3 Sobel with reflect-101 borders needs H, W >= 3)", H, W);
    FF_REQUIRE(max_corners >= 1, "ff_good_features: max_corners = %d (>= 1)", max_corners);
    FF_REQUIRE(quality_level > 0.0 && quality_level <= 1.0, "ff_good_features: quality_level = %g (0 < quality_level <= 1)", quality_level);
    FF_REQUIRE(min_distance >= 0 && min_distance <= MAX_MIN_DISTANCE, "ff_good_features: min_distance = %d (0 .. %d)", min_distance, MAX_MIN_DISTANCE);
    FF_REQUIRE(ff_good_features_ws(B, H, W) > 0 && B <= 65535, "ff_good_features: plane or batch too large (%d x %d x %d)", B, H, W);
    FF_REQUIRE((long long)B * max_corners <= INT_MAX / 2, "ff_good_features: max_corners = %d is too large for a batch of %d", max_corners, B);
    FF_REQUIRE(((size_t)ws & 15) == 0, "ff_good_features: workspace alignment");
    const long long Q = (long long)H * W, n = (long long)B * Q;
    const Ws w = carve(ws, B, Q);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned fill = (unsigned)std::min<long long>((n + 255) / 256, 65535);
    kp_init_kernel<<<fill, 256, 0, s>>>(w.hdr, w.state, mask, points, count, B, n, (long long)B * max_corners * 2);
    kp_lambda_kernel<<<dim3((W + TW - 1) / TW, (H + TH - 1) / TH, B), 256, 0, s>>>(image, channels, ld_b, ld_c, ld_row, H, W, w.lam, w.hdr);
    kp_candidates_kernel<<<dim3((unsigned)((Q + 255) / 256), B), 256, 0, s>>>(w.lam, w.hdr, w.cand, w.state, H, W, quality_level);
    const unsigned round_blocks = (unsigned)std::min<long long>((Q / 16 + 3) / 4 + 1, 4096);      // (a wave per candidate if one pixel in 16 is one)
    for (int r = 0; r < WIDE_ROUNDS; ++r) kp_round_kernel<<<dim3(round_blocks, B), 256, 0, s>>>(w.lam, w.hdr, w.cand, w.state, H, W, min_distance);
    kp_resolve_kernel<<<B, RESOLVE_THREADS, 0, s>>>(w.lam, w.hdr, w.cand, w.work, w.state, H, W, min_distance, max_corners, mask, points, count);
    return ff::check_launch("ff_good_features");
}
