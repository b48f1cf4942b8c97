// forward_interpolate on the device (core/utils/utils.py:26-54): the warm start of the next frame pair of a video.
//
// Per sample of a (B,2,H,W) NCHW flow: source pixel (x0, y0) lands at x1 = x0 + dx, y1 = y0 + dy; it is kept iff
// 0 < x1 < W and 0 < y1 < H (strict: NaN / inf components drop out, a zero flow loses row 0 and column 0); every grid
// pixel takes BOTH components of the kept vector whose landing point is nearest (scipy.griddata 'nearest').
//   - positions and squared distances are fp64, as numpy computes them (int64 + float32 -> float64), products and the sum
//     rounded separately: nearest-neighbour decisions are those of an fp64 brute force, bit for bit
//   - ties: the minimum is taken over the key (d2, source index), so the lowest row-major source index wins whatever the
//     order in which threads or atomics meet the candidates - deterministic run to run and under graph replay
//     (scipy's own tie order is an artefact of its KD-tree and is not reproduced)
//   - ONE DELIBERATE DIFFERENCE: when no vector of a sample lands, scipy returns NaN everywhere, which would poison the
//     next forward; this kernel writes zeros (= a cold start)
//
// Algorithm (exact at every size): landed points are binned by the unit cell [cx, cx+1) x [cy, cy+1) they fall into,
// cells in row-major order (count, prefix sum, scatter: the scatter order inside a cell is arbitrary and does not matter
// to a keyed minimum).  The points of a run of cells of one row are then one contiguous range.  A grid pixel (px, py)
//   1. takes its upper bound from the two points that neighbour its own cell in that order,
//   2. walks the rows outwards, j = 0, 1, ...: rows py-1-j and py+j hold only points with |dy| >= j, so the walk ends when
//      j^2 > best d2 (strictly: an equal distance may still carry a lower index); in a row only the cells within
//      sqrt(best - j^2) (+2 cells of margin for the rounding of that bound) can hold a candidate.
// Rounding to nearest is monotone, so a bound that holds for the exact distance holds for the computed one.
// Five launches on the caller's stream, no allocation, no synchronisation; the workspace (ff_forward_interpolate_ws) is
// the caller's.  The search reads the workspace only, so `out` may alias `flow`.
#pragma clang fp contract(off)
#include <climits>
#include "ff_common.h"

namespace {

constexpr int SCAN_THREADS = 1024;
constexpr int SEARCH_THREADS = 64;      // small planes (48 x 64 = 3072 pixels) still spread over 48 CUs

// a landed point as the search reads it: one 16-byte load
struct __attribute__((aligned(16))) Landed {
    float fx, fy;      // the vector itself (what the output copies)
    int xy;            // source pixel x0 | y0 << 16
    int idx;           // y0 * W + x0: the tie-break key
};

__device__ __forceinline__ bool lands(float fx, float fy, int x0, int y0, int H, int W, double& x1, double& y1) {
    x1 = (double)x0 + (double)fx;
    y1 = (double)y0 + (double)fy;
    return x1 > 0.0 && x1 < (double)W && y1 > 0.0 && y1 < (double)H;
}

__global__ void wi_zero_kernel(int* __restrict__ cell, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) cell[i] = 0;
}

// cell[b][c] = number of vectors of sample b landing in cell c
__global__ void wi_count_kernel(const float* __restrict__ flow, int* __restrict__ cell, int B, int H, int W) {
    const int Q = H * W;
    const long long total = (long long)B * Q;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / Q), p = (int)(i - (long long)b * Q);
        const int y0 = p / W, x0 = p - y0 * W;
        const float* f = flow + (long long)b * 2 * Q;
        double x1, y1;
        if (lands(f[p], f[Q + p], x0, y0, H, W, x1, y1)) atomicAdd(cell + (long long)b * Q + (int)y1 * W + (int)x1, 1);
    }
}

// counts -> exclusive prefix sums, one block per sample: tiles of 4096 cells, four consecutive cells per thread (a wave
// reads and writes whole lines), a shuffle scan inside each wave, the sixteen wave totals through LDS, a running carry
__global__ void __launch_bounds__(SCAN_THREADS) wi_scan_kernel(int* __restrict__ cell, int Q) {
    __shared__ int wave_total[SCAN_THREADS / 64];
    int* c = cell + (long long)blockIdx.x * Q;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;
    for (int base = 0; base < Q; base += 4 * SCAN_THREADS) {      // (uniform trip count: the barriers are safe)
        const int i0 = base + 4 * t;
        int v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = i0 + k < Q ? c[i0 + k] : 0;
            sum += v[k];
        }
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = carry;
#pragma unroll
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            const int s = wave_total[w];
            before += w < wave ? s : 0;
            carry += s;
        }
        int run = before + incl - sum;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < Q) c[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();      // wave_total is rewritten by the next tile
    }
}

// scatter: the atomic cursor of a cell is its prefix sum itself, so that afterwards cell[c] = END of cell c
// (= begin of cell c + 1; the begin of cell 0 is 0)
__global__ void wi_fill_kernel(const float* __restrict__ flow, int* __restrict__ cell, Landed* __restrict__ pts, int B, int H, int W) {
    const int Q = H * W;
    const long long total = (long long)B * Q;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / Q), p = (int)(i - (long long)b * Q);
        const int y0 = p / W, x0 = p - y0 * W;
        const float* f = flow + (long long)b * 2 * Q;
        const float fx = f[p], fy = f[Q + p];
        double x1, y1;
        if (lands(fx, fy, x0, y0, H, W, x1, y1)) {
            const int slot = atomicAdd(cell + (long long)b * Q + (int)y1 * W + (int)x1, 1);      // < number landed <= Q
            pts[(long long)b * Q + slot] = Landed{fx, fy, x0 | (y0 << 16), p};
        }
    }
}

struct Best {
    double d2;
    int idx;
    float fx, fy;
};

__device__ __forceinline__ void consider(const Landed q, double px, double py, Best& best) {
    const double dx = px - ((double)(q.xy & 0xffff) + (double)q.fx);
    const double dy = py - ((double)(q.xy >> 16) + (double)q.fy);
    const double d2 = dx * dx + dy * dy;
    if (d2 < best.d2 || (d2 == best.d2 && q.idx < best.idx)) best = Best{d2, q.idx, q.fx, q.fy};
}

__global__ void __launch_bounds__(SEARCH_THREADS) wi_search_kernel(const int* __restrict__ cell_end, const Landed* __restrict__ pts,
                                                                    float* __restrict__ out, int H, int W) {
    const int Q = H * W;
    const int p = blockIdx.x * SEARCH_THREADS + threadIdx.x;
    if (p >= Q) return;
    const int b = blockIdx.y;
    const int* end = cell_end + (long long)b * Q;
    const Landed* pt = pts + (long long)b * Q;
    float* o = out + (long long)b * 2 * Q;
    const int landed = end[Q - 1];
    if (landed == 0) {      // nothing landed: a cold start (scipy: NaN)
        o[p] = 0.f;
        o[Q + p] = 0.f;
        return;
    }
    const int py = p / W, px = p - py * W;
    const double fpx = (double)px, fpy = (double)py;
    Best best{(double)INFINITY, INT_MAX, 0.f, 0.f};
    const int s = end[p];      // points in cells 0 .. p
    if (s > 0) consider(pt[s - 1], fpx, fpy, best);
    if (s < landed) consider(pt[s], fpx, fpy, best);
    for (int j = 0;; ++j) {
        const double jj = (double)j * (double)j;
        const int ra = py - 1 - j, rb = py + j;
        if (jj > best.d2 || (ra < 0 && rb >= H)) break;
        for (int side = 0; side < 2; ++side) {
            const int row = side ? rb : ra;
            const double rem = best.d2 - jj;      // (the first row of the pair may have lowered best below jj)
            if (row < 0 || row >= H || rem < 0.0) continue;
            const int r = (int)sqrt(rem) + 2;     // rem <= H^2 + W^2
            const int c0 = row * W + max(px - 1 - r, 0), c1 = row * W + min(px + r, W - 1);
            const int lo = c0 > 0 ? end[c0 - 1] : 0, hi = end[c1];
            for (int t = lo; t < hi; ++t) consider(pt[t], fpx, fpy, best);
        }
    }
    o[p] = best.fx;
    o[Q + p] = best.fy;
}

inline unsigned grid_for(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 65535); }

}  // namespace

extern "C" int ff_forward_interpolate_ws(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || H > 32767 || W > 32767) return 0;
    const long long bytes = (long long)B * H * W * (long long)(sizeof(Landed) + sizeof(int));
    return bytes <= INT_MAX ? (int)bytes : 0;
}

extern "C" int ff_forward_interpolate(const float* flow, float* out, void* ws, int B, int H, int W, void* stream) {
    FF_REQUIRE(flow && out && ws && B > 0 && H > 0 && W > 0, "ff_forward_interpolate: bad argument");
    FF_REQUIRE(ff_forward_interpolate_ws(B, H, W) > 0 && B <= 65535, "ff_forward_interpolate: plane or batch too large (%d x %d x %d)", B, H, W);
    FF_REQUIRE(((size_t)ws & 15) == 0, "ff_forward_interpolate: workspace alignment");
    const long long n = (long long)B * H * W;
    Landed* pts = static_cast<Landed*>(ws);
    int* cell = reinterpret_cast<int*>(pts + n);
    hipStream_t s = static_cast<hipStream_t>(stream);
    wi_zero_kernel<<<grid_for(n), 256, 0, s>>>(cell, n);
    wi_count_kernel<<<grid_for(n), 256, 0, s>>>(flow, cell, B, H, W);
    wi_scan_kernel<<<B, SCAN_THREADS, 0, s>>>(cell, H * W);
    wi_fill_kernel<<<grid_for(n), 256, 0, s>>>(flow, cell, pts, B, H, W);
    wi_search_kernel<<<dim3((H * W + SEARCH_THREADS - 1) / SEARCH_THREADS, B), SEARCH_THREADS, 0, s>>>(cell, pts, out, H, W);
    return ff::check_launch("ff_forward_interpolate");
}
