// A frame inside a padded field: what the kernels of a video session (frame_io.hip, tracks.hip, fb_check.hip, flow_viz.hip) share.
// The models work on fields padded to multiples of 8 (B,C,Hp,Wp); a session's consumers speak of the unpadded H x W frame that
// starts at (left, top) inside it.  One struct, one refusal, one sub-pixel read.
#pragma once
#include "ff_common.h"

// The geometry every entry with a frame in a field refuses, in the words all of them use.  Reads the entry's own B, H, W, left,
// top, Hp, Wp.  Limits that only one entry has (2^24 for fp32 positions, pixel and slot counts) stay with that entry.
#define FF_REQUIRE_FRAME_IN_FIELD(name)                                                                                     \
    FF_REQUIRE(B > 0 && H > 0 && W > 0, name ": B = %d, H = %d, W = %d (all > 0)", B, H, W);                                \
    FF_REQUIRE(left >= 0 && (long long)left + W <= Wp, name ": left = %d with W = %d does not fit Wp = %d", left, W, Wp);   \
    FF_REQUIRE(top >= 0 && (long long)top + H <= Hp, name ": top = %d with H = %d does not fit Hp = %d", top, H, Hp)

namespace ff {

// A padded fp32 field by element strides.  The one convention: `p` stands at the frame's corner, pixel (left, top) of sample 0
// and channel 0, so a kernel addresses the frame's pixel (y, x) of sample b at p + b ld_b + y ld_row + x ld_col and never sees
// left or top.  Made on the host by frame_field(), behind FF_REQUIRE_FRAME_IN_FIELD: 0 <= y < H, 0 <= x < W stays inside the field.
struct Field {
    const float* p;
    long long ld_b, ld_c, ld_row, ld_col;
};

inline Field frame_field(const float* field, long long ld_b, long long ld_c, long long ld_row, long long ld_col, int left, int top) {
    return {field + (long long)top * ld_row + (long long)left * ld_col, ld_b, ld_c, ld_row, ld_col};
}

// (u, v) = channels 0, 1 of sample b at the sub-pixel position (x, y) of its H x W frame: four taps blended in fp32, every
// operation rounded separately.  A position inside the frame has floorf in 0 .. W - 1 already; the clamps hold the taps in the
// frame whatever the position holds (fmaxf / fminf drop a NaN).  ff_tracks_advance moves a track by this read and the
// forward-backward check re-samples the flow by it, which is why there is one.
__device__ __forceinline__ void bilinear_uv(const Field& f, int b, float x, float y, int H, int W, float& u, float& v) {
    const int x0 = (int)fminf(fmaxf(floorf(x), 0.f), (float)(W - 1)), y0 = (int)fminf(fmaxf(floorf(y), 0.f), (float)(H - 1));
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = __fsub_rn(x, (float)x0), fy = __fsub_rn(y, (float)y0);
    const long long r0 = (long long)y0 * f.ld_row, r1 = (long long)y1 * f.ld_row;
    const long long c0 = (long long)x0 * f.ld_col, c1 = (long long)x1 * f.ld_col;
    const float* s = f.p + b * f.ld_b;
    u = blend(s[r0 + c0], s[r0 + c1], s[r1 + c0], s[r1 + c1], fx, fy);
    s += f.ld_c;
    v = blend(s[r0 + c0], s[r0 + c1], s[r1 + c0], s[r1 + c1], fx, fy);
}

}  // namespace ff
