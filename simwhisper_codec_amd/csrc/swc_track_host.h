// The serial integer arithmetic of swc_track.hip (include/swc_track.h) that needs no device: the segment count, the workspace
// layout and the Q32 position bounds of swc_warp.  Plain C++ with no HIP in it, so that the same text is compiled into the
// library (host and device) and into swc_track_check, a stand-alone host program built with -fsanitize=address,undefined.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "swc_track.h"

#if defined(__HIPCC__)
#define SWC_TRACK_HD __host__ __device__
#else
#define SWC_TRACK_HD
#endif

// K of the header; -1 for arguments out of range
SWC_TRACK_HD inline int64_t track_segments(int64_t n, int32_t S, int32_t H) {
    if (n > SWC_TRACK_MAX_N || S < 0 || (S > 0 && H < 1)) return -1;
    if (n <= 0) return 0;
    if (S == 0 || n <= S) return 1;
    return (n - S + H - 1) / H + 1;
}

inline size_t track_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// where swc_lag_track keeps what inside its workspace (byte offsets): the peaks [2][B] u32, the sums of |q| [2][B] i64 and
// c [B][K][2 R + 1] i64.  total == 0 with ok == false: arguments out of range
struct TrackLayout {
    size_t peaks, sums, c, total;
    int64_t K, R;
    bool ok;
};

inline TrackLayout track_layout(int32_t B, int64_t max_nx, int64_t max_ny, int32_t S, int32_t H, int32_t Rs) {
    TrackLayout P = {0, 0, 0, 0, 0, 0, false};
    if (B < 0 || B > 65535 || max_nx < 0 || max_nx > SWC_TRACK_MAX_N || max_ny < 0 || max_ny > SWC_TRACK_MAX_N || Rs < 0 ||
        Rs > SWC_TRACK_MAX_RANGE)
        return P;
    P.K = track_segments(max_nx, S, H);
    if (P.K < 0 || P.K > SWC_TRACK_MAX_SEGMENTS) return P;
    P.R = (int64_t)Rs + SWC_TRACK_W + 1;
    size_t o = 0;
    P.peaks = o; o += track_up256((size_t)2 * B * sizeof(uint32_t));
    P.sums = o; o += track_up256((size_t)2 * B * sizeof(int64_t));
    P.c = o; o += track_up256((size_t)B * (size_t)P.K * (size_t)(2 * P.R + 1) * sizeof(int64_t));  // < 2^16 2^12 2^12 2^3
    P.total = o;
    P.ok = true;
    return P;
}

// floor and ceiling of a / q for q > 0 (C++ division truncates towards zero)
SWC_TRACK_HD inline int64_t track_floor_div(int64_t a, int64_t q) { return a / q - ((a % q) < 0 ? 1 : 0); }
SWC_TRACK_HD inline int64_t track_ceil_div(int64_t a, int64_t q) { return a / q + ((a % q) > 0 ? 1 : 0); }

// x0 and m of swc_warp from A = rint(a 2^32), Q = rint((1 + b) 2^32) with |A| <= 2^55, 0.99 2^32 <= Q <= 1.01 2^32,
// 0 <= nx, ny, cols <= 2^22: ny 2^32 <= 2^54 and i Q < 2^55, every term far inside int64
SWC_TRACK_HD inline void warp_bounds(int64_t A, int64_t Q, int64_t nx, int64_t ny, int64_t cols, int64_t* x0, int64_t* m) {
    const int64_t first = track_ceil_div(-A, Q);
    const int64_t last = track_floor_div((ny << 32) - 1 - A, Q);
    const int64_t lo = first > 0 ? first : 0;
    int64_t hi = last + 1 < nx ? last + 1 : nx;
    int64_t len = hi - lo;
    len = len < cols ? len : cols;
    len = len > 0 ? len : 0;
    *x0 = len > 0 ? lo : 0;
    *m = len;
}
