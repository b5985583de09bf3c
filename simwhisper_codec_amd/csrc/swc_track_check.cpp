// swc_track_check: csrc/swc_track_host.h (the segment count, the workspace layout and the Q32 bounds of swc_warp) in a
// stand-alone host program, built with -fsanitize=address,undefined by build.build_track_check (tests/test_track_cpu.py).
//   swc_track_check                 the self-check: warp_bounds against a walk over every i, track_segments against a walk
//                                   over the segments, the layout's parts against their sum; prints "ok <cases>"
//   swc_track_check <query file>    one answer per line of the file:
//                                     segments n S H              -> K
//                                     layout B max_nx max_ny S H Rs -> ok peaks sums c total K R
//                                     bounds A Q nx ny cols       -> x0 m
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "swc_track_host.h"

static int fail(const char* what, long long a, long long b, long long c, long long d) {
    std::fprintf(stderr, "swc_track_check: %s (%lld %lld %lld %lld)\n", what, a, b, c, d);
    return 1;
}

static int self_check() {
    long cases = 0;
    // segments: walk k H until a segment reaches the row's end
    const int Ss[] = {0, 1, 2, 3, 16, 255, 256, 4096, 4097};
    const int Hs[] = {1, 2, 3, 128, 256, 4096, 5000};
    for (int S : Ss)
        for (int H : Hs)
            for (int64_t n = -1; n <= 9000; n += (n < 40 ? 1 : 37)) {
                int64_t want = 0;
                if (n > 0) {
                    want = 1;
                    if (S > 0)
                        while ((want - 1) * H + S < n) ++want;
                }
                if (track_segments(n, S, H) != want) return fail("segments", n, S, H, want);
                ++cases;
            }
    if (track_segments((int64_t)SWC_TRACK_MAX_N + 1, 0, 1) != -1 || track_segments(5, -1, 1) != -1 || track_segments(5, 4, 0) != -1)
        return fail("segments out of range", 0, 0, 0, 0);
    // the Q32 bounds against a walk over every i of the row
    const double as[] = {0.0, 0.25, -0.25, 3.25, -7.5, 12.3, -5.6, 40.0, -40.0, 63.999, -64.0, 100.0, -100.0, 8388608.0, -8388608.0};
    const double bs[] = {0.0, 1e-4, -1e-4, 1e-2, -1e-2};
    const int64_t ns[] = {0, 1, 2, 31, 64, 257};
    for (double a : as)
        for (double b : bs)
            for (int64_t nx : ns)
                for (int64_t ny : ns)
                    for (int64_t cols : ns) {
                        const int64_t A = (int64_t)__builtin_rint(a * 4294967296.0), Q = (int64_t)__builtin_rint((1.0 + b) * 4294967296.0);
                        int64_t first = -1, count = 0;
                        for (int64_t i = 0; i < nx; ++i) {
                            const int64_t ip = (A + i * Q) >> 32;
                            if (ip >= 0 && ip <= ny - 1) {
                                if (first < 0) first = i;
                                ++count;
                            }
                        }
                        if (count > cols) count = cols;
                        if (count == 0) first = 0;
                        int64_t x0 = -7, m = -7;
                        warp_bounds(A, Q, nx, ny, cols, &x0, &m);
                        if (x0 != first || m != count) return fail("bounds", A, Q, nx * 1000 + ny, cols);
                        ++cases;
                    }
    // at the limits: the largest row, the extreme lags
    for (double a : {8388608.0, -8388608.0, 0.0})
        for (double b : {1e-2, -1e-2}) {
            const int64_t A = (int64_t)__builtin_rint(a * 4294967296.0), Q = (int64_t)__builtin_rint((1.0 + b) * 4294967296.0);
            int64_t x0 = -7, m = -7;
            warp_bounds(A, Q, SWC_TRACK_MAX_N, SWC_TRACK_MAX_N, SWC_TRACK_MAX_N, &x0, &m);
            if (x0 < 0 || m < 0 || x0 + m > SWC_TRACK_MAX_N) return fail("bounds at the limits", A, Q, x0, m);
            if (m > 0) {
                const int64_t ip0 = (A + x0 * Q) >> 32, ip1 = (A + (x0 + m - 1) * Q) >> 32;
                if (ip0 < 0 || ip1 > SWC_TRACK_MAX_N - 1) return fail("bounds at the limits: ip", A, Q, ip0, ip1);
                if (x0 > 0 && ((A + (x0 - 1) * Q) >> 32) >= 0) return fail("bounds at the limits: x0", A, Q, x0, m);
            }
            ++cases;
        }
    // the layout: parts in order, 256-byte aligned, the largest call inside size_t
    const TrackLayout P = track_layout(65535, SWC_TRACK_MAX_N, SWC_TRACK_MAX_N, 4096, 1024, SWC_TRACK_MAX_RANGE);
    if (!P.ok || P.K != 4093 || P.R != 1041 || P.peaks != 0 || P.sums % 256 || P.c % 256 || P.total % 256 || P.total <= P.c)
        return fail("layout at the limits", (long long)P.K, (long long)P.R, (long long)P.c, (long long)P.total);
    if (track_layout(1, 10, 10, 1, 1, 0).ok == false || track_layout(1, 5000, 10, 1, 1, 0).ok) return fail("layout: K limit", 0, 0, 0, 0);
    ++cases;
    std::printf("ok %ld\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return self_check();
    std::FILE* f = std::fopen(argv[1], "r");
    if (f == nullptr) return fail("cannot open the query file", 0, 0, 0, 0);
    char line[256];
    while (std::fgets(line, sizeof line, f) != nullptr) {
        long long v[6] = {0, 0, 0, 0, 0, 0};
        char word[32] = {0};
        const int got = std::sscanf(line, "%31s %lld %lld %lld %lld %lld %lld", word, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]);
        if (got < 1) continue;
        if (std::strcmp(word, "segments") == 0 && got == 4) {
            std::printf("%lld\n", (long long)track_segments(v[0], (int32_t)v[1], (int32_t)v[2]));
        } else if (std::strcmp(word, "layout") == 0 && got == 7) {
            const TrackLayout P = track_layout((int32_t)v[0], v[1], v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)v[5]);
            std::printf("%d %zu %zu %zu %zu %lld %lld\n", P.ok ? 1 : 0, P.peaks, P.sums, P.c, P.total, (long long)P.K, (long long)P.R);
        } else if (std::strcmp(word, "bounds") == 0 && got == 6) {
            int64_t x0 = 0, m = 0;
            warp_bounds(v[0], v[1], v[2], v[3], v[4], &x0, &m);
            std::printf("%lld %lld\n", (long long)x0, (long long)m);
        } else {
            std::fclose(f);
            return fail("bad query", got, 0, 0, 0);
        }
    }
    std::fclose(f);
    return 0;
}
