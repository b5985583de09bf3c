// swc_flac_frame.h — the subframe decoder of one FLAC frame (RFC 9639), written once for host and device: plain C++,
// SWC_HD is `__host__ __device__` under hipcc and empty otherwise.  csrc/swc_flac_gpu.hip runs it with one frame per lane,
// tests and the sanitizer program (csrc/swc_flac_check.cpp) run the same text on the host.
//
// Given the bytes of one frame and what swc_flac_index (include/swc_flac.h) read from its header, every subframe is decoded
// into an int32 plane: CONSTANT, VERBATIM, FIXED 0-4, LPC order 1-32, partitioned Rice with 4- and 5-bit parameters and
// escape partitions, wasted bits.  The stereo decorrelation is NOT undone here (that is sample-parallel work).
//
// The contract, whatever the bytes say:
//   * reads only frame[hdr_bytes, n_bytes - 2): the subframes and the padding, never a byte outside the frame;
//   * writes only plane c, elements [0, blocksize), c < channels (and coef[j * coef_stride], j < 32);
//   * every loop is bounded by the block size or by the frame's bit count, unary runs included;
//   * a non-zero SWC_FLAC_ST_* status for a reserved code, for a partition or predictor order inconsistent with the block
//     size, and when the bit position after the last subframe, byte aligned, is not exactly n_bytes - 2.  CRCs are not
//     recomputed: the index checked them.
// A decoded sample must fit its subframe's width (bps, + 1 for a side channel; RFC 9639 requires it of every
// encoder): a stream that breaks this gets SWC_FLAC_ST_RANGE.  That bound is what keeps every LPC sum exact in int64
// and the int32 planes bit-equal to the int64 arithmetic of csrc/swc_flac.c.
#ifndef SWC_FLAC_FRAME_H_
#define SWC_FLAC_FRAME_H_

#include <stdint.h>
#include "swc_flac.h"

#if defined(__HIPCC__)
#define SWC_HD __host__ __device__
#else
#define SWC_HD
#endif

// MSB-first bit reader over p[0, n): a left-aligned 64-bit accumulator whose bits below `bits` are always zero
struct swc_fbr {
    const uint8_t* p;
    uint32_t n, pos;  // pos: the next byte
    uint64_t acc;
    int32_t bits;
    int32_t err;      // set when a read wanted more bits than the frame holds
};

SWC_HD static inline void swc_fbr_refill(swc_fbr& b) {
    if (b.bits <= 32 && b.pos + 4u <= b.n) {  // 4 bytes at once (no alignment assumed), wholly inside the frame
        uint32_t w;
        __builtin_memcpy(&w, b.p + b.pos, 4);
        w = __builtin_bswap32(w);
        b.acc |= (uint64_t)w << (32 - b.bits);
        b.bits += 32;
        b.pos += 4;
        return;
    }
    while (b.bits <= 56 && b.pos < b.n) {
        b.acc |= (uint64_t)b.p[b.pos++] << (56 - b.bits);
        b.bits += 8;
    }
}

SWC_HD static inline uint32_t swc_fbr_read(swc_fbr& b, int k) {  // 0 <= k <= 32
    if (k == 0) return 0;
    if (b.bits < k) swc_fbr_refill(b);
    if (b.bits < k) { b.err = 1; return 0; }
    const uint32_t v = (uint32_t)(b.acc >> (64 - k));
    b.acc <<= k;
    b.bits -= k;
    return v;
}

SWC_HD static inline int32_t swc_fbr_read_signed(swc_fbr& b, int k) {  // 0 <= k <= 32
    if (k == 0) return 0;
    uint32_t v = swc_fbr_read(b, k);
    if (k < 32 && (v >> (k - 1))) v |= ~((1u << k) - 1u);
    return (int32_t)v;
}

// number of 0 bits in front of the next 1 bit; every turn of the loop that does not return consumes the accumulator and
// refills it, so the run is bounded by the frame's bit count
SWC_HD static inline uint32_t swc_fbr_unary(swc_fbr& b) {
    uint32_t q = 0;
    for (;;) {
        if (b.acc == 0) {
            q += (uint32_t)b.bits;
            b.bits = 0;
            swc_fbr_refill(b);
            if (b.bits == 0) { b.err = 1; return 0; }
            continue;
        }
        const int z = __builtin_clzll(b.acc);  // < bits: the bits below `bits` are zero
        q += (uint32_t)z;
        b.acc = z == 63 ? 0 : b.acc << (z + 1);
        b.bits -= z + 1;
        return q;
    }
}

// One subframe of `bps` bits per sample into s[0, bs).  coef: 32 int32 at stride coef_stride (registers' stand-in: LDS on
// the device, a local array on the host); the history of the predictors is read back from s.
SWC_HD static inline int swc_flac_decode_subframe(swc_fbr& b, int32_t* s, int bs, int bps, int32_t* coef, int coef_stride) {
    if (swc_fbr_read(b, 1)) return SWC_FLAC_ST_RESERVED;  // padding bit
    const int type = (int)swc_fbr_read(b, 6);
    int wasted = 0;
    if (swc_fbr_read(b, 1)) {
        const uint32_t z = swc_fbr_unary(b);
        if (b.err) return SWC_FLAC_ST_TRUNCATED;
        if (z >= (uint32_t)bps - 1u) return SWC_FLAC_ST_ORDER;
        wasted = (int)z + 1;
    }
    bps -= wasted;  // >= 1
    int order = 0, lpc = 0, shift = 0;
    if (type == 0) {  // CONSTANT
        const int32_t v = swc_fbr_read_signed(b, bps);
        if (b.err) return SWC_FLAC_ST_TRUNCATED;
        const int32_t w = (int32_t)((uint32_t)v << wasted);
        for (int i = 0; i < bs; ++i) s[i] = w;
        return SWC_FLAC_ST_OK;
    } else if (type == 1) {  // VERBATIM
        for (int i = 0; i < bs; ++i) {
            s[i] = (int32_t)((uint32_t)swc_fbr_read_signed(b, bps) << wasted);
            if (b.err) return SWC_FLAC_ST_TRUNCATED;
        }
        return SWC_FLAC_ST_OK;
    } else if (type >= 8 && type <= 12) {
        order = type - 8;
    } else if (type >= 32) {
        order = (type & 31) + 1;
        lpc = 1;
    } else {
        return SWC_FLAC_ST_RESERVED;
    }
    if (order > bs) return SWC_FLAC_ST_ORDER;
    int32_t h1 = 0, h2 = 0, h3 = 0, h4 = 0;  // the last four samples, newest first (FIXED)
    for (int i = 0; i < order; ++i) {
        const int32_t v = swc_fbr_read_signed(b, bps);
        s[i] = v;
        h4 = h3; h3 = h2; h2 = h1; h1 = v;
    }
    if (lpc) {
        const int prec = (int)swc_fbr_read(b, 4) + 1;
        if (prec == 16) return SWC_FLAC_ST_RESERVED;
        shift = swc_fbr_read_signed(b, 5);
        if (shift < 0) return SWC_FLAC_ST_RESERVED;
        for (int j = 0; j < order; ++j) coef[j * coef_stride] = swc_fbr_read_signed(b, prec);
    }
    const int method = (int)swc_fbr_read(b, 2);
    if (b.err) return SWC_FLAC_ST_TRUNCATED;
    if (method > 1) return SWC_FLAC_ST_RESERVED;
    const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
    const int porder = (int)swc_fbr_read(b, 4);
    const int parts = 1 << porder;
    if ((bs & (parts - 1)) != 0 || (bs >> porder) < order) return SWC_FLAC_ST_ORDER;
    uint64_t wide = 0;  // != 0 once a sample did not fit `bps` bits
    int i = order;
    for (int p = 0; p < parts; ++p) {
        const int end = i + (bs >> porder) - (p == 0 ? order : 0);  // <= bs
        const int k = (int)swc_fbr_read(b, pbits);
        const int raw = k == esc ? (int)swc_fbr_read(b, 5) : -1;
        for (; i < end; ++i) {
            int64_t r;
            if (raw >= 0) {
                r = swc_fbr_read_signed(b, raw);
            } else {
                const uint64_t q = swc_fbr_unary(b);
                const uint64_t u = (q << k) | swc_fbr_read(b, k);
                r = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
            }
            int64_t pred;
            if (lpc) {
                int64_t sum = 0;  // |coef| < 2^14, |s| < 2^16 (the range check below), 32 terms: exact
                for (int j = 0; j < order; ++j) sum += (int64_t)coef[j * coef_stride] * (int64_t)s[i - 1 - j];
                pred = sum >> shift;
            } else {
                switch (order) {
                    case 1: pred = h1; break;
                    case 2: pred = 2 * (int64_t)h1 - h2; break;
                    case 3: pred = 3 * (int64_t)h1 - 3 * (int64_t)h2 + h3; break;
                    case 4: pred = 4 * (int64_t)h1 - 6 * (int64_t)h2 + 4 * (int64_t)h3 - h4; break;
                    default: pred = 0; break;
                }
            }
            const int64_t v = (int64_t)((uint64_t)r + (uint64_t)pred);
            const int64_t t = v >> (bps - 1);  // 0 or -1 when v fits bps bits
            wide |= (uint64_t)(t ^ (t >> 63));
            const int32_t v32 = (int32_t)v;
            s[i] = v32;
            h4 = h3; h3 = h2; h2 = h1; h1 = v32;
        }
        if (b.err) return SWC_FLAC_ST_TRUNCATED;
        if (wide) return SWC_FLAC_ST_RANGE;
    }
    if (wasted)
        for (int j = 0; j < bs; ++j) s[j] = (int32_t)((uint32_t)s[j] << wasted);
    return SWC_FLAC_ST_OK;
}

// One frame: channels subframes into planes[c * plane_stride + i], i < blocksize.  Returns SWC_FLAC_ST_*; after a non-zero
// status the planes hold whatever was decoded up to there.
SWC_HD static inline int swc_flac_decode_frame(const uint8_t* frame, int32_t n_bytes, int32_t hdr_bytes, int32_t blocksize,
                                               int32_t channels, int32_t bps, int32_t chan_assign, int32_t* planes,
                                               int64_t plane_stride, int32_t* coef, int coef_stride) {
    if (n_bytes > SWC_FLAC_MAX_FRAME_BYTES || channels < 1 || channels > SWC_FLAC_MAX_CHANNELS || bps < 4 || bps > SWC_FLAC_MAX_BPS || blocksize < 1 ||
        blocksize > SWC_FLAC_MAX_BLOCKSIZE || hdr_bytes < 5 || n_bytes < hdr_bytes + 2 || chan_assign < 0 || chan_assign > 10 ||
        channels != (chan_assign < 8 ? chan_assign + 1 : 2))
        return SWC_FLAC_ST_ENTRY;
    swc_fbr b;
    b.p = frame; b.n = (uint32_t)(n_bytes - 2); b.pos = (uint32_t)hdr_bytes; b.acc = 0; b.bits = 0; b.err = 0;
    for (int c = 0; c < channels; ++c) {
        const int side = (chan_assign == 8 && c == 1) || (chan_assign == 9 && c == 0) || (chan_assign == 10 && c == 1);
        const int st = swc_flac_decode_subframe(b, planes + (int64_t)c * plane_stride, blocksize, bps + side, coef, coef_stride);
        if (st != SWC_FLAC_ST_OK) return st;
    }
    if (b.err) return SWC_FLAC_ST_TRUNCATED;
    // byte align: the bits consumed so far, rounded up to a byte, must be all the frame holds in front of its CRC-16
    const uint64_t used_bits = (uint64_t)b.pos * 8u - (uint64_t)b.bits;  // 64 bits: no frame length wraps it
    if ((used_bits + 7u) / 8u != (uint64_t)b.n) return SWC_FLAC_ST_LENGTH;
    return SWC_FLAC_ST_OK;
}

// The output side of one sample: planes' values (a, b of channels 0 and 1; only `a` when the frame is not stereo-coded) ->
// the sample of channel c, as csrc/swc_flac.c computes it
SWC_HD static inline int32_t swc_flac_undo_stereo(int32_t a, int32_t b, int chan_assign, int c) {
    if (chan_assign == 8) return c == 0 ? a : a - b;              // left, side
    if (chan_assign == 9) return c == 0 ? a + b : b;              // side, right
    if (chan_assign == 10) {                                      // mid, side
        const int32_t m = a * 2 + (b & 1);
        return c == 0 ? (m + b) >> 1 : (m - b) >> 1;
    }
    return c == 0 ? a : b;
}

#endif  // SWC_FLAC_FRAME_H_
