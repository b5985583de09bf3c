// The arithmetic of SWC2 (include/swc_entropy.h), shared by the kernels of swc_entropy.hip, the host parser behind
// swc_entropy_parse and the stand-alone host program swc_entropy_check.cpp: the range coder's narrowing and renormalisation,
// the count update, the level split, the raw stream's bits, CRC-32 with its combination, and the walk through an image's header
// and stream table.  Plain C++ without the HIP runtime; every function runs the same lines on the host and on the device.
#ifndef SWC_ENTROPY_MODEL_H_
#define SWC_ENTROPY_MODEL_H_

#include <stddef.h>
#include <stdint.h>

#include "swc_entropy.h"

#if defined(__HIPCC__)
#define SWC_ENT_HD __host__ __device__ __forceinline__
#else
#define SWC_ENT_HD inline
#endif

constexpr uint32_t SWC_ENT_TOP = 1u << 24;
constexpr uint32_t SWC_ENT_BOT = 1u << 16;
constexpr uint32_t SWC_ENT_MAGIC = 0x32435753u;  // "SWC2", little endian

struct swc_ent_levels {
    int L[4];
    int base[4];
    int n_codes;
    int w;
};

// 0 when the four levels are inside the limits
SWC_ENT_HD int swc_ent_levels_init(swc_ent_levels& lv, int l0, int l1, int l2, int l3) {
    lv.L[0] = l0, lv.L[1] = l1, lv.L[2] = l2, lv.L[3] = l3;
    int n = 1;
    for (int d = 0; d < 4; ++d) {
        if (lv.L[d] < SWC_ENTROPY_MIN_LEVEL || lv.L[d] > SWC_ENTROPY_MAX_LEVEL) return -1;
        lv.base[d] = n;
        n *= lv.L[d];
    }
    if (n > SWC_ENTROPY_MAX_CODES) return -1;
    lv.n_codes = n;
    lv.w = 0;
    while (((n - 1) >> lv.w) != 0) ++lv.w;
    return 0;
}

SWC_ENT_HD int64_t swc_ent_raw_bytes(int64_t T, int w) { return (T * w + 7) / 8; }

// the four levels of a code below n_codes, 4 bits each (level d at bits [4 d, 4 d + 4)).  Any 32-bit value gives levels inside
// their rows: the caller decides what an invalid value means
SWC_ENT_HD uint32_t swc_ent_split(uint32_t c, const swc_ent_levels& lv) {
    uint32_t p = 0;
    for (int d = 0; d < 4; ++d) {
        p |= (c % (uint32_t)lv.L[d]) << (4 * d);
        c /= (uint32_t)lv.L[d];
    }
    return p;
}

SWC_ENT_HD uint32_t swc_ent_join(uint32_t packed, const swc_ent_levels& lv) {
    uint32_t c = 0;
    for (int d = 0; d < 4; ++d) c += ((packed >> (4 * d)) & 15u) * (uint32_t)lv.base[d];
    return c;
}

// ---- the coder.  State {low, range}; between symbols range >= SWC_ENT_BOT (header, property 1).
SWC_ENT_HD void swc_ent_narrow(uint32_t& low, uint32_t& range, uint32_t cum, uint32_t f, uint32_t tot) {
    range /= tot;
    low += cum * range;
    range *= f;
}

// one turn of the renormalisation loop: false when the state is final for this symbol; otherwise `byte` is what the encoder
// emits (the decoder shifts a byte into its code word instead) and the state has moved on.  At most SWC_ENTROPY_MAX_RENORM turns
// return true after one swc_ent_narrow (header, property 2).
SWC_ENT_HD bool swc_ent_renorm(uint32_t& low, uint32_t& range, uint32_t& byte) {
    if ((low ^ (low + range)) >= SWC_ENT_TOP) {
        if (range >= SWC_ENT_BOT) return false;
        range = (0u - low) & (SWC_ENT_BOT - 1u);
    }
    byte = low >> 24;
    low <<= 8;
    range <<= 8;
    return true;
}

// the decoder's target inside [0, tot): call AFTER range /= tot
SWC_ENT_HD uint32_t swc_ent_target(uint32_t code, uint32_t low, uint32_t range_div, uint32_t tot) {
    const uint32_t v = (code - low) / range_div;
    return v < tot - 1u ? v : tot - 1u;
}

// the count update: x is one entry of the row of the symbol just coded, tot_before the row's sum before the update
SWC_ENT_HD uint32_t swc_ent_update(uint32_t x, bool is_symbol, uint32_t tot_before) {
    if (is_symbol) x += SWC_ENTROPY_INC;
    if (tot_before + SWC_ENTROPY_INC > SWC_ENTROPY_LIMIT) x = (x + 1u) >> 1;
    return x;
}

// ---- the raw stream: byte k of the stream of w-bit values; code(t) is called for t < T only
template <typename F>
SWC_ENT_HD uint32_t swc_ent_raw_byte(uint32_t k, uint32_t T, int w, F code) {
    const uint32_t c0 = (8u * k) / (uint32_t)w;
    const uint32_t mask = (1u << w) - 1u;
    uint64_t acc = 0;
    for (int j = 0; j < 3; ++j)  // w >= 4: three values cover the byte
        if (c0 + j < T) acc |= (uint64_t)(code(c0 + j) & mask) << (w * j);
    return (uint32_t)(acc >> (8u * k - (uint32_t)w * c0)) & 0xffu;
}

// value t of a raw stream of `len` bytes at `s` (bytes behind the stream read as 0)
SWC_ENT_HD uint32_t swc_ent_raw_value(const unsigned char* s, int64_t len, uint32_t t, int w) {
    const uint32_t bit = t * (uint32_t)w;  // < 2^16 * 14
    const int64_t k = bit >> 3;
    uint32_t acc = 0;
    for (int j = 0; j < 3; ++j)  // (bit & 7) + w <= 21 bits
        if (k + j < len) acc |= (uint32_t)s[k + j] << (8 * j);
    return (acc >> (bit & 7u)) & ((1u << w) - 1u);
}

// ---- CRC-32 (zlib's: reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF)
constexpr uint32_t SWC_ENT_POLY = 0xedb88320u;

SWC_ENT_HD uint32_t swc_ent_crc_byte(uint32_t state, uint32_t byte) {  // `state` is the inverted register
    state ^= byte;
    for (int k = 0; k < 8; ++k) state = (state >> 1) ^ (SWC_ENT_POLY & (0u - (state & 1u)));
    return state;
}

// a(x) b(x) mod P in the reflected representation (x^0 = bit 31): 32 turns, whatever the operands
SWC_ENT_HD uint32_t swc_ent_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 31; k >= 0; --k) {
        p ^= b & (0u - ((a >> k) & 1u));
        b = (b >> 1) ^ (SWC_ENT_POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 n) mod P, n < 2^24: 24 turns of square and multiply
SWC_ENT_HD uint32_t swc_ent_xpow8(uint32_t n) {
    uint32_t p = 1u << 31, sq = 1u << 23;  // x^0, x^8
    for (int k = 0; k < 24; ++k) {
        if ((n >> k) & 1u) p = swc_ent_mulmod(sq, p);
        sq = swc_ent_mulmod(sq, sq);
    }
    return p;
}

// crc(A || B) from crc(A), crc(B) and the length of B in bytes
SWC_ENT_HD uint32_t swc_ent_crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) {
    return swc_ent_mulmod(swc_ent_xpow8(len_b), crc_a) ^ crc_b;
}

// byte m of the message the image's CRC covers: image bytes [0, 20) then [24, ...)
SWC_ENT_HD int64_t swc_ent_crc_index(int64_t m) { return m < 20 ? m : m + 4; }

inline uint32_t swc_ent_crc_image(const unsigned char* image, int64_t body_bytes) {
    uint32_t st = 0xffffffffu;
    for (int64_t m = 0; m < 20 + body_bytes; ++m) st = swc_ent_crc_byte(st, image[swc_ent_crc_index(m)]);
    return ~st;
}

// ---- the image
SWC_ENT_HD uint32_t swc_ent_le32(const unsigned char* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// byte q < 24 of an image's fixed header (the CRC field reads 0: it is written last)
SWC_ENT_HD uint32_t swc_ent_header_byte(int q, uint32_t T, int G, const swc_ent_levels& lv, uint32_t body_bytes) {
    uint32_t word;
    switch (q >> 2) {
        case 0: word = SWC_ENT_MAGIC; break;
        case 1: word = T; break;
        case 2: word = (uint32_t)G | ((uint32_t)lv.L[0] << 16) | ((uint32_t)lv.L[1] << 24); break;  // byte 9 = version 0
        case 3: word = (uint32_t)lv.L[2] | ((uint32_t)lv.L[3] << 8); break;
        case 4: word = body_bytes; break;
        default: word = 0; break;
    }
    return (word >> (8 * (q & 3))) & 0xffu;
}

// The host parser (swc_entropy_parse runs exactly this).  Reads image[0, bytes) only.
inline int swc_ent_parse(const unsigned char* image, int64_t bytes, int check_crc, int32_t* T_out, int32_t* G_out, int32_t* levels4,
                         int64_t* stream_off, int64_t* stream_len, int32_t* stream_mode) {
    if (image == nullptr || bytes < SWC_ENTROPY_HEADER_BYTES) return SWC_ENTROPY_E_TRUNCATED;
    if (swc_ent_le32(image) != SWC_ENT_MAGIC) return SWC_ENTROPY_E_MAGIC;
    const uint32_t T = swc_ent_le32(image + 4);
    const int G = image[8];
    if (image[9] != 0 || image[14] != 0 || image[15] != 0) return SWC_ENTROPY_E_VERSION;
    swc_ent_levels lv;
    if (G < 1 || G > SWC_ENTROPY_MAX_GROUPS || T > (uint32_t)SWC_ENTROPY_MAX_FRAMES ||
        swc_ent_levels_init(lv, image[10], image[11], image[12], image[13]) != 0)
        return SWC_ENTROPY_E_LIMITS;
    const uint32_t body = swc_ent_le32(image + 16);
    if (body < 4u * (uint32_t)G || (int64_t)body > bytes - SWC_ENTROPY_HEADER_BYTES) return SWC_ENTROPY_E_TRUNCATED;
    const int64_t raw = swc_ent_raw_bytes(T, lv.w);
    int64_t pos = SWC_ENTROPY_HEADER_BYTES + 4 * G;
    for (int g = 0; g < G; ++g) {
        const uint32_t e = swc_ent_le32(image + SWC_ENTROPY_HEADER_BYTES + 4 * g);
        const int mode = (int)(e >> 24);
        const int64_t len = e & 0xffffffu;
        if (mode > 2 || (mode == 0 && len != raw) || (mode != 0 && (T == 0 || len < 4 || len >= raw))) return SWC_ENTROPY_E_TABLE;
        if (stream_off) stream_off[g] = pos;
        if (stream_len) stream_len[g] = len;
        if (stream_mode) stream_mode[g] = mode;
        pos += len;
    }
    if (pos != SWC_ENTROPY_HEADER_BYTES + (int64_t)body) return SWC_ENTROPY_E_TABLE;
    if (check_crc && swc_ent_crc_image(image, body) != swc_ent_le32(image + 20)) return SWC_ENTROPY_E_CRC;
    if (T_out) *T_out = (int32_t)T;
    if (G_out) *G_out = G;
    if (levels4)
        for (int d = 0; d < 4; ++d) levels4[d] = lv.L[d];
    return 0;
}

// ---- the serial model and coder of one stream, for the host (the kernels keep the same counts one per lane).  `emit(byte)` /
// `next()` move the bytes.
struct swc_ent_model {
    uint32_t cnt[4][16][16];
    uint32_t prev;  // the previous frame's packed levels
    int order;
    swc_ent_levels lv;
    void init(const swc_ent_levels& l, int ord) {
        lv = l, order = ord, prev = 0;
        for (int d = 0; d < 4; ++d)
            for (int r = 0; r < 16; ++r)
                for (int s = 0; s < 16; ++s) cnt[d][r][s] = s < lv.L[d] ? 1u : 0u;
    }
    uint32_t* row(int d) { return cnt[d][order ? (prev >> (4 * d)) & 15u : 0u]; }
    void update(int d, uint32_t s) {
        uint32_t* r = row(d);
        uint32_t tot = 0;
        for (int k = 0; k < 16; ++k) tot += r[k];
        for (int k = 0; k < 16; ++k) r[k] = swc_ent_update(r[k], (uint32_t)k == s, tot);
    }
};

// codes[0, T) (all below n_codes) -> bytes through emit; returns the stream's length.  *most: the most renormalisation turns of
// one symbol
template <typename Emit>
inline int64_t swc_ent_encode_stream(const uint32_t* codes, int64_t T, const swc_ent_levels& lv, int order, Emit emit, int* most) {
    swc_ent_model m;
    m.init(lv, order);
    uint32_t low = 0, range = 0xffffffffu;
    int64_t n = 0;
    for (int64_t t = 0; t < T; ++t) {
        const uint32_t packed = swc_ent_split(codes[t], lv);
        for (int d = 0; d < 4; ++d) {
            const uint32_t s = (packed >> (4 * d)) & 15u;
            const uint32_t* r = m.row(d);
            uint32_t cum = 0, tot = 0;
            for (uint32_t k = 0; k < 16; ++k) {
                if (k < s) cum += r[k];
                tot += r[k];
            }
            swc_ent_narrow(low, range, cum, r[s], tot);
            uint32_t byte = 0;
            int turns = 0;
            while (swc_ent_renorm(low, range, byte)) {
                emit((unsigned char)byte);
                ++n, ++turns;
            }
            if (most && turns > *most) *most = turns;
            m.update(d, s);
        }
        m.prev = packed;
    }
    for (int k = 3; k >= 0; --k) emit((unsigned char)(low >> (8 * k)));
    return n + 4;
}

// any `len` bytes at s -> T codes, all below n_codes
inline void swc_ent_decode_stream(const unsigned char* s, int64_t len, int64_t T, const swc_ent_levels& lv, int order, uint32_t* codes) {
    swc_ent_model m;
    m.init(lv, order);
    uint32_t low = 0, range = 0xffffffffu, code = 0;
    int64_t pos = 0;
    for (; pos < 4; ++pos) code = (code << 8) | (pos < len ? s[pos] : 0u);
    for (int64_t t = 0; t < T; ++t) {
        uint32_t packed = 0;
        for (int d = 0; d < 4; ++d) {
            const uint32_t* r = m.row(d);
            uint32_t tot = 0;
            for (int k = 0; k < 16; ++k) tot += r[k];
            range /= tot;
            const uint32_t v = swc_ent_target(code, low, range, tot);
            uint32_t sym = 0, cum = 0;
            while (cum + r[sym] <= v) cum += r[sym++];
            low += cum * range;
            range *= r[sym];
            uint32_t byte = 0;
            while (swc_ent_renorm(low, range, byte)) {
                code = (code << 8) | (pos < len ? s[pos] : 0u);
                ++pos;
            }
            m.update(d, sym);
            packed |= sym << (4 * d);
        }
        m.prev = packed;
        codes[t] = swc_ent_join(packed, lv);
    }
}

#endif  // SWC_ENTROPY_MODEL_H_
