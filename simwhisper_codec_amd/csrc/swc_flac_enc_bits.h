// swc_flac_enc_bits.h — the serial pieces of the FLAC encoder (include/swc_flac_enc.h), written once for host and device:
// plain C++, SWC_HD is `__host__ __device__` under hipcc and empty otherwise.  The frame header with its CRC-8, the CRC-16
// algebra that lets 256 threads share one frame's checksum, the STREAMINFO image and the MD5 block function.  Integer
// arithmetic only; every loop has a constant bound.
#ifndef SWC_FLAC_ENC_BITS_H_
#define SWC_FLAC_ENC_BITS_H_

#include <stdint.h>
#include "swc_flac_enc.h"

#if defined(__HIPCC__)
#define SWC_HD __host__ __device__
#else
#define SWC_HD
#endif

// RFC 9639's frame-header code of a sample rate: 1 .. 11 from the table, 13 (16 bits of Hz follow) for any other rate up to
// 65535, 0 = the encoder refuses it
SWC_HD static inline int swc_fenc_rate_code(int rate) {
    switch (rate) {
        case 88200: return 1;
        case 176400: return 2;
        case 192000: return 3;
        case 8000: return 4;
        case 16000: return 5;
        case 22050: return 6;
        case 24000: return 7;
        case 32000: return 8;
        case 44100: return 9;
        case 48000: return 10;
        case 96000: return 11;
        default: return (rate >= 1 && rate <= SWC_FLAC_ENC_MAX_RATE_BITS) ? 13 : 0;
    }
}

// log2(BS / 256) for the five block sizes, -1 otherwise
SWC_HD static inline int swc_fenc_bs_log2(int blocksize) {
    for (int l = 0; l < 5; ++l)
        if (blocksize == (256 << l)) return l;
    return -1;
}

SWC_HD static inline uint32_t swc_fenc_crc8_byte(uint32_t c, uint32_t byte) {
    c ^= byte;
    for (int i = 0; i < 8; ++i) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    return c;
}

SWC_HD static inline uint32_t swc_fenc_crc16_byte(uint32_t c, uint32_t byte) {
    c ^= byte << 8;
    for (int i = 0; i < 8; ++i) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
    return c;
}

// a b mod P over GF(2), P = x^16 + x^15 + x^2 + 1 (the CRC-16 polynomial), a and b below 2^16
SWC_HD static inline uint32_t swc_fenc_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xFFFFu : (r << 1);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// x^(8 nbytes) mod P: with the CRC's initial value 0, crc(A | B) = crc(A) x^(8 |B|) + crc(B), so a thread's share of a
// frame's CRC-16 is the CRC of its chunk times this power for the bytes behind the chunk.  nbytes < 2^28.
SWC_HD static inline uint32_t swc_fenc_xpow8(uint32_t nbytes) {
    uint32_t r = 1, base = 0x100u;  // x^8
    for (int i = 0; i < 28 && (nbytes >> i) != 0u; ++i) {
        if ((nbytes >> i) & 1u) r = swc_fenc_mulmod(r, base);
        base = swc_fenc_mulmod(base, base);
    }
    return r;
}

// The header of frame `number` (< 2^26) holding bs samples of a stream with block size 256 << bs_log2: -> its length, CRC-8
// included (<= SWC_FLAC_ENC_MAX_HEADER), the bytes in t[0 .. length).
SWC_HD static inline int swc_fenc_frame_header(uint8_t* t, uint32_t number, int bs, int bs_log2, int rate, int rate_code) {
    int n = 0;
    const int bcode = bs == (256 << bs_log2) ? 8 + bs_log2 : (bs <= 256 ? 6 : 7);
    t[n++] = 0xFF;
    t[n++] = 0xF8;
    t[n++] = (uint8_t)((bcode << 4) | rate_code);
    t[n++] = 0x08;
    if (number < 0x80u) {
        t[n++] = (uint8_t)number;
    } else {
        const int nb = number < (1u << 11) ? 2 : number < (1u << 16) ? 3 : number < (1u << 21) ? 4 : 5;
        t[n++] = (uint8_t)(((0xFF00u >> nb) & 0xFFu) | (number >> (6 * (nb - 1))));
        for (int i = nb - 2; i >= 0; --i) t[n++] = (uint8_t)(0x80u | ((number >> (6 * i)) & 0x3Fu));
    }
    if (bcode == 6) {
        t[n++] = (uint8_t)(bs - 1);
    } else if (bcode == 7) {
        t[n++] = (uint8_t)((bs - 1) >> 8);
        t[n++] = (uint8_t)((bs - 1) & 0xFF);
    }
    if (rate_code == 13) {
        t[n++] = (uint8_t)(rate >> 8);
        t[n++] = (uint8_t)(rate & 0xFF);
    }
    uint32_t c = 0;
    for (int i = 0; i < n; ++i) c = swc_fenc_crc8_byte(c, t[i]);
    t[n++] = (uint8_t)c;
    return n;
}

// "fLaC" + STREAMINFO: SWC_FLAC_ENC_STREAM_HEADER bytes
SWC_HD static inline void swc_fenc_stream_header(uint8_t* h, int blocksize, uint32_t min_frame, uint32_t max_frame, int rate,
                                                 uint64_t n, const uint8_t* md5) {
    h[0] = 'f'; h[1] = 'L'; h[2] = 'a'; h[3] = 'C';
    h[4] = 0x80; h[5] = 0; h[6] = 0; h[7] = 34;
    h[8] = (uint8_t)(blocksize >> 8); h[9] = (uint8_t)blocksize;
    h[10] = h[8]; h[11] = h[9];
    h[12] = (uint8_t)(min_frame >> 16); h[13] = (uint8_t)(min_frame >> 8); h[14] = (uint8_t)min_frame;
    h[15] = (uint8_t)(max_frame >> 16); h[16] = (uint8_t)(max_frame >> 8); h[17] = (uint8_t)max_frame;
    // 20 bits rate, 3 bits channels - 1 = 0, 5 bits width - 1 = 15, 36 bits n
    const uint64_t w = ((uint64_t)(uint32_t)rate << 44) | ((uint64_t)15 << 36) | (n & (((uint64_t)1 << 36) - 1));
    for (int i = 0; i < 8; ++i) h[18 + i] = (uint8_t)(w >> (56 - 8 * i));
    for (int i = 0; i < 16; ++i) h[26 + i] = md5 ? md5[i] : (uint8_t)0;
}

// MD5 (RFC 1321): one 64-byte block, w[16] its little-endian words
SWC_HD static inline uint32_t swc_fenc_rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

#define SWC_FENC_MD5_STEP(f, a, b, c, d, x, s, k) a = b + swc_fenc_rotl(a + f(b, c, d) + (x) + (k), s)
#define SWC_FENC_F(x, y, z) (((x) & (y)) | (~(x) & (z)))
#define SWC_FENC_G(x, y, z) (((x) & (z)) | ((y) & ~(z)))
#define SWC_FENC_H(x, y, z) ((x) ^ (y) ^ (z))
#define SWC_FENC_I(x, y, z) ((y) ^ ((x) | ~(z)))

SWC_HD static inline void swc_fenc_md5_block(uint32_t st[4], const uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
    SWC_FENC_MD5_STEP(SWC_FENC_F, a, b, c, d, w[0], 7, 0xd76aa478u);  SWC_FENC_MD5_STEP(SWC_FENC_F, d, a, b, c, w[1], 12, 0xe8c7b756u);
    SWC_FENC_MD5_STEP(SWC_FENC_F, c, d, a, b, w[2], 17, 0x242070dbu); SWC_FENC_MD5_STEP(SWC_FENC_F, b, c, d, a, w[3], 22, 0xc1bdceeeu);
    SWC_FENC_MD5_STEP(SWC_FENC_F, a, b, c, d, w[4], 7, 0xf57c0fafu);  SWC_FENC_MD5_STEP(SWC_FENC_F, d, a, b, c, w[5], 12, 0x4787c62au);
    SWC_FENC_MD5_STEP(SWC_FENC_F, c, d, a, b, w[6], 17, 0xa8304613u); SWC_FENC_MD5_STEP(SWC_FENC_F, b, c, d, a, w[7], 22, 0xfd469501u);
    SWC_FENC_MD5_STEP(SWC_FENC_F, a, b, c, d, w[8], 7, 0x698098d8u);  SWC_FENC_MD5_STEP(SWC_FENC_F, d, a, b, c, w[9], 12, 0x8b44f7afu);
    SWC_FENC_MD5_STEP(SWC_FENC_F, c, d, a, b, w[10], 17, 0xffff5bb1u); SWC_FENC_MD5_STEP(SWC_FENC_F, b, c, d, a, w[11], 22, 0x895cd7beu);
    SWC_FENC_MD5_STEP(SWC_FENC_F, a, b, c, d, w[12], 7, 0x6b901122u); SWC_FENC_MD5_STEP(SWC_FENC_F, d, a, b, c, w[13], 12, 0xfd987193u);
    SWC_FENC_MD5_STEP(SWC_FENC_F, c, d, a, b, w[14], 17, 0xa679438eu); SWC_FENC_MD5_STEP(SWC_FENC_F, b, c, d, a, w[15], 22, 0x49b40821u);
    SWC_FENC_MD5_STEP(SWC_FENC_G, a, b, c, d, w[1], 5, 0xf61e2562u);  SWC_FENC_MD5_STEP(SWC_FENC_G, d, a, b, c, w[6], 9, 0xc040b340u);
    SWC_FENC_MD5_STEP(SWC_FENC_G, c, d, a, b, w[11], 14, 0x265e5a51u); SWC_FENC_MD5_STEP(SWC_FENC_G, b, c, d, a, w[0], 20, 0xe9b6c7aau);
    SWC_FENC_MD5_STEP(SWC_FENC_G, a, b, c, d, w[5], 5, 0xd62f105du);  SWC_FENC_MD5_STEP(SWC_FENC_G, d, a, b, c, w[10], 9, 0x02441453u);
    SWC_FENC_MD5_STEP(SWC_FENC_G, c, d, a, b, w[15], 14, 0xd8a1e681u); SWC_FENC_MD5_STEP(SWC_FENC_G, b, c, d, a, w[4], 20, 0xe7d3fbc8u);
    SWC_FENC_MD5_STEP(SWC_FENC_G, a, b, c, d, w[9], 5, 0x21e1cde6u);  SWC_FENC_MD5_STEP(SWC_FENC_G, d, a, b, c, w[14], 9, 0xc33707d6u);
    SWC_FENC_MD5_STEP(SWC_FENC_G, c, d, a, b, w[3], 14, 0xf4d50d87u); SWC_FENC_MD5_STEP(SWC_FENC_G, b, c, d, a, w[8], 20, 0x455a14edu);
    SWC_FENC_MD5_STEP(SWC_FENC_G, a, b, c, d, w[13], 5, 0xa9e3e905u); SWC_FENC_MD5_STEP(SWC_FENC_G, d, a, b, c, w[2], 9, 0xfcefa3f8u);
    SWC_FENC_MD5_STEP(SWC_FENC_G, c, d, a, b, w[7], 14, 0x676f02d9u); SWC_FENC_MD5_STEP(SWC_FENC_G, b, c, d, a, w[12], 20, 0x8d2a4c8au);
    SWC_FENC_MD5_STEP(SWC_FENC_H, a, b, c, d, w[5], 4, 0xfffa3942u);  SWC_FENC_MD5_STEP(SWC_FENC_H, d, a, b, c, w[8], 11, 0x8771f681u);
    SWC_FENC_MD5_STEP(SWC_FENC_H, c, d, a, b, w[11], 16, 0x6d9d6122u); SWC_FENC_MD5_STEP(SWC_FENC_H, b, c, d, a, w[14], 23, 0xfde5380cu);
    SWC_FENC_MD5_STEP(SWC_FENC_H, a, b, c, d, w[1], 4, 0xa4beea44u);  SWC_FENC_MD5_STEP(SWC_FENC_H, d, a, b, c, w[4], 11, 0x4bdecfa9u);
    SWC_FENC_MD5_STEP(SWC_FENC_H, c, d, a, b, w[7], 16, 0xf6bb4b60u); SWC_FENC_MD5_STEP(SWC_FENC_H, b, c, d, a, w[10], 23, 0xbebfbc70u);
    SWC_FENC_MD5_STEP(SWC_FENC_H, a, b, c, d, w[13], 4, 0x289b7ec6u); SWC_FENC_MD5_STEP(SWC_FENC_H, d, a, b, c, w[0], 11, 0xeaa127fau);
    SWC_FENC_MD5_STEP(SWC_FENC_H, c, d, a, b, w[3], 16, 0xd4ef3085u); SWC_FENC_MD5_STEP(SWC_FENC_H, b, c, d, a, w[6], 23, 0x04881d05u);
    SWC_FENC_MD5_STEP(SWC_FENC_H, a, b, c, d, w[9], 4, 0xd9d4d039u);  SWC_FENC_MD5_STEP(SWC_FENC_H, d, a, b, c, w[12], 11, 0xe6db99e5u);
    SWC_FENC_MD5_STEP(SWC_FENC_H, c, d, a, b, w[15], 16, 0x1fa27cf8u); SWC_FENC_MD5_STEP(SWC_FENC_H, b, c, d, a, w[2], 23, 0xc4ac5665u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, a, b, c, d, w[0], 6, 0xf4292244u);  SWC_FENC_MD5_STEP(SWC_FENC_I, d, a, b, c, w[7], 10, 0x432aff97u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, c, d, a, b, w[14], 15, 0xab9423a7u); SWC_FENC_MD5_STEP(SWC_FENC_I, b, c, d, a, w[5], 21, 0xfc93a039u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, a, b, c, d, w[12], 6, 0x655b59c3u); SWC_FENC_MD5_STEP(SWC_FENC_I, d, a, b, c, w[3], 10, 0x8f0ccc92u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, c, d, a, b, w[10], 15, 0xffeff47du); SWC_FENC_MD5_STEP(SWC_FENC_I, b, c, d, a, w[1], 21, 0x85845dd1u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, a, b, c, d, w[8], 6, 0x6fa87e4fu);  SWC_FENC_MD5_STEP(SWC_FENC_I, d, a, b, c, w[15], 10, 0xfe2ce6e0u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, c, d, a, b, w[6], 15, 0xa3014314u); SWC_FENC_MD5_STEP(SWC_FENC_I, b, c, d, a, w[13], 21, 0x4e0811a1u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, a, b, c, d, w[4], 6, 0xf7537e82u);  SWC_FENC_MD5_STEP(SWC_FENC_I, d, a, b, c, w[11], 10, 0xbd3af235u);
    SWC_FENC_MD5_STEP(SWC_FENC_I, c, d, a, b, w[2], 15, 0x2ad7d2bbu); SWC_FENC_MD5_STEP(SWC_FENC_I, b, c, d, a, w[9], 21, 0xeb86d391u);
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}

// The MD5 of n int16 samples as they lie in memory (little endian), s 2-byte aligned: -> 16 digest bytes.  Word j of the
// message is samples 2j and 2j + 1; the 0x80 pad byte, the zeros and the 64-bit bit count follow (RFC 1321 3.1 - 3.2).
// (Loading block b + 1 before block b is hashed was measured and bought nothing: a block costs 0.9 us of 64 dependent
// steps, not of waiting for its samples.)
SWC_HD static inline void swc_fenc_md5_i16(const uint16_t* s, int64_t n, uint8_t dig[16]) {
    uint32_t st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    uint32_t w[16];
    const int64_t words = n >> 1;          // whole message words
    const int64_t blocks = words >> 4;     // whole 64-byte blocks
    for (int64_t b = 0; b < blocks; ++b) {
        for (int j = 0; j < 16; ++j) w[j] = (uint32_t)s[32 * b + 2 * j] | ((uint32_t)s[32 * b + 2 * j + 1] << 16);
        swc_fenc_md5_block(st, w);
    }
    // the tail: words [16 blocks, words), perhaps half a word, the pad byte; the length goes into the last two words of this
    // block when the tail ends at or before byte 56, else into a block of its own
    const int tw = (int)(words - 16 * blocks);  // 0 .. 15
    for (int j = 0; j < 16; ++j) {
        uint32_t v = 0;
        if (j < tw) v = (uint32_t)s[32 * blocks + 2 * j] | ((uint32_t)s[32 * blocks + 2 * j + 1] << 16);
        else if (j == tw) v = (n & 1) ? ((uint32_t)s[n - 1] | 0x800000u) : 0x80u;
        w[j] = v;
    }
    const uint64_t bits = (uint64_t)n * 16u;
    if (tw >= 14) {  // the pad byte lies at or behind byte 56: no room for the length
        swc_fenc_md5_block(st, w);
        for (int j = 0; j < 14; ++j) w[j] = 0;
    }
    w[14] = (uint32_t)bits;
    w[15] = (uint32_t)(bits >> 32);
    swc_fenc_md5_block(st, w);
    for (int i = 0; i < 16; ++i) dig[i] = (uint8_t)(st[i >> 2] >> (8 * (i & 3)));
}

#endif /* SWC_FLAC_ENC_BITS_H_ */
