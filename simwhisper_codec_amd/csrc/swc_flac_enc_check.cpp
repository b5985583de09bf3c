// swc_flac_enc_check — a stand-alone host program (its own main) over csrc/swc_flac_enc_bits.h, the serial pieces the FLAC
// encoder's kernels run (csrc/swc_flac_enc.hip): built with -fsanitize=address,undefined by build.build_flac_enc_check and run
// by tests/test_flac_enc_cpu.py, which compares every line printed here with hashlib and the numpy reference.  No GPU code.
//
//   swc_flac_enc_check md5 N...            MD5 of N samples s[i] = (7919 i + 13) mod 2^16, from a heap block of exactly 2 N bytes
//   swc_flac_enc_check crc N...            CRC-16 of N bytes b[i] = (31 i + 7) mod 256: one pass, and as 256 threads share it
//   swc_flac_enc_check hdr K BS LOG2 RATE  the header of frame K holding BS samples of a stream with block size 256 << LOG2
//   swc_flac_enc_check info BS MIN MAX RATE N   the 42 stream header bytes, MD5 bytes 0 .. 15
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "swc_flac_enc_bits.h"

static void hex(const uint8_t* p, int n) {
    for (int i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "md5")) {
        for (int a = 2; a < argc; ++a) {
            const long n = atol(argv[a]);
            uint16_t* s = (uint16_t*)malloc(2 * (size_t)n);  // exactly the samples: a read behind them is reported
            for (long i = 0; i < n; ++i) s[i] = (uint16_t)(7919 * i + 13);
            uint8_t d[16];
            swc_fenc_md5_i16(s, n, d);
            hex(d, 16);
            free(s);
        }
    } else if (!strcmp(argv[1], "crc")) {
        for (int a = 2; a < argc; ++a) {
            const int nb = atoi(argv[a]);
            uint8_t* b = (uint8_t*)malloc((size_t)nb);
            for (int i = 0; i < nb; ++i) b[i] = (uint8_t)(31 * i + 7);
            uint32_t whole = 0;
            for (int i = 0; i < nb; ++i) whole = swc_fenc_crc16_byte(whole, b[i]);
            const int CH = (((nb + 255) / 256) + 3) & ~3;  // the frame kernel's split
            uint32_t shared = 0;
            for (int t = 0; t < 256; ++t) {
                const int c0 = t * CH, c1 = c0 + CH < nb ? c0 + CH : nb;
                uint32_t c = 0;
                for (int i = c0; i < c1; ++i) c = swc_fenc_crc16_byte(c, b[i]);
                if (c0 < nb) shared ^= swc_fenc_mulmod(c, swc_fenc_xpow8((uint32_t)(nb - c1)));
            }
            printf("%04x %04x\n", whole, shared);
            free(b);
        }
    } else if (!strcmp(argv[1], "hdr") && argc == 6) {
        uint8_t* h = (uint8_t*)malloc(SWC_FLAC_ENC_MAX_HEADER);
        const int rate = atoi(argv[5]);
        const int n = swc_fenc_frame_header(h, (uint32_t)atol(argv[2]), atoi(argv[3]), atoi(argv[4]), rate, swc_fenc_rate_code(rate));
        hex(h, n);
        free(h);
    } else if (!strcmp(argv[1], "info") && argc == 7) {
        uint8_t* h = (uint8_t*)malloc(SWC_FLAC_ENC_STREAM_HEADER);
        uint8_t m[16];
        for (int i = 0; i < 16; ++i) m[i] = (uint8_t)i;
        swc_fenc_stream_header(h, atoi(argv[2]), (uint32_t)atol(argv[3]), (uint32_t)atol(argv[4]), atoi(argv[5]), (uint64_t)atoll(argv[6]), m);
        hex(h, SWC_FLAC_ENC_STREAM_HEADER);
        free(h);
    } else {
        return 2;
    }
    return 0;
}
