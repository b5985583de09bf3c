// swc_entropy_check: a stand-alone host program over csrc/swc_entropy_model.h — the coder, model, CRC and parser lines the
// kernels of swc_entropy.hip and swc_entropy_parse run — meant to be compiled with -fsanitize=address,undefined.  No GPU code.
//
//   swc_entropy_check                          the self test: round trips, the renormalisation bound, CRC combination, and
//                                              swc_ent_parse fed truncated, lying and bit-flipped images (exit status 0 = pass)
//   swc_entropy_check encode L0 L1 L2 L3 G T   G T codes (decimal, row by row) on stdin -> the image in hex on stdout
//   swc_entropy_check decode                   an image in hex on stdin -> "T G L0 L1 L2 L3", the modes, then the codes row by row
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "swc_entropy_model.h"

typedef std::vector<unsigned char> bytes_t;

static void put32(bytes_t& v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((unsigned char)(x >> (8 * k)));
}

// the contract's encoder, serially: rows[g][t]
static bytes_t encode_image(const std::vector<std::vector<int64_t>>& rows, const swc_ent_levels& lv, int* most) {
    const int G = (int)rows.size();
    const uint32_t T = (uint32_t)rows[0].size();
    std::vector<bytes_t> streams(G);
    std::vector<int> modes(G, 0);
    for (int g = 0; g < G; ++g) {
        bool valid = true;
        std::vector<uint32_t> c(T);
        for (uint32_t t = 0; t < T; ++t) {
            valid = valid && rows[g][t] >= 0 && rows[g][t] < lv.n_codes;
            c[t] = (uint32_t)rows[g][t];
        }
        bytes_t best((size_t)swc_ent_raw_bytes(T, lv.w));
        for (size_t k = 0; k < best.size(); ++k)
            best[k] = (unsigned char)swc_ent_raw_byte((uint32_t)k, T, lv.w, [&](uint32_t t) { return c[t]; });
        if (valid && T > 0)
            for (int order = 0; order < 2; ++order) {
                bytes_t s;
                swc_ent_encode_stream(c.data(), T, lv, order, [&](unsigned char b) { s.push_back(b); }, most);
                if (s.size() < best.size()) best = s, modes[g] = order + 1;
            }
        streams[g] = best;
    }
    uint32_t body = 4u * G;
    for (int g = 0; g < G; ++g) body += (uint32_t)streams[g].size();
    bytes_t im;
    for (int q = 0; q < SWC_ENTROPY_HEADER_BYTES; ++q) im.push_back((unsigned char)swc_ent_header_byte(q, T, G, lv, body));
    for (int g = 0; g < G; ++g) put32(im, ((uint32_t)modes[g] << 24) | (uint32_t)streams[g].size());
    for (int g = 0; g < G; ++g) im.insert(im.end(), streams[g].begin(), streams[g].end());
    const uint32_t crc = swc_ent_crc_image(im.data(), body);
    for (int k = 0; k < 4; ++k) im[20 + k] = (unsigned char)(crc >> (8 * k));
    return im;
}

static int decode_image(const bytes_t& im, std::vector<std::vector<uint32_t>>& rows, int32_t* T, int32_t* G, int32_t* L, int32_t* mode) {
    int64_t off[8], len[8];
    // an exact-size copy: a read behind the image is a read behind the allocation
    unsigned char* copy = (unsigned char*)malloc(im.size() ? im.size() : 1);
    if (!im.empty()) memcpy(copy, im.data(), im.size());
    const int rc = swc_ent_parse(copy, (int64_t)im.size(), 1, T, G, L, off, len, mode);
    if (rc == 0) {
        swc_ent_levels lv;
        swc_ent_levels_init(lv, L[0], L[1], L[2], L[3]);
        rows.assign(*G, std::vector<uint32_t>(*T));
        for (int g = 0; g < *G; ++g) {
            if (mode[g] == 0)
                for (int t = 0; t < *T; ++t) rows[g][t] = swc_ent_raw_value(copy + off[g], len[g], (uint32_t)t, lv.w);
            else
                swc_ent_decode_stream(copy + off[g], len[g], *T, lv, mode[g] - 1, rows[g].data());
        }
    }
    free(copy);
    return rc;
}

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u, rng_state >> 8; }

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "swc_entropy_check: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int self_test() {
    // CRC: the check value of the standard, and combination against the serial form at every split
    {
        const unsigned char msg[] = "123456789";
        uint32_t st = 0xffffffffu;
        for (int k = 0; k < 9; ++k) st = swc_ent_crc_byte(st, msg[k]);
        REQUIRE(~st == 0xcbf43926u);
        for (int cut = 0; cut <= 9; ++cut) {
            uint32_t a = 0xffffffffu, b = 0xffffffffu;
            for (int k = 0; k < cut; ++k) a = swc_ent_crc_byte(a, msg[k]);
            for (int k = cut; k < 9; ++k) b = swc_ent_crc_byte(b, msg[k]);
            REQUIRE(swc_ent_crc_combine(~a, ~b, (uint32_t)(9 - cut)) == 0xcbf43926u);
        }
        REQUIRE(swc_ent_xpow8(0) == 1u << 31 && swc_ent_xpow8(1) == 1u << 23);
    }
    const int sets[4][4] = {{8, 7, 6, 6}, {2, 2, 2, 2}, {16, 16, 8, 8}, {16, 16, 16, 4}};
    const int lengths[] = {0, 1, 2, 3, 37, 125, 400, 1500};
    int most = 0;
    for (const auto& L : sets) {
        swc_ent_levels lv;
        REQUIRE(swc_ent_levels_init(lv, L[0], L[1], L[2], L[3]) == 0);
        for (int T : lengths)
            for (int kind = 0; kind < 3; ++kind) {  // constant, sticky, uniform
                std::vector<std::vector<int64_t>> rows(3, std::vector<int64_t>(T));
                for (auto& r : rows) {
                    int64_t c = rnd() % lv.n_codes;
                    for (int t = 0; t < T; ++t) {
                        if (kind == 2 || (kind == 1 && rnd() % 5 == 0)) c = rnd() % lv.n_codes;
                        r[t] = c;
                    }
                }
                const bytes_t im = encode_image(rows, lv, &most);
                std::vector<std::vector<uint32_t>> back;
                int32_t t2, g2, l2[4], mode[8];
                REQUIRE(decode_image(im, back, &t2, &g2, l2, mode) == 0 && t2 == T && g2 == 3);
                for (int g = 0; g < 3; ++g)
                    for (int t = 0; t < T; ++t) REQUIRE(back[g][t] == (uint32_t)rows[g][t]);
                // any bytes decode to valid codes: the adaptive decoder over noise
                if (T) {
                    bytes_t junk((size_t)(rnd() % 64));
                    for (auto& b : junk) b = (unsigned char)rnd();
                    std::vector<uint32_t> out(T);
                    unsigned char* exact = (unsigned char*)malloc(junk.size() ? junk.size() : 1);
                    if (!junk.empty()) memcpy(exact, junk.data(), junk.size());
                    swc_ent_decode_stream(exact, (int64_t)junk.size(), T, lv, kind & 1, out.data());
                    free(exact);
                    for (int t = 0; t < T; ++t) REQUIRE(out[t] < (uint32_t)lv.n_codes);
                }
                if (T == 37 || T == 0) {  // the parser against damage
                    std::vector<std::vector<uint32_t>> none;
                    for (size_t cut = 0; cut < im.size(); ++cut)
                        REQUIRE(decode_image(bytes_t(im.begin(), im.begin() + cut), none, &t2, &g2, l2, mode) < 0);
                    for (size_t bit = 0; bit < 8 * im.size(); ++bit) {
                        bytes_t f = im;
                        f[bit >> 3] ^= (unsigned char)(1u << (bit & 7));
                        REQUIRE(decode_image(f, none, &t2, &g2, l2, mode) < 0);
                    }
                    bytes_t lie = im;
                    lie[9] = 1;
                    REQUIRE(decode_image(lie, none, &t2, &g2, l2, mode) == SWC_ENTROPY_E_VERSION);
                    lie = im, lie[10] = 17;
                    REQUIRE(decode_image(lie, none, &t2, &g2, l2, mode) == SWC_ENTROPY_E_LIMITS);
                    lie = im, lie[8] = 9;
                    REQUIRE(decode_image(lie, none, &t2, &g2, l2, mode) == SWC_ENTROPY_E_LIMITS);
                    lie = im, lie[0] = 'X';
                    REQUIRE(decode_image(lie, none, &t2, &g2, l2, mode) == SWC_ENTROPY_E_MAGIC);
                    lie = im, lie[16] ^= 1;  // body_bytes off by one: truncated, or a table that does not sum to it
                    const int rc = decode_image(lie, none, &t2, &g2, l2, mode);
                    REQUIRE(rc == SWC_ENTROPY_E_TRUNCATED || rc == SWC_ENTROPY_E_TABLE);
                    lie = im, lie.push_back(0), lie[16] += 1;
                    REQUIRE(decode_image(lie, none, &t2, &g2, l2, mode) == SWC_ENTROPY_E_TABLE);
                    lie = im, lie[7] = 0xff;  // T far above the limit
                    REQUIRE(decode_image(lie, none, &t2, &g2, l2, mode) == SWC_ENTROPY_E_LIMITS);
                }
            }
    }
    REQUIRE(most <= SWC_ENTROPY_MAX_RENORM);
    printf("swc_entropy_check: ok (most renormalisation turns per symbol: %d)\n", most);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_test();
    if (argc == 8 && strcmp(argv[1], "encode") == 0) {
        swc_ent_levels lv;
        const int G = atoi(argv[6]), T = atoi(argv[7]);
        if (swc_ent_levels_init(lv, atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])) != 0 || G < 1 || G > 8 || T < 0 ||
            T > SWC_ENTROPY_MAX_FRAMES)
            return 2;
        std::vector<std::vector<int64_t>> rows(G, std::vector<int64_t>(T));
        for (auto& r : rows)
            for (auto& c : r) {
                long long v;
                if (scanf("%lld", &v) != 1) return 2;
                c = v;
            }
        for (unsigned char b : encode_image(rows, lv, nullptr)) printf("%02x", b);
        printf("\n");
        return 0;
    }
    if (argc == 2 && strcmp(argv[1], "decode") == 0) {
        bytes_t im;
        unsigned v;
        while (scanf("%2x", &v) == 1) im.push_back((unsigned char)v);
        std::vector<std::vector<uint32_t>> rows;
        int32_t T, G, L[4], mode[8];
        const int rc = decode_image(im, rows, &T, &G, L, mode);
        if (rc != 0) {
            printf("refused %d\n", rc);
            return 3;
        }
        printf("%d %d %d %d %d %d\n", T, G, L[0], L[1], L[2], L[3]);
        for (int g = 0; g < G; ++g) printf("%d%c", mode[g], g + 1 < G ? ' ' : '\n');
        for (auto& r : rows) {
            for (uint32_t c : r) printf("%u ", c);
            printf("\n");
        }
        return 0;
    }
    fprintf(stderr, "usage: swc_entropy_check [encode L0 L1 L2 L3 G T | decode]\n");
    return 2;
}
