// swc_flac_check — the shared frame decoder (csrc/swc_flac_frame.h, the text the GPU kernel runs) on the host, stand-alone.
//
//   swc_flac_check [--dump DIR] FILE.flac ...
//
// Every file is indexed by swc_flac_index, every frame is copied into a heap block of exactly its size and decoded into
// planes of exactly channels x blocksize int32, the stereo decorrelation is undone, and the result is compared with
// swc_flac_decode (the host decoder).  Built with -fsanitize=address,undefined (build.build_flac_check) any read outside a
// frame or store outside a plane ends the program with a report.  One line per file:
//
//   <file> index=<frames or -code> host=<samples or -code> status=<s0,s1,...> verdict=<equal|status|refused|MISMATCH>
//
// equal: all statuses 0 and the samples are the host decoder's, bit for bit.  status: at least one frame has a non-zero
// status.  refused: the index turned the stream away.  MISMATCH (exit 1): statuses all 0 but the host decoder failed or gave
// other samples.  --dump DIR writes <DIR>/<basename>.i32, the decoded interleaved int32 samples, for files with verdict equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "swc_flac.h"
#include "swc_flac_frame.h"

extern "C" int64_t swc_flac_decode(const uint8_t* data, size_t n, int32_t* out, int64_t cap, int32_t* md5_state);

static bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    const char* dump = nullptr;
    int first = 1;
    if (argc >= 3 && !strcmp(argv[1], "--dump")) { dump = argv[2]; first = 3; }
    const int64_t ceiling = 1 << 24;  // samples per channel: test streams are short
    int mismatches = 0;
    for (int a = first; a < argc; ++a) {
        std::vector<uint8_t> data;
        if (!read_file(argv[a], data)) { fprintf(stderr, "%s: cannot be read\n", argv[a]); return 2; }
        swc_flac_stream info;
        int64_t nf = swc_flac_index(data.data(), data.size(), ceiling, &info, nullptr, 0);
        if (nf < 0) { printf("%s index=%ld host=- status= verdict=refused\n", argv[a], (long)nf); continue; }
        std::vector<swc_flac_frame> frames((size_t)nf);
        if (swc_flac_index(data.data(), data.size(), ceiling, &info, frames.data(), nf) != nf) { fprintf(stderr, "%s: index not repeatable\n", argv[a]); return 2; }
        const int ch = info.channels;
        std::vector<int32_t> got((size_t)(info.total * ch));
        std::string st;
        bool all_ok = true;
        for (int64_t k = 0; k < nf; ++k) {
            const swc_flac_frame& fr = frames[(size_t)k];
            // exactly the frame's bytes and exactly the frame's planes, each in a heap block of its own
            uint8_t* fb = (uint8_t*)malloc((size_t)fr.n_bytes);
            int32_t* planes = (int32_t*)malloc(sizeof(int32_t) * (size_t)fr.blocksize * (size_t)ch);
            int32_t* coef = (int32_t*)malloc(sizeof(int32_t) * 32);
            memcpy(fb, data.data() + fr.byte_off, (size_t)fr.n_bytes);
            memset(planes, 0x5A, sizeof(int32_t) * (size_t)fr.blocksize * (size_t)ch);
            const int s = swc_flac_decode_frame(fb, fr.n_bytes, fr.hdr_bytes, fr.blocksize, ch, info.bps, fr.chan_assign, planes,
                                                fr.blocksize, coef, 1);
            st += (k ? "," : "") + std::to_string(s);
            if (s == SWC_FLAC_ST_OK) {
                for (int i = 0; i < fr.blocksize; ++i)
                    for (int c = 0; c < ch; ++c)
                        got[(size_t)((fr.first_sample + i) * ch + c)] =
                            fr.chan_assign >= 8 ? swc_flac_undo_stereo(planes[i], planes[fr.blocksize + i], fr.chan_assign, c)
                                                : planes[(size_t)c * fr.blocksize + i];
            } else {
                all_ok = false;
            }
            free(fb); free(planes); free(coef);
        }
        std::vector<int32_t> want((size_t)(info.total * ch) + 1);
        int32_t md5 = 0;
        const int64_t hn = swc_flac_decode(data.data(), data.size(), want.data(), info.total, &md5);
        const char* verdict = "status";
        if (all_ok) {
            const bool same = hn == info.total && (info.total == 0 || !memcmp(want.data(), got.data(), sizeof(int32_t) * got.size()));
            verdict = same ? "equal" : "MISMATCH";
            mismatches += !same;
            if (same && dump) {
                std::string base = argv[a];
                const size_t slash = base.find_last_of('/');
                if (slash != std::string::npos) base = base.substr(slash + 1);
                const std::string out = std::string(dump) + "/" + base + ".i32";
                FILE* f = fopen(out.c_str(), "wb");
                if (!f) { fprintf(stderr, "%s: cannot be written\n", out.c_str()); return 2; }
                if (!got.empty()) fwrite(got.data(), sizeof(int32_t), got.size(), f);
                fclose(f);
            }
        }
        printf("%s index=%ld host=%ld status=%s verdict=%s\n", argv[a], (long)nf, (long)hn, st.c_str(), verdict);
    }
    return mismatches ? 1 : 0;
}
