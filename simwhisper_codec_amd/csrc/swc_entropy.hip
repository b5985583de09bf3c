// SWC2 on the device (include/swc_entropy.h): a ragged batch of utterances <-> their entropy-coded, checksummed images.
//
// The adaptive coder is serial in its symbols, so what is parallel is the batch: ONE WAVE per (utterance, group, order) stream,
// 2 G B waves per encode call.  Inside a wave the lanes do what is parallel in a symbol step:
//   - codes are read in coalesced chunks of 64 frames and split into their four levels by the lanes (the divisions by L_d);
//   - the four dimensions of a frame use four independent rows, so lane 16 d + s holds count s of dimension d's current row:
//     one 16-lane segmented scan (four DPP row shifts) gives cum and tot of all four symbols of the frame, the count update is
//     one lane-local operation, and the decoder finds its symbol by a ballot on cum <= v;
//   - the count rows live in LDS, entry [d][row][s] only ever touched by lane 16 d + s (no barrier, no cross-lane LDS traffic);
//   - low, range (and the decoder's code word) are wave-uniform and follow csrc/swc_entropy_model.h line by line.
// Output bytes collect in a uniform dword and leave as aligned dword stores of lane 0 into the stream's workspace slot.
// Every loop's trip count is a function of T, G and the levels (the renormalisation loop: at most SWC_ENTROPY_MAX_RENORM turns).
#include "swc_common.h"
#include "swc_entropy.h"
#include "swc_entropy_model.h"

namespace {

constexpr int ENT_WAVE = 64;
constexpr int ENT_THREADS = 256;  // layout, gather, crc
constexpr int ENT_NOLEN = 0x7fffffff;

__device__ __forceinline__ uint32_t lane_read(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

// inclusive sum over each 16-lane segment: four DPP row shifts (a row is 16 lanes; a lane shifted in from outside the row reads 0)
__device__ __forceinline__ uint32_t seg16_scan(uint32_t x) {
    int incl = (int)x;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, true);  // row_shr:1
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, true);  // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, true);  // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, true);  // row_shr:8
    return (uint32_t)incl;
}

// the sum of this lane's dimension out of the four (wave-uniform) sums
__device__ __forceinline__ uint32_t pick4(int d, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
    return d == 0 ? t0 : (d == 1 ? t1 : (d == 2 ? t2 : t3));
}

// this lane's count entries start at 1 (a symbol of its dimension) or 0 (a lane past L_d: it never becomes a symbol)
__device__ __forceinline__ void counts_init(uint32_t* cnt, const swc_ent_levels& lv, int myd, int mys) {
    const int myL = myd == 0 ? lv.L[0] : (myd == 1 ? lv.L[1] : (myd == 2 ? lv.L[2] : lv.L[3]));
    const uint32_t one = mys < myL ? 1u : 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) cnt[((myd * 16 + r) << 4) + mys] = one;
}

inline int64_t slot_bytes_of(int64_t max_frames, int w) { return (swc_ent_raw_bytes(max_frames, w) + 3) & ~(int64_t)3; }
inline int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// ------------------------------------------------------------------------------------------------ the adaptive streams
template <typename E>
__global__ __launch_bounds__(ENT_WAVE) void ent_code_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ ldgs,
                                                            const int64_t* __restrict__ n_frames, swc_ent_levels lv, int G,
                                                            int max_frames, int* __restrict__ lens,
                                                            unsigned char* __restrict__ slots, long slot_bytes,
                                                            int* __restrict__ bad) {
    __shared__ uint32_t cnt[4 * 16 * 16];
    const int order = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x, myd = lane >> 4, mys = lane & 15;
    const long idx = ((long)b * G + g) * 2 + order;
    long Tl = n_frames[b];
    Tl = Tl < 0 ? 0 : (Tl > max_frames ? max_frames : Tl);
    const int T = (int)Tl;
    if (T == 0) {  // (uniform) the layout kernel does not read the lengths of an empty utterance
        if (lane == 0) lens[idx] = ENT_NOLEN;
        return;
    }
    const E* row = reinterpret_cast<const E*>(rows[b]) + (long)g * ldgs[b];
    uint32_t* slot = reinterpret_cast<uint32_t*>(slots + idx * slot_bytes);
    counts_init(cnt, lv, myd, mys);

    uint32_t low = 0, range = 0xffffffffu, acc = 0, prev = 0;
    int n = 0, nbad = 0;
    // byte n of the stream: into the dword, the dword out when it is full and lies inside the slot
    auto emit = [&](uint32_t byte) {
        acc |= byte << (8 * (n & 3));
        ++n;
        if ((n & 3) == 0) {
            if (lane == 0 && n <= slot_bytes) slot[(n >> 2) - 1] = acc;
            acc = 0;
        }
    };
    for (int t0 = 0; t0 < T; t0 += ENT_WAVE) {
        uint32_t packed = 0;
        if (t0 + lane < T) {
            const E c = row[t0 + lane];
            nbad += (c < 0 || c >= (E)lv.n_codes) ? 1 : 0;
            packed = swc_ent_split((uint32_t)c, lv);
        }
        const int nf = T - t0 < ENT_WAVE ? T - t0 : ENT_WAVE;
        for (int j = 0; j < nf; ++j) {
            const uint32_t cur = lane_read(packed, j);
            const uint32_t ctx = order ? (prev >> (4 * myd)) & 15u : 0u;
            uint32_t* p = &cnt[((myd * 16 + (int)ctx) << 4) + mys];
            uint32_t x = *p;
            const uint32_t incl = seg16_scan(x);
            const uint32_t excl = incl - x;
            const uint32_t tots[4] = {lane_read(incl, 15), lane_read(incl, 31), lane_read(incl, 47), lane_read(incl, 63)};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int src = d * 16 + (int)((cur >> (4 * d)) & 15u);
                swc_ent_narrow(low, range, lane_read(excl, src), lane_read(x, src), tots[d]);
                for (int k = 0; k < SWC_ENTROPY_MAX_RENORM; ++k) {
                    uint32_t byte = 0;
                    if (!swc_ent_renorm(low, range, byte)) break;
                    emit(byte);
                }
            }
            x = swc_ent_update(x, ((cur >> (4 * myd)) & 15u) == (uint32_t)mys, pick4(myd, tots[0], tots[1], tots[2], tots[3]));
            *p = x;
            prev = cur;
        }
    }
#pragma unroll
    for (int k = 3; k >= 0; --k) emit((low >> (8 * k)) & 0xffu);
    if ((n & 3) != 0 && lane == 0 && ((n + 3) & ~3) <= slot_bytes) slot[n >> 2] = acc;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nbad += __shfl_xor(nbad, off);
    if (lane == 0) {
        lens[idx] = nbad ? ENT_NOLEN : n;  // a stream with an invalid value is written raw
        if (order == 0 && nbad && bad != nullptr) atomicAdd(bad, nbad);
    }
}

// ------------------------------------------------------------------------------------------------ modes, sizes, offsets
__global__ __launch_bounds__(ENT_THREADS) void ent_layout_kernel(const int64_t* __restrict__ n_frames, const int* __restrict__ lens,
                                                                 uint32_t* __restrict__ table, int64_t* __restrict__ sizes,
                                                                 int64_t* __restrict__ byte_off, int B, int G, int w, int max_frames) {
    __shared__ long part[ENT_THREADS];
    const int tid = threadIdx.x;
    const int per = (B + ENT_THREADS - 1) / ENT_THREADS;
    const int b0 = tid * per < B ? tid * per : B, b1 = b0 + per < B ? b0 + per : B;
    long sum = 0;
    for (int b = b0; b < b1; ++b) {
        long Tl = n_frames[b];
        Tl = Tl < 0 ? 0 : (Tl > max_frames ? max_frames : Tl);
        const int raw = (int)swc_ent_raw_bytes(Tl, w);
        long size = SWC_ENTROPY_HEADER_BYTES + 4 * G;
        for (int g = 0; g < G; ++g) {
            int mode = 0, len = raw;
            if (Tl > 0) {
                const int l1 = lens[((long)b * G + g) * 2], l2 = lens[((long)b * G + g) * 2 + 1];
                if (l1 < len) mode = 1, len = l1;
                if (l2 < len) mode = 2, len = l2;
            }
            table[(long)b * G + g] = ((uint32_t)mode << 24) | (uint32_t)len;
            size += len;
        }
        sizes[b] = size;
        sum += size;
    }
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < ENT_THREADS; off <<= 1) {  // inclusive scan of the 256 partial sums
        const long y = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += y;
        __syncthreads();
    }
    long pos = part[tid] - sum;
    for (int b = b0; b < b1; ++b) {
        byte_off[b] = pos;
        pos += sizes[b];
    }
}

// ------------------------------------------------------------------------------------------------ the images
// A thread owns one 4-byte-ALIGNED dword of the output buffer; dwords wholly inside an image are one store, the others are
// written byte by byte, so back-to-back images never write the same byte and nothing outside an image is touched.
template <typename E>
__global__ __launch_bounds__(ENT_THREADS) void ent_gather_kernel(const void* const* __restrict__ rows, const int64_t* __restrict__ ldgs,
                                                                 const int64_t* __restrict__ n_frames, swc_ent_levels lv, int G,
                                                                 int max_frames, const uint32_t* __restrict__ table,
                                                                 const unsigned char* __restrict__ slots, long slot_bytes,
                                                                 const int64_t* __restrict__ sizes, const int64_t* __restrict__ byte_off,
                                                                 unsigned char* __restrict__ out, long out_bytes) {
    __shared__ uint32_t s_entry[SWC_ENTROPY_MAX_GROUPS];
    __shared__ long s_start[SWC_ENTROPY_MAX_GROUPS + 1];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        long pos = SWC_ENTROPY_HEADER_BYTES + 4 * G;
        for (int g = 0; g < SWC_ENTROPY_MAX_GROUPS; ++g) {
            const uint32_t e = g < G ? table[(long)b * G + g] : 0u;
            s_entry[g] = e;
            s_start[g] = pos;
            pos += e & 0xffffffu;
        }
        s_start[SWC_ENTROPY_MAX_GROUPS] = pos;
    }
    __syncthreads();
    long Tl = n_frames[b];
    Tl = Tl < 0 ? 0 : (Tl > max_frames ? max_frames : Tl);
    const uint32_t T = (uint32_t)Tl;
    const long size = sizes[b], off = byte_off[b];
    if (off < 0 || off > out_bytes - size) return;  // (cannot happen with the checked out_bytes)
    const long lead = (long)((reinterpret_cast<uintptr_t>(out) + (uintptr_t)off) & 3u);
    const long p = 4L * ((long)blockIdx.x * ENT_THREADS + threadIdx.x) - lead;
    if (p >= size) return;
    const E* row0 = T ? reinterpret_cast<const E*>(rows[b]) : nullptr;
    const long ldg = ldgs[b];
    auto image_byte = [&](long q) -> uint32_t {
        if (q < SWC_ENTROPY_HEADER_BYTES) return swc_ent_header_byte((int)q, T, G, lv, (uint32_t)(size - SWC_ENTROPY_HEADER_BYTES));
        if (q < SWC_ENTROPY_HEADER_BYTES + 4 * G) {
            const long k = q - SWC_ENTROPY_HEADER_BYTES;
            return (s_entry[k >> 2] >> (8 * (int)(k & 3))) & 0xffu;
        }
        int g = 0;
        for (int k = 1; k < SWC_ENTROPY_MAX_GROUPS; ++k) g += q >= s_start[k] ? 1 : 0;  // (empty streams share a start: the last wins)
        const long k = q - s_start[g];
        const int mode = (int)(s_entry[g] >> 24);
        if (mode == 0) {
            const E* row = row0 + (long)g * ldg;
            return swc_ent_raw_byte((uint32_t)k, T, lv.w, [&](uint32_t t) { return (uint32_t)row[t]; });
        }
        return slots[(((long)b * G + g) * 2 + (mode - 1)) * slot_bytes + k];
    };
    unsigned char* dst = out + off + p;
    if (p >= 0 && p + 4 <= size) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= image_byte(p + k) << (8 * k);
        *reinterpret_cast<uint32_t*>(dst) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p + k >= 0 && p + k < size) dst[k] = (unsigned char)image_byte(p + k);
}

// One workgroup per image: thread i takes the CRC of its share of the message, moves it to the message's end by x^(8 n) mod P,
// and the 256 results are xor-ed (CRC combination: the CRC of a concatenation is linear in the CRCs of its parts).
__global__ __launch_bounds__(ENT_THREADS) void ent_crc_kernel(const int64_t* __restrict__ sizes, const int64_t* __restrict__ byte_off,
                                                              unsigned char* __restrict__ out, long out_bytes) {
    __shared__ uint32_t part[ENT_THREADS / ENT_WAVE];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long size = sizes[b], off = byte_off[b];
    if (off < 0 || off > out_bytes - size || size < SWC_ENTROPY_HEADER_BYTES) return;  // (uniform)
    const unsigned char* image = out + off;
    const long N = size - 4;
    const long chunk = (N + ENT_THREADS - 1) / ENT_THREADS;
    const long m0 = tid * chunk < N ? tid * chunk : N, m1 = m0 + chunk < N ? m0 + chunk : N;
    uint32_t st = 0xffffffffu;
    for (long k = 0; k < chunk; ++k)
        if (m0 + k < m1) st = swc_ent_crc_byte(st, image[swc_ent_crc_index(m0 + k)]);
    uint32_t v = m0 < m1 ? swc_ent_mulmod(swc_ent_xpow8((uint32_t)(N - m1)), ~st) : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        const uint32_t crc = part[0] ^ part[1] ^ part[2] ^ part[3];
#pragma unroll
        for (int k = 0; k < 4; ++k) out[off + 20 + k] = (unsigned char)(crc >> (8 * k));
    }
}

// ------------------------------------------------------------------------------------------------ decode
__global__ __launch_bounds__(ENT_WAVE) void ent_decode_kernel(const unsigned char* __restrict__ in, long in_bytes,
                                                              const int64_t* __restrict__ stream_off, const int64_t* __restrict__ stream_len,
                                                              const int* __restrict__ stream_mode, const int64_t* __restrict__ n_frames,
                                                              swc_ent_levels lv, int G, int* __restrict__ codes, long ldg, long ldb,
                                                              int L, int n_codes, int* __restrict__ bad) {
    __shared__ uint32_t cnt[4 * 16 * 16];
    const int g = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x, myd = lane >> 4, mys = lane & 15;
    const long idx = (long)b * G + g;
    long Tl = n_frames[b];
    const long off = stream_off[idx], len = stream_len[idx];
    const int mode = stream_mode[idx];
    Tl = Tl > L ? L : Tl;
    if (Tl < 0 || off < 0 || len < 0 || off > in_bytes - len || mode < 0 || mode > 2) {  // not a stream of this buffer
        if (bad != nullptr && lane == 0) atomicAdd(bad, 1);
        Tl = 0;
    }
    const int T = (int)Tl;
    int* dst = codes + (long)g * ldg + (long)b * ldb;
    const unsigned char* s = in + off;
    if (mode == 0 || T == 0) {  // (uniform) raw, and the empty row
        int nbad = 0;
        for (int t = lane; t < L; t += ENT_WAVE) {
            int v = 0;
            if (t < T) {
                v = (int)swc_ent_raw_value(s, len, (uint32_t)t, lv.w);
                nbad += v >= n_codes ? 1 : 0;
            }
            dst[t] = v;
        }
        if (bad != nullptr && nbad) atomicAdd(bad, nbad);
        return;
    }
    const int order = mode - 1;
    counts_init(cnt, lv, myd, mys);
    // the stream's next 64 bytes, one per lane (bytes behind the stream read as 0)
    long bufbase = 0;
    uint32_t bb = lane < len ? s[lane] : 0u;
    long pos = 0;
    auto next_byte = [&]() -> uint32_t {
        if (pos - bufbase >= ENT_WAVE) {  // (uniform)
            bufbase = pos;
            bb = pos + lane < len ? s[pos + lane] : 0u;
        }
        const uint32_t v = lane_read(bb, (int)(pos - bufbase));
        ++pos;
        return v;
    };
    uint32_t low = 0, range = 0xffffffffu, code = 0, prev = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) code = (code << 8) | next_byte();
    for (int t0 = 0; t0 < T; t0 += ENT_WAVE) {
        const int nf = T - t0 < ENT_WAVE ? T - t0 : ENT_WAVE;
        int mine = 0;
        for (int j = 0; j < nf; ++j) {
            const uint32_t ctx = order ? (prev >> (4 * myd)) & 15u : 0u;
            uint32_t* p = &cnt[((myd * 16 + (int)ctx) << 4) + mys];
            uint32_t x = *p;
            const uint32_t incl = seg16_scan(x);
            const uint32_t excl = incl - x;
            const uint32_t tots[4] = {lane_read(incl, 15), lane_read(incl, 31), lane_read(incl, 47), lane_read(incl, 63)};
            uint32_t cur = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t tot = tots[d];
                range /= tot;
                const uint32_t v = swc_ent_target(code, low, range, tot);
                // lanes past L_d hold excl == tot > v; excl of symbol 0 is 0 <= v: at least one bit, the highest is the symbol
                const unsigned long long ball = __ballot(myd == d && excl <= v);
                const int sym = __popcll((ball >> (16 * d)) & 0xffffull) - 1;
                const int src = d * 16 + sym;
                low += lane_read(excl, src) * range;
                range *= lane_read(x, src);
                for (int k = 0; k < SWC_ENTROPY_MAX_RENORM; ++k) {
                    uint32_t byte = 0;
                    if (!swc_ent_renorm(low, range, byte)) break;
                    code = (code << 8) | next_byte();
                }
                cur |= (uint32_t)sym << (4 * d);
            }
            x = swc_ent_update(x, ((cur >> (4 * myd)) & 15u) == (uint32_t)mys, pick4(myd, tots[0], tots[1], tots[2], tots[3]));
            *p = x;
            prev = cur;
            if (lane == j) mine = (int)swc_ent_join(cur, lv);
        }
        if (t0 + lane < T) dst[t0 + lane] = mine;
    }
    for (int t = T + lane; t < L; t += ENT_WAVE) dst[t] = 0;
}

int levels_of(const int32_t* levels4, int32_t G, swc_ent_levels& lv) {
    if (levels4 == nullptr || G < 1 || G > SWC_ENTROPY_MAX_GROUPS) return -1;
    return swc_ent_levels_init(lv, levels4[0], levels4[1], levels4[2], levels4[3]);
}

}  // namespace

extern "C" int64_t swc_entropy_worst_bytes(int64_t T, int32_t G, const int32_t* levels4) {
    swc_ent_levels lv;
    if (T < 0 || T > SWC_ENTROPY_MAX_FRAMES || levels_of(levels4, G, lv) != 0) return -1;
    return SWC_ENTROPY_HEADER_BYTES + 4 * G + G * swc_ent_raw_bytes(T, lv.w);
}

extern "C" int64_t swc_entropy_workspace_bytes(const int64_t* n_frames, int32_t B, int32_t G, const int32_t* levels4, int64_t* out_cap) {
    swc_ent_levels lv;
    if (B < 0 || B > 65535 || (B > 0 && n_frames == nullptr) || levels_of(levels4, G, lv) != 0) return -1;
    int64_t max_t = 0, cap = 0;
    for (int b = 0; b < B; ++b) {
        if (n_frames[b] < 0 || n_frames[b] > SWC_ENTROPY_MAX_FRAMES) return -1;
        max_t = n_frames[b] > max_t ? n_frames[b] : max_t;
        cap += SWC_ENTROPY_HEADER_BYTES + 4 * G + G * swc_ent_raw_bytes(n_frames[b], lv.w);
    }
    if (out_cap) *out_cap = cap;
    if (B == 0) return 0;
    return up256((int64_t)B * G * 2 * 4) + up256((int64_t)B * G * 4) + up256((int64_t)B * G * 2 * slot_bytes_of(max_t, lv.w));
}

extern "C" int swc_entropy_encode_batch(const void* const* rows, const int64_t* ldg, const int64_t* n_frames, int32_t elem_size,
                                        const int32_t* levels_host4, int32_t G, int32_t max_frames, void* out, int64_t out_bytes,
                                        int64_t* byte_off, int64_t* sizes, int32_t* bad, void* workspace, int64_t workspace_bytes,
                                        int32_t B, void* stream) {
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_entropy_encode_batch: B=%d (0..65535)", B);
    SWC_CHECK_ARG(elem_size == 4 || elem_size == 8, "swc_entropy_encode_batch: elem_size=%d (4 = int32 or 8 = int64)", elem_size);
    swc_ent_levels lv;
    SWC_CHECK_ARG(levels_of(levels_host4, G, lv) == 0,
                  "swc_entropy_encode_batch: G=%d (1..8) with four levels in 2..16 whose product is at most 16384", G);
    SWC_CHECK_ARG(max_frames >= 0 && max_frames <= SWC_ENTROPY_MAX_FRAMES, "swc_entropy_encode_batch: max_frames=%d (0..%d)", max_frames,
                  SWC_ENTROPY_MAX_FRAMES);
    if (B == 0) return SWC_OK;
    SWC_CHECK_ARG(rows && ldg && n_frames && out && byte_off && sizes && workspace, "swc_entropy_encode_batch: null pointer");
    SWC_CHECK_ARG(((uintptr_t)rows | (uintptr_t)ldg | (uintptr_t)n_frames | (uintptr_t)byte_off | (uintptr_t)sizes) % 8 == 0 &&
                      (uintptr_t)workspace % 16 == 0 && (bad == nullptr || (uintptr_t)bad % 4 == 0),
                  "swc_entropy_encode_batch: the int64 arrays need 8-byte alignment, the workspace 16, bad 4");
    const int64_t worst = SWC_ENTROPY_HEADER_BYTES + 4 * G + G * swc_ent_raw_bytes(max_frames, lv.w);
    SWC_CHECK_ARG(out_bytes >= (int64_t)B * worst, "swc_entropy_encode_batch: out_bytes=%ld cannot hold %d images of up to %ld bytes",
                  (long)out_bytes, B, (long)worst);
    const int64_t slot = slot_bytes_of(max_frames, lv.w);
    const int64_t need = up256((int64_t)B * G * 2 * 4) + up256((int64_t)B * G * 4) + up256((int64_t)B * G * 2 * slot);
    SWC_CHECK_ARG(workspace_bytes >= need, "swc_entropy_encode_batch: workspace_bytes=%ld, %ld needed", (long)workspace_bytes, (long)need);
    unsigned char* ws = (unsigned char*)workspace;
    int* lens = (int*)ws;
    uint32_t* table = (uint32_t*)(ws + up256((int64_t)B * G * 2 * 4));
    unsigned char* slots = ws + up256((int64_t)B * G * 2 * 4) + up256((int64_t)B * G * 4);
    hipStream_t st = (hipStream_t)stream;
    const long words = (worst + 3 + 3) / 4;  // dwords an image can touch: its bytes + 3 of lead in front of an unaligned start
    const dim3 cgrid(2, (unsigned)G, (unsigned)B), ggrid((unsigned)((words + ENT_THREADS - 1) / ENT_THREADS), (unsigned)B);
    if (max_frames > 0) {
        if (elem_size == 4)
            hipLaunchKernelGGL(ent_code_kernel<int>, cgrid, dim3(ENT_WAVE), 0, st, rows, ldg, n_frames, lv, (int)G, (int)max_frames, lens,
                               slots, (long)slot, (int*)bad);
        else
            hipLaunchKernelGGL(ent_code_kernel<long long>, cgrid, dim3(ENT_WAVE), 0, st, rows, ldg, n_frames, lv, (int)G, (int)max_frames,
                               lens, slots, (long)slot, (int*)bad);
        SWC_CHECK_LAUNCH("swc_entropy_encode_batch (code)");
    }
    hipLaunchKernelGGL(ent_layout_kernel, dim3(1), dim3(ENT_THREADS), 0, st, n_frames, lens, table, sizes, byte_off, (int)B, (int)G, lv.w,
                       (int)max_frames);
    SWC_CHECK_LAUNCH("swc_entropy_encode_batch (layout)");
    if (elem_size == 4)
        hipLaunchKernelGGL(ent_gather_kernel<int>, ggrid, dim3(ENT_THREADS), 0, st, rows, ldg, n_frames, lv, (int)G, (int)max_frames, table,
                           slots, (long)slot, sizes, byte_off, (unsigned char*)out, (long)out_bytes);
    else
        hipLaunchKernelGGL(ent_gather_kernel<long long>, ggrid, dim3(ENT_THREADS), 0, st, rows, ldg, n_frames, lv, (int)G, (int)max_frames,
                           table, slots, (long)slot, sizes, byte_off, (unsigned char*)out, (long)out_bytes);
    SWC_CHECK_LAUNCH("swc_entropy_encode_batch (gather)");
    hipLaunchKernelGGL(ent_crc_kernel, dim3((unsigned)B), dim3(ENT_THREADS), 0, st, sizes, byte_off, (unsigned char*)out, (long)out_bytes);
    SWC_CHECK_LAUNCH("swc_entropy_encode_batch (crc)");
    return SWC_OK;
}

extern "C" int swc_entropy_decode_batch(const void* bytes, int64_t in_bytes, const int64_t* stream_off, const int64_t* stream_len,
                                        const int32_t* stream_mode, const int64_t* n_frames, const int32_t* levels_host4, int32_t G,
                                        int32_t* codes, int64_t ldg, int64_t ldb, int64_t L, int32_t B, int32_t n_codes, int32_t* bad,
                                        void* stream) {
    SWC_CHECK_ARG(bytes && stream_off && stream_len && stream_mode && n_frames && codes, "swc_entropy_decode_batch: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_entropy_decode_batch: B=%d (0..65535)", B);
    swc_ent_levels lv;
    SWC_CHECK_ARG(levels_of(levels_host4, G, lv) == 0,
                  "swc_entropy_decode_batch: G=%d (1..8) with four levels in 2..16 whose product is at most 16384", G);
    SWC_CHECK_ARG(L >= 0 && L <= SWC_ENTROPY_MAX_FRAMES, "swc_entropy_decode_batch: L=%ld (0..%d)", (long)L, SWC_ENTROPY_MAX_FRAMES);
    SWC_CHECK_ARG(ldb >= L && ldg >= (int64_t)B * ldb, "swc_entropy_decode_batch: strides ldg=%ld ldb=%ld must give ldb >= L=%ld and ldg >= B ldb",
                  (long)ldg, (long)ldb, (long)L);
    SWC_CHECK_ARG(in_bytes >= 0, "swc_entropy_decode_batch: in_bytes=%ld", (long)in_bytes);
    SWC_CHECK_ARG(n_codes >= 1, "swc_entropy_decode_batch: n_codes=%d", n_codes);
    if (B == 0 || L == 0) return SWC_OK;
    hipLaunchKernelGGL(ent_decode_kernel, dim3((unsigned)G, (unsigned)B), dim3(ENT_WAVE), 0, (hipStream_t)stream, (const unsigned char*)bytes,
                       (long)in_bytes, stream_off, stream_len, stream_mode, n_frames, lv, (int)G, (int*)codes, (long)ldg, (long)ldb, (int)L,
                       (int)n_codes, (int*)bad);
    SWC_CHECK_LAUNCH("swc_entropy_decode_batch");
    return SWC_OK;
}

extern "C" int swc_entropy_parse(const void* image, int64_t bytes, int32_t check_crc, int32_t* T, int32_t* G, int32_t* levels4,
                                 int64_t* stream_off, int64_t* stream_len, int32_t* stream_mode) {
    return swc_ent_parse((const unsigned char*)image, bytes, check_crc, T, G, levels4, stream_off, stream_len, stream_mode);
}
