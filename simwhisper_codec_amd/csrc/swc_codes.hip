// Batched code files on the device (include/swc_codes.h): a ragged batch of utterances <-> their SWC1 images, one
// launch per batch and direction.
//
// Both kernels are launch-bound at the sizes that occur (32 x 10 s = 44 KB), so what they are built for is ONE launch per
// batch and memory transactions of full width wherever alignment allows:
//   pack    a thread owns one 4-byte-ALIGNED dword of the output buffer (not one frame): the payload is a stream of
//           11-bit codes, so a dword is 32 consecutive bits of it, assembled from the 3 - 4 codes it touches.  A wave
//           stores 256 contiguous bytes; swc_codes_pack writes 11 single bytes per thread at stride 11.  Only the
//           dwords that straddle an image's ends or its header (at most 5 per image) are written byte by byte, so two
//           back-to-back images never write the same byte and nothing outside an image is touched.
//   unpack  a workgroup owns 256 frames of one utterance = 2816 contiguous payload bytes: they are staged in LDS with
//           aligned dword loads (bytes at the ragged ends), then every thread takes its 88 bits out of LDS and writes
//           its 8 codes; per group the 64 stores of a wave are 256 contiguous bytes.
#include "swc_common.h"
#include "swc_codes.h"

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_HDR = SWC_CODEFILE_HEADER_BYTES;
constexpr int CF_FRAME = SWC_CODEFILE_FRAME_BYTES;

// 32 bits of utterance `row`'s payload starting at payload byte pb: code c = 8 t + g sits at bits [11 c, 11 c + 11).
// Codes of frames >= T read as 0 and are not loaded.  (11 T <= 11 * 2^24, so bit positions fit 32 bits.)
template <typename E>
__device__ __forceinline__ unsigned payload_bits(const E* __restrict__ row, long ldg, unsigned T, unsigned pb) {
    const unsigned s = 8u * pb;
    const unsigned c0 = s / 11u;
    const unsigned sh = s - 11u * c0;  // 0..10: 4 codes = 44 bits cover sh + 32
    unsigned long long acc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned c = c0 + j, t = c >> 3, g = c & 7u;
        if (t < T) acc |= (unsigned long long)((unsigned)row[(long)g * ldg + t] & 0x7ffu) << (11 * j);
    }
    return (unsigned)(acc >> sh);
}

template <typename E>
__global__ __launch_bounds__(CF_THREADS) void codes_pack_batch_kernel(const void* const* __restrict__ rows,
                                                                      const int64_t* __restrict__ ldgs,
                                                                      const int64_t* __restrict__ n_frames,
                                                                      const int64_t* __restrict__ byte_off,
                                                                      unsigned char* __restrict__ out, long out_bytes,
                                                                      int max_frames) {
    const int b = blockIdx.y;
    long Tl = n_frames[b];
    Tl = Tl < 0 ? 0 : (Tl > max_frames ? max_frames : Tl);
    const unsigned T = (unsigned)Tl;
    const long size = CF_HDR + (long)CF_FRAME * T;
    const long off = byte_off[b];
    if (off < 0 || off > out_bytes - size) return;  // the image does not lie inside the buffer: nothing of it is written
    const uintptr_t base = reinterpret_cast<uintptr_t>(out) + (uintptr_t)off;
    const long lead = (long)(base & 3u);
    // this thread's dword: the aligned address base - lead + 4 i, image-relative bytes [p, p + 4)
    const long p = 4L * ((long)blockIdx.x * CF_THREADS + threadIdx.x) - lead;
    if (p >= size) return;
    const E* row = T ? reinterpret_cast<const E*>(rows[b]) : nullptr;
    const long ldg = ldgs[b];
    unsigned char* dst = out + off + p;
    if (p >= CF_HDR && p + 4 <= size) {
        *reinterpret_cast<unsigned*>(dst) = payload_bits<E>(row, ldg, T, (unsigned)(p - CF_HDR));
        return;
    }
    // a dword on the image's edge or in its header: the bytes that belong to THIS image, one by one
    const unsigned h0 = 0x31435753u /* "SWC1" */, h1 = T, h2 = 8u | (11u << 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long q = p + k;
        if (q < 0 || q >= size) continue;
        unsigned v;
        if (q < CF_HDR) {
            const unsigned w = q < 4 ? h0 : (q < 8 ? h1 : h2);
            v = w >> (8 * (int)(q & 3));
        } else {
            v = payload_bits<E>(row, ldg, T, (unsigned)(q - CF_HDR));
        }
        dst[k] = (unsigned char)v;
    }
}

// LDS words of one tile: 256 frames x 11 bytes, up to 3 bytes of lead, and 3 words a thread's 4-word window may reach past
// the last staged one (those bits are masked away)
constexpr int CF_TILE_WORDS = (CF_THREADS * CF_FRAME + 3) / 4 + 1 + 3;

__global__ __launch_bounds__(CF_THREADS) void codes_unpack_batch_kernel(const unsigned char* __restrict__ in, long in_bytes,
                                                                        const int64_t* __restrict__ payload_off,
                                                                        const int64_t* __restrict__ n_frames,
                                                                        int* __restrict__ codes, long ldg, long ldb, int L,
                                                                        int n_codes, int* __restrict__ bad) {
    __shared__ unsigned tile[CF_TILE_WORDS];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * CF_THREADS;  // < L
    long Tl = n_frames[b];
    const long off = payload_off[b];
    Tl = Tl > L ? L : Tl;
    if (Tl < 0 || off < 0 || off > in_bytes - (long)CF_FRAME * Tl) {  // not a payload of this buffer: an empty row, counted once
        if (bad != nullptr && blockIdx.x == 0 && tid == 0) atomicAdd(bad, 1);
        Tl = 0;
    }
    const int T = (int)Tl;
    const int t = t0 + tid;
    int* dst = codes + (long)b * ldb + t;
    if (t0 >= T) {  // (uniform) the zero tail of the row
        if (t < L) {
#pragma unroll
            for (int g = 0; g < 8; ++g) dst[g * ldg] = 0;
        }
        return;
    }
    // stage payload bytes [11 t0, 11 tend) at tile byte `lead`: aligned dwords inside, single bytes at the two ends
    const int tend = t0 + CF_THREADS < T ? t0 + CF_THREADS : T;
    const int nbytes = CF_FRAME * (tend - t0);
    const unsigned char* src = in + off + (long)CF_FRAME * t0;
    const int lead = (int)(reinterpret_cast<uintptr_t>(src) & 3u);
    const int nwords = (lead + nbytes + 3) >> 2;
    for (int w = tid; w < nwords; w += CF_THREADS) {
        const int q = 4 * w - lead;  // source byte of this word's byte 0
        unsigned v = 0;
        if (q >= 0 && q + 4 <= nbytes) {
            v = *reinterpret_cast<const unsigned*>(src + q);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (q + k >= 0 && q + k < nbytes) v |= (unsigned)src[q + k] << (8 * k);
        }
        tile[w] = v;
    }
    __syncthreads();
    if (t >= L) return;
    int nbad = 0;
    if (t < T) {
        const int q = lead + CF_FRAME * tid;
        const int w = q >> 2, r = 8 * (q & 3);  // the frame's 88 bits start r bits into word w: they end inside word w + 3
        const unsigned long long lo64 = tile[w] | ((unsigned long long)tile[w + 1] << 32);
        const unsigned long long hi64 = tile[w + 2] | ((unsigned long long)tile[w + 3] << 32);
        const unsigned long long lo = r ? (lo64 >> r) | (hi64 << (64 - r)) : lo64;  // bits 0..63 of the frame
        const unsigned hi = (unsigned)(hi64 >> r);                                   // bits 64..87 (+ bits that are masked)
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int sh = 11 * g;
            unsigned long long v = sh < 64 ? lo >> sh : 0;
            if (sh + 11 > 64) v |= sh >= 64 ? (unsigned long long)(hi >> (sh - 64)) : (unsigned long long)hi << (64 - sh);
            const int c = (int)(v & 0x7ffu);
            nbad += c >= n_codes;
            dst[g * ldg] = c;
        }
    } else {
#pragma unroll
        for (int g = 0; g < 8; ++g) dst[g * ldg] = 0;
    }
    if (bad != nullptr && nbad) atomicAdd(bad, nbad);
}

}  // namespace

extern "C" int64_t swc_codefile_bytes(int64_t n_frames) {
    if (n_frames < 0) return -1;
    return CF_HDR + (int64_t)CF_FRAME * n_frames;
}

extern "C" int swc_codes_pack_batch(const void* const* rows, const int64_t* ldg, const int64_t* n_frames,
                                    const int64_t* byte_off, int32_t elem_size, void* out, int64_t out_bytes,
                                    int32_t max_frames, int32_t B, void* stream) {
    SWC_CHECK_ARG(rows && ldg && n_frames && byte_off && out, "swc_codes_pack_batch: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_codes_pack_batch: B=%d (0..65535)", B);
    SWC_CHECK_ARG(elem_size == 4 || elem_size == 8, "swc_codes_pack_batch: elem_size=%d (4 = int32 or 8 = int64)", elem_size);
    SWC_CHECK_ARG(max_frames >= 0 && max_frames <= SWC_CODEFILE_MAX_FRAMES, "swc_codes_pack_batch: max_frames=%d (0..%d)",
                  max_frames, SWC_CODEFILE_MAX_FRAMES);
    SWC_CHECK_ARG(out_bytes >= (int64_t)CF_HDR * B, "swc_codes_pack_batch: out_bytes=%ld cannot hold %d images (%d bytes of header each)",
                  (long)out_bytes, B, CF_HDR);
    if (B == 0) return SWC_OK;
    // dwords an image of max_frames frames can touch: its bytes, + 3 of lead in front of an unaligned start
    const long words = (CF_HDR + (long)CF_FRAME * max_frames + 3 + 3) / 4;
    const dim3 grid((unsigned)((words + CF_THREADS - 1) / CF_THREADS), (unsigned)B), block(CF_THREADS);
    if (elem_size == 4)
        hipLaunchKernelGGL(codes_pack_batch_kernel<int>, grid, block, 0, (hipStream_t)stream, rows, ldg, n_frames, byte_off,
                           (unsigned char*)out, (long)out_bytes, (int)max_frames);
    else
        hipLaunchKernelGGL(codes_pack_batch_kernel<long long>, grid, block, 0, (hipStream_t)stream, rows, ldg, n_frames, byte_off,
                           (unsigned char*)out, (long)out_bytes, (int)max_frames);
    SWC_CHECK_LAUNCH("swc_codes_pack_batch");
    return SWC_OK;
}

extern "C" int swc_codes_unpack_batch(const void* bytes, int64_t in_bytes, const int64_t* payload_off, const int64_t* n_frames,
                                      int32_t* codes, int64_t ldg, int64_t ldb, int64_t L, int32_t B, int32_t n_codes,
                                      int32_t* bad, void* stream) {
    SWC_CHECK_ARG(bytes && payload_off && n_frames && codes, "swc_codes_unpack_batch: null pointer");
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_codes_unpack_batch: B=%d (0..65535)", B);
    SWC_CHECK_ARG(L >= 0 && L <= SWC_CODEFILE_MAX_FRAMES, "swc_codes_unpack_batch: L=%ld (0..%d)", (long)L, SWC_CODEFILE_MAX_FRAMES);
    SWC_CHECK_ARG(ldb >= L && ldg >= (int64_t)B * ldb, "swc_codes_unpack_batch: strides ldg=%ld ldb=%ld must give ldb >= L=%ld and ldg >= B ldb",
                  (long)ldg, (long)ldb, (long)L);
    SWC_CHECK_ARG(in_bytes >= 0, "swc_codes_unpack_batch: in_bytes=%ld", (long)in_bytes);
    SWC_CHECK_ARG(n_codes >= 1, "swc_codes_unpack_batch: n_codes=%d", n_codes);
    if (B == 0 || L == 0) return SWC_OK;
    const dim3 grid((unsigned)((L + CF_THREADS - 1) / CF_THREADS), (unsigned)B), block(CF_THREADS);
    hipLaunchKernelGGL(codes_unpack_batch_kernel, grid, block, 0, (hipStream_t)stream, (const unsigned char*)bytes, (long)in_bytes,
                       payload_off, n_frames, (int*)codes, (long)ldg, (long)ldb, (int)L, (int)n_codes, (int*)bad);
    SWC_CHECK_LAUNCH("swc_codes_unpack_batch");
    return SWC_OK;
}
