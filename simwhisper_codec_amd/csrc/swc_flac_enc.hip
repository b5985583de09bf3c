// FLAC written on the device (include/swc_flac_enc.h, which states the format contract): B mono int16 rows -> B file images.
//
//   frame kernel   one workgroup of 256 threads per frame.  The block's samples go to LDS (padded by one word every 16, so
//                  that threads walking contiguous runs of up to 16 samples do not meet on a bank).  Per predictor order o
//                  every thread sums zz >> k, k = 0 .. 14, over a contiguous run of its fine partition (the block is cut into
//                  2^pmax fine partitions, pmax = min(6, trailing zeros of bs), and each of those among 256 / 2^pmax threads);
//                  the runs' sums are added per fine partition, the coarser partition orders are sums of pairs (a pyramid of
//                  2^(pmax+1) - 1 nodes x 15 sums in LDS), every node takes its cheapest Rice parameter and every order p
//                  adds its nodes up: bits(o, p) for all 35 candidates without touching a sample more than five times.
//                  Thread 0 makes the choice.  Then an exclusive scan of the code lengths gives every sample its bit position
//                  and each sample ORs its stop bit and low bits into a zeroed LDS bit buffer (at most two 32-bit ORs per
//                  code, whatever the unary length; OR is order-independent, so the bytes are deterministic).  The CRC-16 is
//                  shared too: every thread takes the CRC of its run of bytes and multiplies it by x^(8 bytes behind it).
//                  The frame goes to its fixed-stride slot of the workspace with 32-bit stores, its size beside it.
//   MD5 kernel     one lane per file (RFC 1321 is a serial chain); launched only when asked for.
//   layout kernels per file: the exclusive scan of its frame sizes, their minimum and maximum, the file's size.  Across the
//                  files: the exclusive scan of the sizes.
//   gather kernel  one workgroup per frame copies its slot into the image; one more per file writes the 42 header bytes.
//
// No workgroup waits for another: the phases are separate launches.  No float arithmetic, no global atomics.  Every loop is
// bounded by the block size, the frame count or the file count.
#include "swc_common.h"
#include "swc_flac_enc.h"
#include "swc_flac_enc_bits.h"

namespace {

constexpr int FE_THREADS = 256;
constexpr int FE_MAX_BS = 4096;
constexpr int FE_NK = 15;         // Rice parameters 0 .. 14
constexpr int FE_MAX_P = 6;       // partition orders 0 .. 6
constexpr int FE_NODES = (2 << FE_MAX_P) - 1;  // 127 partitions over all orders
constexpr int FE_MAX_FRAME = SWC_FLAC_ENC_MAX_HEADER + 1 + 2 * FE_MAX_BS + 2;
constexpr int FE_BITWORDS = (FE_MAX_FRAME + 3) / 4 + 1;
constexpr unsigned FE_NONE = 0xFFFFFFFFu;
enum { FE_CONSTANT = 0, FE_VERBATIM = 1, FE_FIXED = 2 };

struct EncArgs {
    const short* const* rows;
    const int64_t* n_samples;
    int64_t max_n;
    int rate, rate_code, bs_log2, BS, F, B;
    int64_t slot;            // bytes per frame slot
    int64_t* frame_off;      // [B][F] byte offset of a frame behind its file's 42 header bytes
    int* frame_bytes;        // [B][F]
    unsigned char* md5;      // [B][16] (null: no signature)
    int* minmax;             // [B][2]
    unsigned char* slots;    // [B][F][slot]
    unsigned char* out;
    int64_t* byte_off;
    int64_t* sizes;
};

__host__ __device__ inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t slot_bytes(int BS) { return (SWC_FLAC_ENC_MAX_HEADER + 1 + 2 * (int64_t)BS + 2 + 15) / 16 * 16; }
inline int64_t worst_file_bytes(int64_t n, int BS) {
    return n <= 0 ? 0 : SWC_FLAC_ENC_STREAM_HEADER + (n + BS - 1) / BS * (SWC_FLAC_ENC_MAX_HEADER + 1 + 2) + 2 * n;
}

// the row's length as the kernels take it: 0 for a row that writes nothing
__device__ __forceinline__ int64_t row_len(const EncArgs& a, int b) {
    const int64_t n = a.n_samples[b];
    return (n <= 0 || n > a.max_n) ? 0 : n;
}

// sample i of the block in the padded LDS image
__device__ __forceinline__ int si(int i) { return i + (i >> 4); }

// exclusive scan over the workgroup's 256 values (buf: 256 elements of LDS); total = their sum
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* buf, T& total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < FE_THREADS; d <<= 1) {
        const T x = t >= d ? buf[t - d] : (T)0;
        __syncthreads();
        buf[t] += x;
        __syncthreads();
    }
    total = buf[FE_THREADS - 1];
    const T incl = buf[t];
    __syncthreads();
    return incl - v;
}

// OR the nbits (1 .. 32) low bits of v (v < 2^nbits) into the MSB-first bit buffer at bit position P
__device__ __forceinline__ void put_bits(unsigned* bw, unsigned P, unsigned v, int nbits) {
    const unsigned w = P >> 5;
    const int room = 32 - (int)(P & 31u);
    if (nbits <= room) {
        atomicOr(&bw[w], v << (room - nbits));
    } else {
        atomicOr(&bw[w], v >> (nbits - room));
        atomicOr(&bw[w + 1], v << (32 - (nbits - room)));
    }
}

__device__ __forceinline__ unsigned zigzag(int e) { return e >= 0 ? (unsigned)e << 1 : ((unsigned)(-e) << 1) - 1u; }

// the o-th finite difference at a sample x with its four predecessors
__device__ __forceinline__ int fixed_residual(int o, int x, int p1, int p2, int p3, int p4) {
    switch (o) {
        case 0: return x;
        case 1: return x - p1;
        case 2: return x - 2 * p1 + p2;
        case 3: return x - 3 * p1 + 3 * p2 - p3;
        default: return x - 4 * p1 + 6 * p2 - 4 * p3 + p4;
    }
}

__global__ __launch_bounds__(FE_THREADS) void flac_enc_frame_kernel(EncArgs a) {
    __shared__ int smp[FE_MAX_BS + FE_MAX_BS / 16];
    __shared__ unsigned part[FE_THREADS * FE_NK];        // the threads' partial sums; the scan's 256 words afterwards
    __shared__ unsigned long long pyr[FE_NODES * FE_NK]; // node (2^p - 1 + j) = partition j of order p
    __shared__ unsigned bitw[FE_BITWORDS];
    __shared__ unsigned nodebits[FE_NODES];
    __shared__ unsigned char bestk[5][FE_NODES + 1];
    __shared__ unsigned cand[5][FE_MAX_P + 1];
    __shared__ unsigned char hdr[16];
    __shared__ int choice[5];  // kind, o, p, subframe bits, header bytes
    __shared__ unsigned crcw[FE_THREADS / 64];

    const int b = blockIdx.y, f = blockIdx.x, t = threadIdx.x;
    const int64_t n = row_len(a, b);
    const int64_t first = (int64_t)f * a.BS;
    if (first >= n) return;  // (uniform) also every frame of a row that writes nothing
    const int bs = (int)((n - first) < (int64_t)a.BS ? (n - first) : (int64_t)a.BS);
    const short* row = a.rows[b] + first;

    int equal = 1;
    const int s0 = row[0];
    for (int i = t; i < bs; i += FE_THREADS) {
        const int v = row[i];
        smp[si(i)] = v;
        equal &= (v == s0);
    }
    for (int w = t; w < FE_BITWORDS; w += FE_THREADS) bitw[w] = 0u;
    if (t < 35) cand[t / 7][t % 7] = FE_NONE;
    const int all_equal = __syncthreads_and(equal);

    int pmax = 0;
    while (pmax < FE_MAX_P && ((bs >> pmax) & 1) == 0) ++pmax;
    const int nfine = 1 << pmax, Lf = bs >> pmax;
    const int S = FE_THREADS >> pmax;            // threads per fine partition (>= 4)
    const int C = (Lf + S - 1) / S;              // samples per thread (<= 16)
    const int omax = bs - 1 < 4 ? bs - 1 : 4;
    const int fj = t / S, fq = t - fj * S;
    const int lo = fj * Lf + fq * C;
    const int hi = (lo + C < (fj + 1) * Lf) ? lo + C : (fj + 1) * Lf;  // (lo >= hi: a thread without samples)

    for (int o = 0; o <= omax; ++o) {
        unsigned acc[FE_NK];
#pragma unroll
        for (int k = 0; k < FE_NK; ++k) acc[k] = 0u;
        {
            // (a thread without samples, lo >= hi, may have lo behind the block: it reads nothing)
            const bool work = lo < hi;
            int p1 = work && lo >= 1 ? smp[si(lo - 1)] : 0, p2 = work && lo >= 2 ? smp[si(lo - 2)] : 0;
            int p3 = work && lo >= 3 ? smp[si(lo - 3)] : 0, p4 = work && lo >= 4 ? smp[si(lo - 4)] : 0;
            for (int i = lo; i < hi; ++i) {
                const int x = smp[si(i)];
                if (i >= o) {
                    const unsigned zz = zigzag(fixed_residual(o, x, p1, p2, p3, p4));
#pragma unroll
                    for (int k = 0; k < FE_NK; ++k) acc[k] += zz >> k;  // <= 16 samples x 2^21
                }
                p4 = p3; p3 = p2; p2 = p1; p1 = x;
            }
        }
#pragma unroll
        for (int k = 0; k < FE_NK; ++k) part[t * FE_NK + k] = acc[k];
        __syncthreads();
        // the fine partitions' sums: the bottom row of the pyramid
        for (int idx = t; idx < nfine * FE_NK; idx += FE_THREADS) {
            const int j = idx / FE_NK, k = idx - j * FE_NK;
            unsigned long long s = 0;
            for (int q = 0; q < S; ++q) s += part[(j * S + q) * FE_NK + k];
            pyr[(nfine - 1 + j) * FE_NK + k] = s;
        }
        __syncthreads();
        for (int p = pmax - 1; p >= 0; --p) {
            for (int idx = t; idx < (FE_NK << p); idx += FE_THREADS) {
                const int j = idx / FE_NK, k = idx - j * FE_NK;
                const int child = (2 << p) - 1 + 2 * j;
                pyr[((1 << p) - 1 + j) * FE_NK + k] = pyr[child * FE_NK + k] + pyr[(child + 1) * FE_NK + k];
            }
            __syncthreads();
        }
        // every partition of every order: its cheapest parameter (the smallest on a tie)
        for (int node = t; node < 2 * nfine - 1; node += FE_THREADS) {
            const int p = 31 - __clz(node + 1), j = node + 1 - (1 << p);
            const int L = bs >> p;
            const long long count = L - (j == 0 ? o : 0);  // may be <= 0 for an order that is not a candidate: not used then
            unsigned long long best = ~0ull;
            int kb = 0;
            for (int k = 0; k < FE_NK; ++k) {
                const unsigned long long c = pyr[node * FE_NK + k] + (unsigned long long)((k + 1) * (count > 0 ? count : 0));
                if (c < best) { best = c; kb = k; }
            }
            nodebits[node] = 4u + (unsigned)(best < 0x0FFFFFFFull ? best : 0x0FFFFFFFull);  // (the minimum is below 2^20)
            bestk[o][node] = (unsigned char)kb;
        }
        __syncthreads();
        if (t <= pmax && (bs >> t) > o) {
            unsigned long long total = 8u + 16u * o + 6u;
            for (int j = 0; j < (1 << t); ++j) total += nodebits[(1 << t) - 1 + j];
            cand[o][t] = total < 0xFFFFFFF0ull ? (unsigned)total : 0xFFFFFFF0u;
        }
        __syncthreads();
    }

    if (t == 0) {
        const unsigned verbatim = 8u + 16u * (unsigned)bs;
        unsigned best = FE_NONE;
        int bo = 0, bp = 0;
        for (int o = 0; o <= omax; ++o)
            for (int p = 0; p <= pmax; ++p)
                if (cand[o][p] < best) { best = cand[o][p]; bo = o; bp = p; }
        int kind = FE_VERBATIM;
        unsigned bits = verbatim;
        if (best < verbatim) { kind = FE_FIXED; bits = best; }
        if (all_equal && 24u <= bits) { kind = FE_CONSTANT; bits = 24u; }
        choice[0] = kind; choice[1] = bo; choice[2] = bp; choice[3] = (int)bits;
        choice[4] = swc_fenc_frame_header(hdr, (unsigned)f, bs, a.bs_log2, a.rate, a.rate_code);
    }
    __syncthreads();
    const int kind = choice[0], o = choice[1], p = choice[2], hlen = choice[4];
    const unsigned P0 = 8u * (unsigned)hlen;          // the subframe's first bit
    const unsigned total_bits = P0 + (unsigned)choice[3];
    const int nb = (int)((total_bits + 7u) >> 3);     // frame bytes in front of the CRC-16

    if (t < hlen) put_bits(bitw, 8u * t, hdr[t], 8);
    if (kind == FE_CONSTANT) {
        if (t == 0) put_bits(bitw, P0 + 8u, (unsigned)s0 & 0xFFFFu, 16);
    } else if (kind == FE_VERBATIM) {
        if (t == 0) put_bits(bitw, P0, 0x02u, 8);
        for (int i = t; i < bs; i += FE_THREADS) put_bits(bitw, P0 + 8u + 16u * i, (unsigned)smp[si(i)] & 0xFFFFu, 16);
    } else {
        if (t == 0) {
            put_bits(bitw, P0, (unsigned)(8 + o) << 1, 8);
            put_bits(bitw, P0 + 8u + 16u * o, (unsigned)p, 6);  // Rice method 00, the partition order
        }
        if (t < o) put_bits(bitw, P0 + 8u + 16u * t, (unsigned)smp[si(t)] & 0xFFFFu, 16);
        const unsigned R0 = P0 + 8u + 16u * o + 6u;  // the first partition's parameter
        const int L = bs >> p;
        const int C2 = (bs + FE_THREADS - 1) / FE_THREADS;
        const int lo2 = t * C2 < bs ? t * C2 : bs;
        const int hi2 = lo2 + C2 < bs ? lo2 + C2 : bs;
        const unsigned char* ks = &bestk[o][(1 << p) - 1];
        // pass 1: the bits of this thread's codes
        unsigned mine = 0;
        {
            int p1 = lo2 >= 1 ? smp[si(lo2 - 1)] : 0, p2 = lo2 >= 2 ? smp[si(lo2 - 2)] : 0;
            int p3 = lo2 >= 3 ? smp[si(lo2 - 3)] : 0, p4 = lo2 >= 4 ? smp[si(lo2 - 4)] : 0;
            int j = lo2 / L, jend = (j + 1) * L;
            int k = ks[j < (1 << p) ? j : 0];
            for (int i = lo2; i < hi2; ++i) {
                if (i == jend) { ++j; jend += L; k = ks[j]; }
                const int x = smp[si(i)];
                if (i >= o) mine += (zigzag(fixed_residual(o, x, p1, p2, p3, p4)) >> k) + 1u + (unsigned)k;
                p4 = p3; p3 = p2; p2 = p1; p1 = x;
            }
        }
        unsigned all;
        unsigned run = block_excl_scan<unsigned>(mine, part, all);
        // pass 2: the codes, and the parameter in front of a partition's first code
        {
            int p1 = lo2 >= 1 ? smp[si(lo2 - 1)] : 0, p2 = lo2 >= 2 ? smp[si(lo2 - 2)] : 0;
            int p3 = lo2 >= 3 ? smp[si(lo2 - 3)] : 0, p4 = lo2 >= 4 ? smp[si(lo2 - 4)] : 0;
            int j = lo2 / L, jend = (j + 1) * L;
            int k = ks[j < (1 << p) ? j : 0];
            for (int i = lo2; i < hi2; ++i) {
                if (i == jend) { ++j; jend += L; k = ks[j]; }
                const int x = smp[si(i)];
                if (i >= o) {
                    if (i == (j == 0 ? o : j * L)) put_bits(bitw, R0 + 4u * j + run, (unsigned)k, 4);
                    const unsigned zz = zigzag(fixed_residual(o, x, p1, p2, p3, p4));
                    const unsigned q = zz >> k;
                    put_bits(bitw, R0 + 4u * (j + 1) + run + q, (1u << k) | (zz & ((1u << k) - 1u)), k + 1);
                    run += q + 1u + (unsigned)k;
                }
                p4 = p3; p3 = p2; p2 = p1; p1 = x;
            }
        }
    }
    __syncthreads();

    // CRC-16 of bytes [0, nb): a run of whole words per thread, shifted behind by the bytes that follow it
    {
        const int CH = (((nb + FE_THREADS - 1) / FE_THREADS) + 3) & ~3;
        const int c0 = t * CH, c1 = c0 + CH < nb ? c0 + CH : nb;
        unsigned c = 0;
        for (int i = c0; i < c1; ++i) c = swc_fenc_crc16_byte(c, (bitw[i >> 2] >> (24 - 8 * (i & 3))) & 0xFFu);
        if (c0 < nb) c = swc_fenc_mulmod(c, swc_fenc_xpow8((unsigned)(nb - c1)));
        for (int d = 32; d >= 1; d >>= 1) c ^= (unsigned)__shfl_xor((int)c, d, 64);
        if ((t & 63) == 0) crcw[t >> 6] = c;
        __syncthreads();
        if (t == 0) put_bits(bitw, 8u * (unsigned)nb, crcw[0] ^ crcw[1] ^ crcw[2] ^ crcw[3], 16);
        __syncthreads();
    }

    const int64_t fi = (int64_t)b * a.F + f;
    unsigned* dst = reinterpret_cast<unsigned*>(a.slots + fi * a.slot);  // 16-byte aligned; (nb + 2) rounded up to 4 <= slot
    for (int w = t; w < (nb + 2 + 3) / 4; w += FE_THREADS) dst[w] = __builtin_bswap32(bitw[w]);
    if (t == 0) a.frame_bytes[fi] = nb + 2;
}

__global__ __launch_bounds__(64) void flac_enc_md5_kernel(EncArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const int64_t n = row_len(a, b);
    if (n == 0) return;
    swc_fenc_md5_i16(reinterpret_cast<const uint16_t*>(a.rows[b]), n, a.md5 + 16 * (int64_t)b);
}

// per file: where its frames go, the smallest and the largest, the file's size
__global__ __launch_bounds__(FE_THREADS) void flac_enc_file_layout_kernel(EncArgs a) {
    __shared__ unsigned buf[FE_THREADS];
    __shared__ int mm[2][FE_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t n = row_len(a, b);
    const int nf = (int)((n + a.BS - 1) / a.BS);  // <= F
    int64_t carry = 0;
    int mn = 0x7FFFFFFF, mx = 0;
    for (int base = 0; base < nf; base += FE_THREADS) {
        const int fr = base + t;
        const unsigned v = fr < nf ? (unsigned)a.frame_bytes[(int64_t)b * a.F + fr] : 0u;
        unsigned total;
        const unsigned ex = block_excl_scan<unsigned>(v, buf, total);
        if (fr < nf) {
            a.frame_off[(int64_t)b * a.F + fr] = carry + ex;
            mn = (int)v < mn ? (int)v : mn;
            mx = (int)v > mx ? (int)v : mx;
        }
        carry += total;
    }
    mm[0][t] = mn; mm[1][t] = mx;
    __syncthreads();
    for (int d = FE_THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) {
            mm[0][t] = mm[0][t + d] < mm[0][t] ? mm[0][t + d] : mm[0][t];
            mm[1][t] = mm[1][t + d] > mm[1][t] ? mm[1][t + d] : mm[1][t];
        }
        __syncthreads();
    }
    if (t == 0) {
        a.minmax[2 * b] = nf ? mm[0][0] : 0;
        a.minmax[2 * b + 1] = mm[1][0];
        a.sizes[b] = nf ? SWC_FLAC_ENC_STREAM_HEADER + carry : 0;
    }
}

// across the files: byte_off = the exclusive scan of sizes
__global__ __launch_bounds__(FE_THREADS) void flac_enc_batch_layout_kernel(EncArgs a) {
    __shared__ int64_t buf[FE_THREADS];
    const int t = threadIdx.x;
    int64_t carry = 0;
    for (int base = 0; base < a.B; base += FE_THREADS) {
        const int b = base + t;
        const int64_t v = b < a.B ? a.sizes[b] : 0;
        int64_t total;
        const int64_t ex = block_excl_scan<int64_t>(v, buf, total);
        if (b < a.B) a.byte_off[b] = carry + ex;
        carry += total;
    }
}

// blockIdx.x < F: frame x of file y, slot -> image.  blockIdx.x == F: the file's 42 header bytes.  The images lie at any
// byte address: byte stores.
__global__ __launch_bounds__(FE_THREADS) void flac_enc_gather_kernel(EncArgs a) {
    __shared__ unsigned char head[SWC_FLAC_ENC_STREAM_HEADER];
    const int b = blockIdx.y, f = blockIdx.x, t = threadIdx.x;
    const int64_t n = row_len(a, b);
    if (n == 0) return;
    unsigned char* img = a.out + a.byte_off[b];
    if (f == a.F) {
        if (t == 0)
            swc_fenc_stream_header(head, a.BS, (unsigned)a.minmax[2 * b], (unsigned)a.minmax[2 * b + 1], a.rate, (uint64_t)n,
                                   a.md5 ? a.md5 + 16 * (int64_t)b : nullptr);
        __syncthreads();
        if (t < SWC_FLAC_ENC_STREAM_HEADER) img[t] = head[t];
        return;
    }
    if ((int64_t)f * a.BS >= n) return;
    const int64_t fi = (int64_t)b * a.F + f;
    const unsigned char* src = a.slots + fi * a.slot;
    unsigned char* dst = img + SWC_FLAC_ENC_STREAM_HEADER + a.frame_off[fi];
    const int nbytes = a.frame_bytes[fi];
    for (int i = t; i < nbytes; i += FE_THREADS) dst[i] = src[i];
}

// the parts of the workspace for B files of up to max_n samples: -> its size; offsets[5] = frame_off, frame_bytes, md5,
// minmax, slots
int64_t workspace_parts(int B, int64_t max_n, int BS, int64_t* offsets) {
    const int64_t F = (max_n + BS - 1) / BS;
    int64_t pos = 0;
    const int64_t sizes[5] = {8 * B * F, 4 * B * F, 16 * (int64_t)B, 8 * (int64_t)B, B * F * slot_bytes(BS)};
    for (int i = 0; i < 5; ++i) {
        if (offsets) offsets[i] = pos;
        pos += align256(sizes[i]);
    }
    return pos;
}

}  // namespace

extern "C" int64_t swc_flac_encode_workspace_bytes(const int64_t* n_samples, int32_t B, int32_t blocksize, int64_t* out_cap) {
    if (B < 0 || B > 65535 || (B > 0 && !n_samples) || swc_fenc_bs_log2(blocksize) < 0) return -1;
    int64_t max_n = 0, cap = 0;
    for (int b = 0; b < B; ++b) {
        if (n_samples[b] < 0 || n_samples[b] > 0x7FFFFFFFLL) return -1;
        max_n = n_samples[b] > max_n ? n_samples[b] : max_n;
        cap += worst_file_bytes(n_samples[b], blocksize);
    }
    if ((max_n + blocksize - 1) / blocksize * B > SWC_FLAC_ENC_MAX_FRAMES) return -1;
    if (out_cap) *out_cap = cap;
    return B == 0 ? 0 : workspace_parts(B, max_n, blocksize, nullptr);
}

extern "C" int swc_flac_encode_batch(const void* rows, const int64_t* n_samples, int32_t rate, int32_t blocksize, int32_t md5,
                                     void* out, int64_t out_bytes, int64_t* byte_off, int64_t* sizes, void* workspace,
                                     int64_t workspace_bytes, int64_t max_n, int32_t B, void* stream) {
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_flac_encode_batch: B=%d (0..65535)", B);
    const int bs_log2 = swc_fenc_bs_log2(blocksize);
    SWC_CHECK_ARG(bs_log2 >= 0, "swc_flac_encode_batch: blocksize=%d (256, 512, 1024, 2048 or 4096)", blocksize);
    const int rate_code = swc_fenc_rate_code(rate);
    SWC_CHECK_ARG(rate_code != 0, "swc_flac_encode_batch: rate=%d (one of RFC 9639's frame-header table, or 1..65535)", rate);
    SWC_CHECK_ARG(max_n >= 0 && max_n <= 0x7FFFFFFFLL, "swc_flac_encode_batch: max_n=%ld (0..2^31-1)", (long)max_n);
    SWC_CHECK_ARG(out_bytes >= 0 && workspace_bytes >= 0, "swc_flac_encode_batch: out_bytes=%ld workspace_bytes=%ld", (long)out_bytes,
                  (long)workspace_bytes);
    if (B == 0) return SWC_OK;
    SWC_CHECK_ARG(rows && n_samples && out && byte_off && sizes && workspace, "swc_flac_encode_batch: null pointer");
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(rows) & 7u) == 0 && (reinterpret_cast<uintptr_t>(n_samples) & 7u) == 0 &&
                      (reinterpret_cast<uintptr_t>(byte_off) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sizes) & 7u) == 0 &&
                      aligned16(workspace),
                  "swc_flac_encode_batch: rows, n_samples, byte_off and sizes need 8-byte alignment, the workspace 16");
    const int64_t F = (max_n + blocksize - 1) / blocksize;
    SWC_CHECK_ARG(F * B <= SWC_FLAC_ENC_MAX_FRAMES, "swc_flac_encode_batch: %ld frames (B=%d, max_n=%ld; at most %d)", (long)(F * B), B,
                  (long)max_n, SWC_FLAC_ENC_MAX_FRAMES);
    const int64_t worst = B * worst_file_bytes(max_n, blocksize);
    SWC_CHECK_ARG(out_bytes >= worst, "swc_flac_encode_batch: out_bytes=%ld is below the worst case %ld of %d files of %ld samples",
                  (long)out_bytes, (long)worst, B, (long)max_n);
    int64_t off[5];
    const int64_t need = workspace_parts(B, max_n, blocksize, off);
    SWC_CHECK_ARG(workspace_bytes >= need, "swc_flac_encode_batch: workspace_bytes=%ld, %ld needed", (long)workspace_bytes, (long)need);

    unsigned char* ws = (unsigned char*)workspace;
    EncArgs a;
    a.rows = (const short* const*)rows; a.n_samples = n_samples; a.max_n = max_n;
    a.rate = rate; a.rate_code = rate_code; a.bs_log2 = bs_log2; a.BS = blocksize; a.F = (int)F; a.B = B;
    a.slot = slot_bytes(blocksize);
    a.frame_off = (int64_t*)(ws + off[0]); a.frame_bytes = (int*)(ws + off[1]);
    a.md5 = md5 ? ws + off[2] : nullptr; a.minmax = (int*)(ws + off[3]); a.slots = ws + off[4];
    a.out = (unsigned char*)out; a.byte_off = byte_off; a.sizes = sizes;
    hipStream_t st = (hipStream_t)stream;
    if (F > 0) {
        hipLaunchKernelGGL(flac_enc_frame_kernel, dim3((unsigned)F, (unsigned)B), dim3(FE_THREADS), 0, st, a);
        SWC_CHECK_LAUNCH("swc_flac_encode_batch (frames)");
        if (md5) {
            hipLaunchKernelGGL(flac_enc_md5_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, a);
            SWC_CHECK_LAUNCH("swc_flac_encode_batch (md5)");
        }
    }
    hipLaunchKernelGGL(flac_enc_file_layout_kernel, dim3((unsigned)B), dim3(FE_THREADS), 0, st, a);
    SWC_CHECK_LAUNCH("swc_flac_encode_batch (file layout)");
    hipLaunchKernelGGL(flac_enc_batch_layout_kernel, dim3(1), dim3(FE_THREADS), 0, st, a);
    SWC_CHECK_LAUNCH("swc_flac_encode_batch (batch layout)");
    if (F > 0) {
        hipLaunchKernelGGL(flac_enc_gather_kernel, dim3((unsigned)F + 1u, (unsigned)B), dim3(FE_THREADS), 0, st, a);
        SWC_CHECK_LAUNCH("swc_flac_encode_batch (gather)");
    }
    return SWC_OK;
}
