// FLAC on the device (include/swc_flac.h): the compressed bytes of a batch of files -> interleaved int16 samples.
//
//   frame kernel   a work item (one lane) is one frame: the entropy and predictor chain inside a frame is serial by nature of
//                  the format, the frames are independent (swc_flac_index found and proved them on the host).  The lane runs
//                  csrc/swc_flac_frame.h — the text the host tests and the sanitizer program run — into int32 planes of the
//                  workspace and stores its status word.  Per-lane state stays out of scratch: the bit accumulator lives in
//                  registers, the 32 LPC coefficients in LDS (lane-interleaved: coefficient j of lane l at word 64 j + l, no
//                  bank conflict), the predictor history is read back from the planes.
//                  A wave is one workgroup of 64 lanes of which `fpw` (frames per wave: 1, 2, 4 ... 64) are active.  The work
//                  of a lane is long and latency bound (every sample waits for its history to come back from the planes),
//                  and an instruction costs the same however many lanes are active, so a wave is NOT filled: 8 frames per
//                  wave measured fastest, or within its spread of the fastest, both at 1 280 frames (32 x 10 s, 16 kHz mono,
//                  block size 4096) and at 3 776 (48 kHz stereo); 1 and 64 per wave are 10 - 38 % slower.  The table is in
//                  DESIGN.md 17, the raw output in profiles/flac_bench.txt.
//                  fpw = 8, doubled while the grid would exceed FL_TARGET_WAVES.
//   output kernel  a workgroup is one frame again, but all its threads share the block's samples: stereo decorrelation
//                  undone, bps < 16 shifted up, narrowed to int16, stored channel-interleaved in consecutive order.  It
//                  first reduces the status words of the frame's FILE (__syncthreads_or): a file with one failed frame
//                  writes nothing.  No atomics anywhere.
#include "swc_common.h"
#include "swc_flac.h"
#include "swc_flac_frame.h"

namespace {

constexpr int FL_WAVE = 64;
constexpr int FL_MIN_FPW = 8;
constexpr int FL_TARGET_WAVES = 2048;  // 256 CUs x 4 SIMDs x 2
constexpr int FL_OUT_THREADS = 256;

struct FlacArgs {
    const unsigned char* bytes;
    long n_bytes;
    const swc_flac_frame* frames;
    int n_frames;
    const swc_flac_file* files;
    int B;
    long out_elems;
    long plane_elems;
};

// Is table entry f (and the file it names) wholly inside every buffer and consistent?  Both kernels ask the same question
// of the same words; nothing is read or written through an entry that fails.
__device__ __forceinline__ bool entry_ok(const FlacArgs& a, const swc_flac_frame& fr, int f, swc_flac_file& fi) {
    if (fr.file < 0 || fr.file >= a.B) return false;
    fi = a.files[fr.file];
    if (fi.channels < 1 || fi.channels > SWC_FLAC_MAX_CHANNELS || fi.bps < 4 || fi.bps > SWC_FLAC_MAX_BPS) return false;
    if (fi.n_samples < 0 || fi.n_samples > (1L << 40) || fi.blocksize < 1 || fi.blocksize > SWC_FLAC_MAX_BLOCKSIZE) return false;
    const long span = fi.n_samples * fi.channels;
    if (fi.out_off < 0 || fi.out_off > a.out_elems - span) return false;
    if (fi.plane_off < 0 || fi.plane_off > a.plane_elems - span) return false;
    if (fi.n_frames < 0 || fi.first_frame < 0 || fi.first_frame > a.n_frames - fi.n_frames) return false;
    if (f < fi.first_frame || f >= fi.first_frame + fi.n_frames) return false;
    if (fr.blocksize < 1 || fr.blocksize > fi.blocksize) return false;
    // fixed block size: frame k of its file starts at sample k blocksize (the output kernel relies on nothing else)
    if (fr.first_sample != (long)(f - fi.first_frame) * fi.blocksize || fr.first_sample > fi.n_samples - fr.blocksize) return false;
    if (fr.hdr_bytes < 5 || fr.n_bytes < fr.hdr_bytes + 2 || fr.n_bytes > SWC_FLAC_MAX_FRAME_BYTES) return false;
    if (fr.byte_off < 0 || fr.byte_off > a.n_bytes - fr.n_bytes) return false;
    if (fr.chan_assign < 0 || fr.chan_assign > 10 || fi.channels != (fr.chan_assign < 8 ? fr.chan_assign + 1 : 2)) return false;
    return true;
}

__global__ __launch_bounds__(FL_WAVE) void flac_frame_kernel(FlacArgs a, int* __restrict__ planes, int* __restrict__ status,
                                                             int fpw) {
    __shared__ int coef[32 * FL_WAVE];
    const int lane = threadIdx.x;
    const long fl = (long)blockIdx.x * fpw + lane;
    if (lane >= fpw || fl >= a.n_frames) return;
    const int f = (int)fl;
    const swc_flac_frame fr = a.frames[f];
    swc_flac_file fi;
    int st = SWC_FLAC_ST_ENTRY;
    if (entry_ok(a, fr, f, fi))
        st = swc_flac_decode_frame(a.bytes + fr.byte_off, fr.n_bytes, fr.hdr_bytes, fr.blocksize, fi.channels, fi.bps,
                                   fr.chan_assign, planes + fi.plane_off + fr.first_sample, fi.n_samples, coef + lane, FL_WAVE);
    status[f] = st;
}

__global__ __launch_bounds__(FL_OUT_THREADS) void flac_output_kernel(FlacArgs a, const int* __restrict__ planes,
                                                                     const int* __restrict__ status, short* __restrict__ out) {
    const int f = blockIdx.x;
    const swc_flac_frame fr = a.frames[f];
    swc_flac_file fi;
    if (!entry_ok(a, fr, f, fi)) return;  // (uniform)
    int bad = 0;
    for (int k = threadIdx.x; k < fi.n_frames; k += FL_OUT_THREADS) bad |= status[fi.first_frame + k];
    if (__syncthreads_or(bad)) return;
    const int ch = fi.channels, up = 16 - fi.bps, ca = fr.chan_assign;
    const int* p0 = planes + fi.plane_off + fr.first_sample;
    short* dst = out + fi.out_off + fr.first_sample * ch;
    const int n = fr.blocksize * ch;  // <= 65536 * 8
    for (int e = threadIdx.x; e < n; e += FL_OUT_THREADS) {
        const int i = e / ch, c = e - i * ch;
        int v;
        if (ca >= 8) v = swc_flac_undo_stereo(p0[i], p0[fi.n_samples + i], ca, c);
        else v = p0[(long)c * fi.n_samples + i];
        dst[e] = (short)((unsigned)v << up);
    }
}

int pick_fpw(int n_frames) {
    int fpw = FL_MIN_FPW;
    while (fpw < FL_WAVE && (long)fpw * FL_TARGET_WAVES < n_frames) fpw *= 2;
    return fpw;
}

}  // namespace

extern "C" int64_t swc_flac_decode_workspace_bytes(const int64_t* n_samples, const int32_t* channels, int32_t B, int64_t* plane_off) {
    if (B < 0 || B > 65535 || (B > 0 && (!n_samples || !channels))) return -1;
    int64_t pos = 0;
    for (int b = 0; b < B; ++b) {
        if (n_samples[b] < 0 || n_samples[b] > ((int64_t)1 << 40) || channels[b] < 1 || channels[b] > SWC_FLAC_MAX_CHANNELS) return -1;
        if (plane_off) plane_off[b] = pos;
        const int64_t e = n_samples[b] * channels[b];
        pos += (e + SWC_FLAC_PLANE_ALIGN - 1) / SWC_FLAC_PLANE_ALIGN * SWC_FLAC_PLANE_ALIGN;
    }
    return pos * 4;
}

extern "C" int swc_flac_decode_batch_ex(const void* bytes, int64_t n_bytes, const swc_flac_frame* frames, int32_t n_frames,
                                        const swc_flac_file* files, int32_t B, int16_t* out_i16, int64_t out_elems,
                                        int32_t* status, void* workspace, int64_t workspace_bytes, int32_t frames_per_wave,
                                        void* stream) {
    SWC_CHECK_ARG(n_frames >= 0 && n_frames <= SWC_FLAC_MAX_FRAMES, "swc_flac_decode_batch: n_frames=%d (0..%d)", n_frames,
                  SWC_FLAC_MAX_FRAMES);
    SWC_CHECK_ARG(B >= 0 && B <= 65535, "swc_flac_decode_batch: B=%d (0..65535)", B);
    SWC_CHECK_ARG(n_bytes >= 0 && out_elems >= 0 && workspace_bytes >= 0, "swc_flac_decode_batch: n_bytes=%ld out_elems=%ld workspace_bytes=%ld",
                  (long)n_bytes, (long)out_elems, (long)workspace_bytes);
    SWC_CHECK_ARG(frames_per_wave >= 0 && frames_per_wave <= FL_WAVE && (frames_per_wave & (frames_per_wave - 1)) == 0,
                  "swc_flac_decode_batch: frames_per_wave=%d (0 or a power of two up to 64)", frames_per_wave);
    SWC_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out_i16) & 1u) == 0 &&
                      (reinterpret_cast<uintptr_t>(status) & 3u) == 0 && (reinterpret_cast<uintptr_t>(frames) & 7u) == 0 &&
                      (reinterpret_cast<uintptr_t>(files) & 7u) == 0,
                  "swc_flac_decode_batch: workspace needs 16-byte alignment, the tables 8, status 4, out_i16 2");
    if (n_frames == 0) return SWC_OK;
    SWC_CHECK_ARG(bytes && frames && files && out_i16 && status && workspace, "swc_flac_decode_batch: null pointer");
    SWC_CHECK_ARG(B >= 1, "swc_flac_decode_batch: %d frames of no file", n_frames);
    FlacArgs a;
    a.bytes = (const unsigned char*)bytes; a.n_bytes = (long)n_bytes; a.frames = frames; a.n_frames = n_frames;
    a.files = files; a.B = B; a.out_elems = (long)out_elems; a.plane_elems = (long)(workspace_bytes / 4);
    const int fpw = frames_per_wave ? frames_per_wave : pick_fpw(n_frames);
    const unsigned waves = (unsigned)((n_frames + fpw - 1) / fpw);
    hipLaunchKernelGGL(flac_frame_kernel, dim3(waves), dim3(FL_WAVE), 0, (hipStream_t)stream, a, (int*)workspace, (int*)status, fpw);
    SWC_CHECK_LAUNCH("swc_flac_decode_batch (frames)");
    hipLaunchKernelGGL(flac_output_kernel, dim3((unsigned)n_frames), dim3(FL_OUT_THREADS), 0, (hipStream_t)stream, a,
                       (const int*)workspace, (const int*)status, (short*)out_i16);
    SWC_CHECK_LAUNCH("swc_flac_decode_batch (output)");
    return SWC_OK;
}

extern "C" int swc_flac_decode_batch(const void* bytes, int64_t n_bytes, const swc_flac_frame* frames, int32_t n_frames,
                                     const swc_flac_file* files, int32_t B, int16_t* out_i16, int64_t out_elems, int32_t* status,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    return swc_flac_decode_batch_ex(bytes, n_bytes, frames, n_frames, files, B, out_i16, out_elems, status, workspace,
                                    workspace_bytes, 0, stream);
}
