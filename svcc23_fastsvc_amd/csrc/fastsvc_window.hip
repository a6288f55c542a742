// fastsvc_window.hip - the two ends of a windowed decode on gfx950 (decode.DecodeSession.convert_windowed): a long
// utterance runs as overlapping windows - rows of a ragged batch - and the windows' waveforms are cross-faded back
// into one.
//
//   window_assemble   batch row r is a SLICE of an utterance: `frames[r]` frames of the packed time-major ppg from
//                     element ppg_off[r], and the matching frames * hop samples of the packed lft and of the packed
//                     excitation (both from element sig_off[r]: the two buffers share one layout) ->
//                         ppg_out (R, C, width)         transposed to channel-major, columns >= frames zero
//                         lft_out, sine_out (R, 1, width * hop)   copied bit for bit, the tail zero
//                     gather_time_major's transpose and fanout_assemble's row copies, on slices whose offsets have no
//                     alignment at all.
//   window_stitch     the forward's (B, width * hop) waveform rows -> packed PCM-16 and / or packed float32, each
//                     utterance sample written once: outside the fade zones the owning window's sample, inside the zone
//                     around an interior boundary (1 - w) * y_left + w * y_right in float64, w = (j + 0.5) / (2 * half)
//                     for the zone's sample j - decode.stitch_windows' arithmetic bit for bit (this unit is compiled
//                     with -ffp-contract=off: the two products and the sum round separately, as numpy's do).
//
// The reference decodes one whole utterance at a time (decode_fastsvc.py:150-200) and has no counterpart.  Both kernels
// are data movement, priced as (bytes read + bytes written) / HBM bandwidth; they have no tunables.
//
// Where the other window of a fade zone comes from.  A zone needs two rows, and bucket_ragged may put them into different
// batches.  Only the zones are kept across batches - 2 * half samples per interior boundary, not whole rows: the row that
// runs FIRST copies its zone samples into a slot of a small per-call float32 staging buffer (mode STAGE) and writes no
// output for the zone; the row that runs LATER reads the slot (mode FROM_STAGE) and writes the blended samples.  When both
// rows are in the same batch the left one reads the right one's samples straight out of `y` (mode FROM_Y) and the right
// one leaves the zone alone (mode SKIP).  Launches of one stream run in order, so a slot is complete before it is read,
// and no sample is written twice.  Every row therefore writes ONE contiguous run of its utterance - its core, minus the
// zones it does not resolve, plus the ones it does - which goes to dst + dst_off[r].
//
// Block roles of the assemble, by blockIdx.x range (uniform per block):
//     [0, n_sig)        padded row copies of lft       (1024 destination elements per block)
//     [.., + n_sig)     padded row copies of the excitation
//     [.., + n_tile)    64 x 64 ppg transpose tiles through LDS (pitch 65 dwords: see fastsvc_decodeio.hip)
// Row descriptors travel IN the kernel arguments, 64 rows per launch: 20 bytes a row for the assemble, 48 for the stitch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "fastsvc_hip.h"

namespace fastsvc {
int set_last_error(int code, const char* msg);      // fastsvc_plan.cpp: the text fastsvc_last_error() returns
}

namespace {

constexpr int WN_MAX = 64;                          // rows per launch (the arguments hold their descriptors)
constexpr int WN_TILE = 64;
constexpr int WN_PITCH = 65;
constexpr int WN_CHUNK = 1024;                      // elements of a row one copy block covers (256 lanes x 16 bytes)

struct WindowArgs {
    long ppg_off[WN_MAX];                           // first element of the row's (frames, C) slice in `ppg`
    long sig_off[WN_MAX];                           // first of its frames * hop samples in `lft` and in `sine`
    int frames[WN_MAX];
};

struct WindowDims {
    int C, hop, width;
    int sig_chunks;                                 // copy blocks per row and signal
    int tiles_t, tiles_c;                           // ppg tiles per row
    unsigned n_sig, n_tile;
};

inline int row_chunks(long len) { return (int)((len + 3 + WN_CHUNK - 1) / WN_CHUNK); }

// Lane `tid` of copy block `chunk` owns one 16-byte aligned piece of dst[0, width): with s = elements between the
// previous 16-byte boundary and dst, piece g = chunk * 256 + tid holds elements [4 g - s, 4 g - s + 4) clipped to
// [0, width).  Element k is src[k] for k < len and 0 from len on; src is read at [0, len) only.
__device__ __forceinline__ void padded_piece(const float* __restrict__ src, float* __restrict__ dst, int len, int width,
                                             int chunk, int tid) {
    const int s = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
    const long k0 = ((long)chunk * 256 + tid) * 4 - s;
    if (k0 >= width) return;
    if (k0 >= 0 && k0 + 4 <= width) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + 4 <= len) {
            if ((reinterpret_cast<uintptr_t>(src + k0) & 15) == 0) {
                v = *reinterpret_cast<const float4*>(src + k0);
            } else {
                v.x = src[k0]; v.y = src[k0 + 1]; v.z = src[k0 + 2]; v.w = src[k0 + 3];
            }
        } else if (k0 < len) {                      // (the piece that holds the slice's end: 1 - 3 elements of it)
            v.x = src[k0];
            if (k0 + 1 < len) v.y = src[k0 + 1];
            if (k0 + 2 < len) v.z = src[k0 + 2];
        }
        *reinterpret_cast<float4*>(dst + k0) = v;
    } else {
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long k = k0 + e;
            if (k >= 0 && k < width) dst[k] = k < len ? src[k] : 0.f;
        }
    }
}

__global__ __launch_bounds__(256)
void window_assemble_kernel(WindowArgs a, WindowDims d, const float* __restrict__ ppg, const float* __restrict__ lft,
                            const float* __restrict__ sine, float* __restrict__ ppg_out, float* __restrict__ lft_out,
                            float* __restrict__ sine_out) {
    __shared__ float tile[WN_TILE * WN_PITCH];
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x;
    if (blk < 2 * d.n_sig) {                        // ---- lft, then the excitation: row b, chunk
        const bool second = blk >= d.n_sig;
        if (second) blk -= d.n_sig;
        const int chunk = (int)(blk % (unsigned)d.sig_chunks), b = (int)(blk / (unsigned)d.sig_chunks);
        const int W = d.width * d.hop;
        padded_piece((second ? sine : lft) + a.sig_off[b], (second ? sine_out : lft_out) + (long)b * W,
                     a.frames[b] * d.hop, W, chunk, tid);
        return;
    }
    blk -= 2 * d.n_sig;                             // ---- ppg: a 64 (time) x 64 (channel) tile of row b
    const int C = d.C, width = d.width;
    const int per_row = d.tiles_t * d.tiles_c;
    const int b = (int)(blk / (unsigned)per_row), q = (int)(blk % (unsigned)per_row);
    const int c0 = (q / d.tiles_t) * WN_TILE, t0 = (q % d.tiles_t) * WN_TILE;
    const int len = a.frames[b];
    const bool live = t0 < len;                     // (uniform per block) a tile past the slice's end is all padding
    if (live) {
        const float* s = ppg + a.ppg_off[b];
        if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
            const int cl = tid & 15, tl = tid >> 4;
            const int c = c0 + 4 * cl;
            #pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int tt = tl + 16 * p, t = t0 + tt;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t < len && c < C) v = *reinterpret_cast<const float4*>(s + (long)t * C + c);   // (C % 4 == 0: c + 3 < C)
                float* w = tile + (4 * cl) * WN_PITCH + tt;
                w[0] = v.x; w[WN_PITCH] = v.y; w[2 * WN_PITCH] = v.z; w[3 * WN_PITCH] = v.w;
            }
        } else {
            const int cc = tid & 63, tl = tid >> 6;
            const int c = c0 + cc;
            #pragma unroll 4
            for (int p = 0; p < 16; ++p) {
                const int tt = tl + 4 * p, t = t0 + tt;
                tile[cc * WN_PITCH + tt] = (t < len && c < C) ? s[(long)t * C + c] : 0.f;
            }
        }
        __syncthreads();
    }
    const int tq = tid & 15, cr = tid >> 4;
    const int t = t0 + 4 * tq;
    if (t >= width) return;
    #pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int cc = cr + 16 * p, c = c0 + cc;
        if (c >= C) break;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const float* r = tile + cc * WN_PITCH + 4 * tq;             // (the fill wrote zeros at t >= len)
            #pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = r[e];
        }
        float* o = ppg_out + ((long)b * C + c) * width + t;
        if (t + 3 < width && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            #pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < width) o[e] = v[e];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- stitch

enum : int { WS_NONE = 0, WS_STAGE = 1, WS_FROM_STAGE = 2, WS_FROM_Y = 3, WS_SKIP = 4 };

// One row of a stitch launch, in samples of its own y row.  The left zone is [zl0, zl1), the right one [zr0, zr1)
// (empty when the side has no boundary); [lo, hi) is what the row reads: the run it writes plus the zones it stages.
struct StitchArgs {
    long dst_off[WN_MAX];                           // where the row's written run starts in the destinations
    long lsrc[WN_MAX], rsrc[WN_MAX];                // the zone's first sample: in `stage` (STAGE, FROM_STAGE) or in `y` (FROM_Y)
    int zl0[WN_MAX], zl1[WN_MAX], zr0[WN_MAX], zr1[WN_MAX];
    int modes[WN_MAX];                              // left | right << 4
    int utt[WN_MAX];                                // entry of `report`
};

typedef short short8 __attribute__((ext_vector_type(8)));

// decode.to_pcm16 for one float64 sample: rint(v * 32767.0) saturated to [-32768, 32767]; NaN gives 0.
__device__ __forceinline__ short pcm16_of(double v) {
    if (v != v) return 0;
    double r = __builtin_rint(v * 32767.0);
    r = r < -32768.0 ? -32768.0 : (r > 32767.0 ? 32767.0 : r);
    return (short)(int)r;
}

// pcm16_tally of fastsvc_decodeio.hip: what the conversion of the float32 sample hides.
constexpr float PCM16_CLIPS_FROM = 0x1.000102p+0f;             // bits 0x3f800081
constexpr float PCM16_CLIPS_DOWN_FROM = -0x1.000302p+0f;       // bits 0xbf800181

__device__ __forceinline__ void tally(float y, unsigned& counts, unsigned& maxbits) {
    const unsigned mag = __float_as_uint(y) & 0x7fffffffu;
    const bool finite = mag < 0x7f800000u;
    const bool clips = y >= PCM16_CLIPS_FROM || y <= PCM16_CLIPS_DOWN_FROM;        // (false for a NaN)
    counts += finite ? (clips ? 0x10000u : 0u) : 1u;
    maxbits = (finite && mag > maxbits) ? mag : maxbits;
}

// A lane owns 8 consecutive samples of the row's written run, cut so that destination element dst_off + 8 g is the
// first of piece g when dst_off is a multiple of 8 (then every whole piece is one 16-byte int16 store and two 16-byte
// float32 stores); otherwise the pieces are shifted by dst_off % 8 and the clipped head and tail go out sample by sample.
// Samples of a zone the row only stages precede / follow the run and are handled by the lanes of an extra head / tail
// range: the lane index space covers [lo, hi) of the row, the run [run_lo, run_hi) inside it.
template <bool CHECK>
__global__ __launch_bounds__(256)
void window_stitch_kernel(StitchArgs a, const float* __restrict__ y, long row0, int width, int half,
                          float* __restrict__ stage, short* __restrict__ dst16, float* __restrict__ dstf,
                          fastsvc_row_report* __restrict__ report) {
    __shared__ unsigned red[2][4];
    const int b = blockIdx.y;
    const int lm = a.modes[b] & 15, rm = a.modes[b] >> 4;
    const int zl0 = a.zl0[b], zl1 = a.zl1[b], zr0 = a.zr0[b], zr1 = a.zr1[b];
    const bool lblend = lm == WS_FROM_STAGE || lm == WS_FROM_Y, rblend = rm == WS_FROM_STAGE || rm == WS_FROM_Y;
    const int run_lo = lblend ? zl0 : zl1, run_hi = rblend ? zr1 : zr0;        // the samples this row writes
    const int lo = lm == WS_STAGE ? zl0 : run_lo, hi = rm == WS_STAGE ? zr1 : run_hi;
    const long d0 = a.dst_off[b];
    const int s = (int)(d0 & 7);
    // piece g covers run samples [8 g - s, 8 g - s + 8) + run_lo; the staged head needs (run_lo - lo) more samples in front
    const int head = run_lo - lo;
    const int shift = ((head + s + 7) / 8) * 8;                                 // whole pieces in front of the run's piece 0
    if ((long)blockIdx.x * 2048 - shift + run_lo - s >= hi) return;             // (uniform: the block starts past the row)
    const long x0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8 - shift - s + run_lo;
    const float* yr = y + (row0 + b) * (long)width;
    const double fh = (double)(2 * half);
    unsigned counts = 0, maxbits = 0;
    if (x0 < hi && x0 + 8 > lo) {
        if (x0 >= zl1 && x0 + 8 <= zr0 && x0 >= run_lo && x0 + 8 <= run_hi) {   // a whole piece of the row's own samples
            float v[8];
            if ((reinterpret_cast<uintptr_t>(yr + x0) & 15) == 0) {
                const float4 p = *reinterpret_cast<const float4*>(yr + x0), q = *reinterpret_cast<const float4*>(yr + x0 + 4);
                v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w; v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
            } else {
                #pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = yr[x0 + e];
            }
            const long o = d0 + (x0 - run_lo);
            if (CHECK) {
                #pragma unroll
                for (int e = 0; e < 8; ++e) tally(v[e], counts, maxbits);
            }
            if (dst16) {
                short8 w;
                #pragma unroll
                for (int e = 0; e < 8; ++e) w[e] = pcm16_of((double)v[e]);
                if ((reinterpret_cast<uintptr_t>(dst16 + o) & 15) == 0) {
                    *reinterpret_cast<short8*>(dst16 + o) = w;
                } else {
                    #pragma unroll
                    for (int e = 0; e < 8; ++e) dst16[o + e] = w[e];
                }
            }
            if (dstf) {
                if ((reinterpret_cast<uintptr_t>(dstf + o) & 15) == 0) {
                    *reinterpret_cast<float4*>(dstf + o) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(dstf + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
                } else {
                    #pragma unroll
                    for (int e = 0; e < 8; ++e) dstf[o + e] = v[e];
                }
            }
        } else {
            #pragma unroll 1
            for (int e = 0; e < 8; ++e) {
                const long x = x0 + e;
                if (x < lo || x >= hi) continue;
                const float own = yr[x];
                double v;
                if (x < zl1 && x >= zl0) {                                      // left zone: this row is the RIGHT window
                    const long j = x - zl0;
                    if (lm == WS_STAGE) { stage[a.lsrc[b] + j] = own; continue; }
                    const float other = lm == WS_FROM_Y ? y[a.lsrc[b] + j] : stage[a.lsrc[b] + j];
                    const double w = ((double)j + 0.5) / fh;
                    const double p = (1.0 - w) * (double)other;
                    const double q = w * (double)own;
                    v = p + q;
                } else if (x >= zr0 && x < zr1) {                               // right zone: this row is the LEFT window
                    const long j = x - zr0;
                    if (rm == WS_STAGE) { stage[a.rsrc[b] + j] = own; continue; }
                    const float other = rm == WS_FROM_Y ? y[a.rsrc[b] + j] : stage[a.rsrc[b] + j];
                    const double w = ((double)j + 0.5) / fh;
                    const double p = (1.0 - w) * (double)own;
                    const double q = w * (double)other;
                    v = p + q;
                } else {
                    v = (double)own;
                }
                const long o = d0 + (x - run_lo);                               // (x is in the run: staged samples left above)
                const float vf = (float)v;
                if (CHECK) tally(vf, counts, maxbits);
                if (dst16) dst16[o] = pcm16_of(v);
                if (dstf) dstf[o] = vf;
            }
        }
    }
    if (!CHECK) return;
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        counts += __shfl_down(counts, o);
        const unsigned m = __shfl_down(maxbits, o);
        maxbits = m > maxbits ? m : maxbits;
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = counts;
        red[1][threadIdx.x >> 6] = maxbits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0, m = 0;
        #pragma unroll
        for (int w = 0; w < 4; ++w) {
            c += red[0][w];
            m = red[1][w] > m ? red[1][w] : m;
        }
        fastsvc_row_report* r = report + a.utt[b];
        if (c & 0xffffu) atomicAdd(&r->nonfinite, (int)(c & 0xffffu));
        if (c >> 16) atomicAdd(&r->clipped, (int)(c >> 16));
        if (m) atomicMax(reinterpret_cast<unsigned*>(&r->max_abs), m);
    }
}

int invalid(const char* fmt, long a = 0, long b = 0, long c = 0, long e = 0) {
    char buf[240];
    snprintf(buf, sizeof buf, fmt, a, b, c, e);
    return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
}

}  // namespace

extern "C" {

int fastsvc_window_launch_count(int32_t R) { return R < 1 ? 0 : (R + WN_MAX - 1) / WN_MAX; }

int fastsvc_window_assemble(const float* ppg, int64_t ppg_elems, const float* lft, const float* sine, int64_t sig_elems,
                            const int64_t* ppg_off, const int64_t* sig_off, const int32_t* n_frames,
                            float* ppg_out, float* lft_out, float* sine_out,
                            int32_t R, int32_t C, int32_t hop, int32_t width, void* stream_) {
    if (!ppg || !lft || !sine || !ppg_off || !sig_off || !n_frames || !ppg_out || !lft_out || !sine_out)
        return invalid("fastsvc_window_assemble: null pointer");
    if (R < 1 || C < 1 || hop < 1 || width < 1 || ppg_elems < 0 || sig_elems < 0)
        return invalid("fastsvc_window_assemble: size out of range (R %ld, C %ld, hop %ld, width %ld)", R, C, hop, width);
    if ((int64_t)width * hop > INT32_MAX || (int64_t)width * C > INT32_MAX)
        return invalid("fastsvc_window_assemble: row too large (width %ld, hop %ld, C %ld)", width, hop, C);
    const void* ptrs[] = {ppg, lft, sine, ppg_out, lft_out, sine_out};
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 3) return invalid("fastsvc_window_assemble: pointers must be 4-byte aligned");
    for (int r = 0; r < R; ++r) {
        const int64_t n = n_frames[r];
        if (n < 0 || n > width)
            return invalid("fastsvc_window_assemble: row %ld has %ld frames, outside [0, width %ld]", r, n, width);
        if (ppg_off[r] < 0 || ppg_off[r] > ppg_elems || n * C > ppg_elems - ppg_off[r])
            return invalid("fastsvc_window_assemble: row %ld: ppg slice [%ld, +%ld) leaves its buffer", r, ppg_off[r], n * C);
        if (sig_off[r] < 0 || sig_off[r] > sig_elems || n * hop > sig_elems - sig_off[r])
            return invalid("fastsvc_window_assemble: row %ld: sample slice [%ld, +%ld) leaves its buffer", r, sig_off[r], n * hop);
    }
    const int64_t W = (int64_t)width * hop;
    WindowDims d;
    d.C = C; d.hop = hop; d.width = width;
    d.sig_chunks = row_chunks(W);
    d.tiles_t = (width + WN_TILE - 1) / WN_TILE;
    d.tiles_c = (C + WN_TILE - 1) / WN_TILE;
    const int64_t per_row = 2 * (int64_t)d.sig_chunks + (int64_t)d.tiles_t * d.tiles_c;
    if (per_row * (R < WN_MAX ? R : WN_MAX) > INT32_MAX) return invalid("fastsvc_window_assemble: grid too large");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < R; b0 += WN_MAX) {
        const int nb = R - b0 < WN_MAX ? R - b0 : WN_MAX;
        WindowArgs a;
        for (int i = 0; i < WN_MAX; ++i) {
            const bool on = i < nb;
            a.frames[i] = on ? n_frames[b0 + i] : 0;
            a.ppg_off[i] = on ? (long)ppg_off[b0 + i] : 0;
            a.sig_off[i] = on ? (long)sig_off[b0 + i] : 0;
        }
        d.n_sig = (unsigned)nb * (unsigned)d.sig_chunks;
        d.n_tile = (unsigned)nb * (unsigned)(d.tiles_t * d.tiles_c);
        hipLaunchKernelGGL(window_assemble_kernel, dim3((unsigned)(per_row * nb)), dim3(256), 0, stream,
                           a, d, ppg, lft, sine, ppg_out + (long)b0 * C * width, lft_out + (long)b0 * W, sine_out + (long)b0 * W);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK
                                           : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_window_assemble: launch failed");
}

int fastsvc_window_stitch(const float* y, int32_t B, int32_t width, const int32_t* n_samples,
                          const int32_t* core_lo, const int32_t* core_hi, int32_t half,
                          const int32_t* left_mode, const int32_t* right_mode, const int64_t* left_src, const int64_t* right_src,
                          float* stage, int64_t stage_elems, const int64_t* dst_off, int16_t* dst16, float* dstf,
                          int64_t dst_elems, const int32_t* utt, fastsvc_row_report* report, int32_t n_utts, void* stream_) {
    if (!y || !n_samples || !core_lo || !core_hi || !left_mode || !right_mode || !left_src || !right_src || !dst_off)
        return invalid("fastsvc_window_stitch: null pointer");
    if (!dst16 && !dstf) return invalid("fastsvc_window_stitch: no destination");
    if (B < 1 || width < 1 || half < 0 || half > (1 << 28) || stage_elems < 0 || dst_elems < 0 || (report && (!utt || n_utts < 1)))
        return invalid("fastsvc_window_stitch: size out of range (B %ld, width %ld, half %ld)", B, width, half);
    if ((reinterpret_cast<uintptr_t>(y) & 3) || (reinterpret_cast<uintptr_t>(stage) & 3) || (reinterpret_cast<uintptr_t>(dstf) & 3) ||
            (reinterpret_cast<uintptr_t>(dst16) & 1))
        return invalid("fastsvc_window_stitch: misaligned pointer");
    const int64_t y_elems = (int64_t)B * width;
    int maxspan = 0;
    std::vector<std::pair<int64_t, int64_t>> runs;    // [first, last) destination elements of every row that writes
    runs.reserve(B);
    // per row: zones clipped to the row's samples, then every range the kernel touches is checked here
    struct Z { int zl0, zl1, zr0, zr1, lo, hi, run_lo, run_hi; };
    auto zones = [&](int r) {
        Z z;
        const int lm = left_mode[r], rm = right_mode[r], n = n_samples[r];
        z.zl0 = lm != WS_NONE ? core_lo[r] - half : core_lo[r];
        z.zl1 = lm != WS_NONE ? (core_lo[r] + half < n ? core_lo[r] + half : n) : core_lo[r];
        z.zr0 = rm != WS_NONE ? core_hi[r] - half : core_hi[r];
        z.zr1 = rm != WS_NONE ? (core_hi[r] + half < n ? core_hi[r] + half : n) : core_hi[r];
        if (z.zr0 < z.zl1) z.zr0 = z.zl1;             // (a last window shorter than half a zone: its core lies inside the left zone)
        if (z.zr1 < z.zr0) z.zr1 = z.zr0;
        const bool lb = lm == WS_FROM_STAGE || lm == WS_FROM_Y, rb = rm == WS_FROM_STAGE || rm == WS_FROM_Y;
        z.run_lo = lb ? z.zl0 : z.zl1;
        z.run_hi = rb ? z.zr1 : z.zr0;
        z.lo = lm == WS_STAGE ? z.zl0 : z.run_lo;
        z.hi = rm == WS_STAGE ? z.zr1 : z.run_hi;
        return z;
    };
    for (int r = 0; r < B; ++r) {
        const int lm = left_mode[r], rm = right_mode[r], n = n_samples[r];
        if (lm < 0 || lm > WS_SKIP || rm < 0 || rm > WS_SKIP) return invalid("fastsvc_window_stitch: row %ld: unknown mode", r);
        if (half == 0 && (lm != WS_NONE || rm != WS_NONE)) return invalid("fastsvc_window_stitch: row %ld: a zone without a fade", r);
        if (n < 0 || n > width || core_lo[r] < 0 || core_hi[r] < core_lo[r] || core_hi[r] > n)
            return invalid("fastsvc_window_stitch: row %ld: core [%ld, %ld) outside its %ld samples", r, core_lo[r], core_hi[r], n);
        if (lm != WS_NONE && core_lo[r] - half < 0)
            return invalid("fastsvc_window_stitch: row %ld: the left zone starts before the row (core_lo %ld, half %ld)", r, core_lo[r], half);
        if (rm != WS_NONE && core_hi[r] - half < core_lo[r] && lm == WS_NONE)
            return invalid("fastsvc_window_stitch: row %ld: the right zone starts before the core", r);
        if (rm != WS_NONE && lm != WS_NONE && core_hi[r] - core_lo[r] < 2 * half)
            return invalid("fastsvc_window_stitch: row %ld: the core is shorter than the fade", r);
        const Z z = zones(r);
        const int64_t ll = z.zl1 - z.zl0, rl = z.zr1 - z.zr0;
        if ((lm == WS_STAGE || lm == WS_FROM_STAGE) && (left_src[r] < 0 || left_src[r] > stage_elems || ll > stage_elems - left_src[r] || !stage))
            return invalid("fastsvc_window_stitch: row %ld: left zone slot [%ld, +%ld) leaves the staging buffer", r, left_src[r], ll);
        if ((rm == WS_STAGE || rm == WS_FROM_STAGE) && (right_src[r] < 0 || right_src[r] > stage_elems || rl > stage_elems - right_src[r] || !stage))
            return invalid("fastsvc_window_stitch: row %ld: right zone slot [%ld, +%ld) leaves the staging buffer", r, right_src[r], rl);
        if (lm == WS_FROM_Y && (left_src[r] < 0 || left_src[r] > y_elems || ll > y_elems - left_src[r]))
            return invalid("fastsvc_window_stitch: row %ld: left neighbour samples [%ld, +%ld) leave y", r, left_src[r], ll);
        if (rm == WS_FROM_Y && (right_src[r] < 0 || right_src[r] > y_elems || rl > y_elems - right_src[r]))
            return invalid("fastsvc_window_stitch: row %ld: right neighbour samples [%ld, +%ld) leave y", r, right_src[r], rl);
        const int64_t run = z.run_hi - z.run_lo;
        if (run < 0 || dst_off[r] < 0 || dst_off[r] > dst_elems || run > dst_elems - dst_off[r])
            return invalid("fastsvc_window_stitch: row %ld: its run [%ld, +%ld) leaves the destination", r, dst_off[r], run);
        if (report && (utt[r] < 0 || utt[r] >= n_utts))
            return invalid("fastsvc_window_stitch: row %ld: utterance %ld outside [0, %ld)", r, utt[r], n_utts);
        const int span = z.hi - z.lo + 24;            // (the lanes start up to 2 * 7 + 7 samples in front of the row's first)
        maxspan = span > maxspan ? span : maxspan;
        if (run > 0) runs.push_back({(int64_t)dst_off[r], (int64_t)dst_off[r] + run});
    }
    // two rows that wrote the same destination samples would race: the runs of one call must be disjoint
    std::sort(runs.begin(), runs.end());
    for (size_t i = 1; i < runs.size(); ++i)
        if (runs[i].first < runs[i - 1].second)
            return invalid("fastsvc_window_stitch: the runs [%ld, %ld) and [%ld, %ld) of two rows overlap in the destination",
                           runs[i - 1].first, runs[i - 1].second, runs[i].first, runs[i].second);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned gx = (unsigned)(((long)maxspan + 2047) / 2048);
    for (int b0 = 0; b0 < B; b0 += WN_MAX) {
        const int nb = B - b0 < WN_MAX ? B - b0 : WN_MAX;
        StitchArgs a;
        for (int i = 0; i < WN_MAX; ++i) {
            const bool on = i < nb;
            Z z = {0, 0, 0, 0, 0, 0, 0, 0};
            if (on) z = zones(b0 + i);
            a.zl0[i] = z.zl0; a.zl1[i] = z.zl1; a.zr0[i] = z.zr0; a.zr1[i] = z.zr1;
            a.modes[i] = on ? (left_mode[b0 + i] | (right_mode[b0 + i] << 4)) : 0;
            a.dst_off[i] = on ? (long)dst_off[b0 + i] : 0;
            a.lsrc[i] = on ? (long)left_src[b0 + i] : 0;
            a.rsrc[i] = on ? (long)right_src[b0 + i] : 0;
            a.utt[i] = (on && report) ? utt[b0 + i] : 0;
        }
        if (report)
            hipLaunchKernelGGL(window_stitch_kernel<true>, dim3(gx, (unsigned)nb), dim3(256), 0, stream, a, y, (long)b0, width,
                               half, stage, reinterpret_cast<short*>(dst16), dstf, report);
        else
            hipLaunchKernelGGL(window_stitch_kernel<false>, dim3(gx, (unsigned)nb), dim3(256), 0, stream, a, y, (long)b0, width,
                               half, stage, reinterpret_cast<short*>(dst16), dstf, report);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK
                                           : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_window_stitch: launch failed");
}

}  // extern "C"
