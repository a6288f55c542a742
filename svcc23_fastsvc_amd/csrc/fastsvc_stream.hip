// fastsvc_stream.hip - the device state of live streams on gfx950 (decode.StreamSession): features arrive a few frames
// at a time, for many streams at once, and windows are cut out of what has arrived.
//
//   stream_push       per stream, n frames (0 allowed) of one packed upload buffer - time-major ppg n x C, then f0 n,
//                     then lft n x hop - are appended to the stream's RINGS: ppg (cap x C, time-major), lft (cap x hop)
//                     and the excitation (cap x hop), which the same launch synthesises.  Frame p of a stream lives at
//                     ring index p % cap; a chunk is at most cap frames, so it wraps at most once.  With a null exc_ring
//                     the slice holds no f0 - ppg, then n x hop samples - and the launch only copies (stream_append_kernel):
//                     a session that makes the F0 itself synthesises when the frames are final (fastsvc_stream_f0.hip).
//   stream_assemble   fastsvc_window_assemble's outputs for rows (stream, first_frame, n_frames) read from the rings
//                     modulo cap: ppg transposed to channel-major, lft and the excitation copied, the tails zero.
//
// The reference decodes whole files (decode_fastsvc.py:150-200) and has no counterpart.  Both kernels are data movement
// plus one sin per sample; they have no tunables.
//
// Excitation.  The whole-utterance synthesis (fastsvc_signal.hip) scans hop * rad_f over all frames; here the prefix is
// carried: C_{f+1} = frac(C_f + hop * rad_f) in float64, the recurrence frame_phase_kernel itself runs inside a lane's
// segment.  hop * rad_f is a float32 times a small integer and the partial sums stay far below 2^53 ulps of it, so every
// add is exact and the carried prefix has the bits of the scan.  One lane of every block runs the
// recurrence over the chunk (at most SP_MAX_PUSH adds) into LDS; after a barrier all lanes write samples with the closed
// form of fastsvc_signal.inc.  The stream's phase lives in a float64 pair, phase[slot][2]: a launch READS entry
// `parity` and block 0 WRITES entry `parity ^ 1`, because the blocks of one stream all read the phase and are not
// ordered against the one that stores the new one.  `first` starts the phase at 0 without reading: opening a slot needs
// no memset.  Noise is keyed by the stream's seed and the ABSOLUTE sample index pos * hop + k: it does not depend on
// the slot or on how the stream was cut into pushes.
//
// Descriptors travel IN the kernel arguments, 64 streams / rows per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "fastsvc_hip.h"

namespace fastsvc {
int set_last_error(int code, const char* msg);      // fastsvc_plan.cpp: the text fastsvc_last_error() returns
}

namespace {

#include "fastsvc_signal.inc"      // frame_rad, phase_step, sine_sample: shared with fastsvc_signal.hip

constexpr int SP_MAX = 64;                          // streams / rows per launch (the arguments hold their descriptors)
constexpr int SP_MAX_PUSH = 1024;                   // frames of one chunk (their prefixes: 8 KiB of LDS)
constexpr int SP_MAX_BLOCKS = 64;                   // blocks per stream of a push (grid-stride beyond)
constexpr int SP_TILE = 64;
constexpr int SP_PITCH = 65;
constexpr int SP_CHUNK = 1024;                      // elements of a row one copy block covers (256 lanes x 16 bytes)

struct PushArgs {
    long up_off[SP_MAX];                            // first element of the stream's slice of the upload buffer
    long pos[SP_MAX];                               // frames the stream held before this push
    unsigned long long seed[SP_MAX];
    int n[SP_MAX];
    int slot[SP_MAX];
    int flags[SP_MAX];                              // bit 0: first push of the stream; bit 1: the phase entry to read
};

struct PushDims {
    int C, hop, cap;
    float sr, sine_amp, noise_amp;
};

// Group g of a contiguous copy of `total` elements from src to ring[(start + e) % ring_len]: elements [4 g, 4 g + 4).
// start < ring_len and total <= ring_len, so one subtraction wraps.
__device__ __forceinline__ void ring_put4(const float* __restrict__ src, float* __restrict__ ring, long ring_len, long start,
                                          long total, long g) {
    const long e0 = 4 * g;
    long d0 = start + e0;
    if (d0 >= ring_len) d0 -= ring_len;
    if (e0 + 4 <= total && d0 + 4 <= ring_len && (reinterpret_cast<uintptr_t>(src + e0) & 15) == 0 &&
            (reinterpret_cast<uintptr_t>(ring + d0) & 15) == 0) {
        *reinterpret_cast<float4*>(ring + d0) = *reinterpret_cast<const float4*>(src + e0);
        return;
    }
    #pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e0 + e >= total) break;
        long d = d0 + e;
        if (d >= ring_len) d -= ring_len;
        ring[d] = src[e0 + e];
    }
}

__global__ __launch_bounds__(256)
void stream_push_kernel(PushArgs a, PushDims d, const float* __restrict__ up, float* __restrict__ ppg_ring,
                        float* __restrict__ lft_ring, float* __restrict__ exc_ring, double* __restrict__ phase) {
    __shared__ double pre[SP_MAX_PUSH];
    __shared__ float rads[SP_MAX_PUSH];
    const int b = blockIdx.y;
    const int n = a.n[b];
    if (n == 0) return;                             // (uniform per block)
    const int slot = a.slot[b], flags = a.flags[b];
    const int C = d.C, hop = d.hop, cap = d.cap;
    const float* src = up + a.up_off[b];
    const float* f0 = src + (long)n * C;
    const float* lft = f0 + n;
    for (int f = threadIdx.x; f < n; f += 256) rads[f] = frame_rad(f0[f], d.sr);      // (the lane below then waits on LDS only)
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = (flags & 1) ? 0.0 : phase[2 * slot + ((flags >> 1) & 1)];
        for (int f = 0; f < n; ++f) {
            pre[f] = c;
            c = phase_step(c, rads[f], hop);
        }
        if (blockIdx.x == 0) phase[2 * slot + (((flags >> 1) & 1) ^ 1)] = c;
    }
    __syncthreads();
    const long p0 = a.pos[b] % cap;
    const long np = (long)n * C, ns = (long)n * hop;
    const long gp = (np + 3) / 4, gs = (ns + 3) / 4;
    const long ring_p = (long)cap * C, ring_s = (long)cap * hop;
    float* rp = ppg_ring + slot * ring_p;
    float* rl = lft_ring + slot * ring_s;
    float* re = exc_ring + slot * ring_s;
    const uint64_t t0 = (uint64_t)a.pos[b] * (uint64_t)hop;         // the chunk's first sample in the stream
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < gp + 2 * gs; g += (long)gridDim.x * 256) {
        if (g < gp) {
            ring_put4(src, rp, ring_p, p0 * C, np, g);
        } else if (g < gp + gs) {
            ring_put4(lft, rl, ring_s, p0 * hop, ns, g - gp);
        } else {
            const long k0 = 4 * (g - gp - gs);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long k = k0 + e;
                if (k >= ns) break;
                const int fr = (int)(k / hop);
                const int j = (int)(k - (long)fr * hop);
                v[e] = sine_sample(f0[fr], pre[fr], j, d.sr, d.sine_amp, d.noise_amp, a.seed[b], t0 + (uint64_t)k);
            }
            long d0 = p0 * hop + k0;
            if (d0 >= ring_s) d0 -= ring_s;
            if (k0 + 4 <= ns && d0 + 4 <= ring_s && (reinterpret_cast<uintptr_t>(re + d0) & 15) == 0) {
                *reinterpret_cast<float4*>(re + d0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                #pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (k0 + e >= ns) break;
                    long x = d0 + e;
                    if (x >= ring_s) x -= ring_s;
                    re[x] = v[e];
                }
            }
        }
    }
}

// The push of a session that makes the F0 itself (StreamSession(f0="audio")): the slice is ppg n x C, then audio n x hop -
// no f0 - and nothing is synthesised: the excitation is made when the frames are final (fastsvc_stream_f0.hip).  The
// copies are stream_push_kernel's, through ring_put4.
__global__ __launch_bounds__(256)
void stream_append_kernel(PushArgs a, PushDims d, const float* __restrict__ up, float* __restrict__ ppg_ring,
                          float* __restrict__ sig_ring) {
    const int b = blockIdx.y;
    const int n = a.n[b];
    if (n == 0) return;                             // (uniform per block)
    const int slot = a.slot[b];
    const int C = d.C, hop = d.hop, cap = d.cap;
    const float* src = up + a.up_off[b];
    const float* sig = src + (long)n * C;
    const long p0 = a.pos[b] % cap;
    const long np = (long)n * C, ns = (long)n * hop;
    const long gp = (np + 3) / 4, gs = (ns + 3) / 4;
    const long ring_p = (long)cap * C, ring_s = (long)cap * hop;
    float* rp = ppg_ring + slot * ring_p;
    float* rs = sig_ring + slot * ring_s;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < gp + gs; g += (long)gridDim.x * 256) {
        if (g < gp) ring_put4(src, rp, ring_p, p0 * C, np, g);
        else ring_put4(sig, rs, ring_s, p0 * hop, ns, g - gp);
    }
}

// ---------------------------------------------------------------------------------------------------------- assemble

struct RowArgs {
    int slot[SP_MAX];
    int first[SP_MAX];                              // ring index of the row's first frame: first_frame % cap
    int frames[SP_MAX];
};

struct RowDims {
    int C, hop, width, cap;
    int sig_chunks;                                 // copy blocks per row and signal
    int tiles_t, tiles_c;                           // ppg tiles per row
    unsigned n_sig;
};

inline int row_chunks(long len) { return (int)((len + 3 + SP_CHUNK - 1) / SP_CHUNK); }

// fastsvc_window.hip's padded_piece with the source in a ring: element k of the row is ring[(start + k) % ring_len] for
// k < len and 0 from len on.  Lane `tid` of copy block `chunk` owns one 16-byte aligned piece of dst[0, width).
__device__ __forceinline__ void ring_piece(const float* __restrict__ ring, long ring_len, long start, float* __restrict__ dst,
                                           int len, int width, int chunk, int tid) {
    const int s = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
    const long k0 = ((long)chunk * 256 + tid) * 4 - s;
    if (k0 >= width) return;
    auto at = [&](long k) { long x = start + k; if (x >= ring_len) x -= ring_len; return ring[x]; };
    if (k0 >= 0 && k0 + 4 <= width) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + 4 <= len) {
            long x = start + k0;
            if (x >= ring_len) x -= ring_len;
            if (x + 4 <= ring_len && (reinterpret_cast<uintptr_t>(ring + x) & 15) == 0) {
                v = *reinterpret_cast<const float4*>(ring + x);
            } else {
                v.x = at(k0); v.y = at(k0 + 1); v.z = at(k0 + 2); v.w = at(k0 + 3);
            }
        } else if (k0 < len) {                      // (the piece that holds the row's end: 1 - 3 elements of it)
            v.x = at(k0);
            if (k0 + 1 < len) v.y = at(k0 + 1);
            if (k0 + 2 < len) v.z = at(k0 + 2);
        }
        *reinterpret_cast<float4*>(dst + k0) = v;
    } else {
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long k = k0 + e;
            if (k >= 0 && k < width) dst[k] = k < len ? at(k) : 0.f;
        }
    }
}

// Block roles by blockIdx.x range, as in window_assemble_kernel: lft copies, excitation copies, 64 x 64 ppg tiles.
__global__ __launch_bounds__(256)
void stream_assemble_kernel(RowArgs a, RowDims d, const float* __restrict__ ppg_ring, const float* __restrict__ lft_ring,
                            const float* __restrict__ exc_ring, float* __restrict__ ppg_out, float* __restrict__ lft_out,
                            float* __restrict__ sine_out) {
    __shared__ float tile[SP_TILE * SP_PITCH];
    const int tid = threadIdx.x;
    unsigned blk = blockIdx.x;
    if (blk < 2 * d.n_sig) {                        // ---- lft, then the excitation: row b, chunk
        const bool second = blk >= d.n_sig;
        if (second) blk -= d.n_sig;
        const int chunk = (int)(blk % (unsigned)d.sig_chunks), b = (int)(blk / (unsigned)d.sig_chunks);
        const int W = d.width * d.hop;
        const long ring_s = (long)d.cap * d.hop;
        ring_piece((second ? exc_ring : lft_ring) + a.slot[b] * ring_s, ring_s, (long)a.first[b] * d.hop,
                   (second ? sine_out : lft_out) + (long)b * W, a.frames[b] * d.hop, W, chunk, tid);
        return;
    }
    blk -= 2 * d.n_sig;                             // ---- ppg: a 64 (time) x 64 (channel) tile of row b
    const int C = d.C, width = d.width, cap = d.cap;
    const int per_row = d.tiles_t * d.tiles_c;
    const int b = (int)(blk / (unsigned)per_row), q = (int)(blk % (unsigned)per_row);
    const int c0 = (q / d.tiles_t) * SP_TILE, t0 = (q % d.tiles_t) * SP_TILE;
    const int len = a.frames[b], first = a.first[b];
    const bool live = t0 < len;                     // (uniform per block) a tile past the row's end is all padding
    if (live) {
        const float* s = ppg_ring + (long)a.slot[b] * cap * C;
        if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
            const int cl = tid & 15, tl = tid >> 4;
            const int c = c0 + 4 * cl;
            #pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int tt = tl + 16 * p, t = t0 + tt;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t < len && c < C) {             // (C % 4 == 0: c + 3 < C; t < len <= cap: one subtraction wraps)
                    int fr = first + t;
                    if (fr >= cap) fr -= cap;
                    v = *reinterpret_cast<const float4*>(s + (long)fr * C + c);
                }
                float* w = tile + (4 * cl) * SP_PITCH + tt;
                w[0] = v.x; w[SP_PITCH] = v.y; w[2 * SP_PITCH] = v.z; w[3 * SP_PITCH] = v.w;
            }
        } else {
            const int cc = tid & 63, tl = tid >> 6;
            const int c = c0 + cc;
            #pragma unroll 4
            for (int p = 0; p < 16; ++p) {
                const int tt = tl + 4 * p, t = t0 + tt;
                float v = 0.f;
                if (t < len && c < C) {
                    int fr = first + t;
                    if (fr >= cap) fr -= cap;
                    v = s[(long)fr * C + c];
                }
                tile[cc * SP_PITCH + tt] = v;
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
            const float* r = tile + cc * SP_PITCH + 4 * tq;             // (the fill wrote zeros at t >= len)
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

int invalid(const char* fmt, long a = 0, long b = 0, long c = 0, long e = 0) {
    char buf[240];
    snprintf(buf, sizeof buf, fmt, a, b, c, e);
    return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
}

// what both entry points ask of the rings
int check_rings(const char* who, const void* ppg_ring, const void* lft_ring, const void* exc_ring, int32_t n_streams,
                int32_t cap, int32_t C, int32_t hop) {
    char buf[200];
    if (!ppg_ring || !lft_ring || !exc_ring) {
        snprintf(buf, sizeof buf, "%s: null ring pointer", who);
        return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
    }
    if (n_streams < 1 || cap < 4 || (cap & 3) || C < 1 || hop < 1 || (int64_t)cap * C > INT32_MAX || (int64_t)cap * hop > INT32_MAX ||
            (int64_t)n_streams * cap * (C > hop ? C : hop) > ((int64_t)1 << 40)) {
        snprintf(buf, sizeof buf, "%s: size out of range (n_streams %d, cap %d: a multiple of 4, C %d, hop %d)", who, n_streams, cap, C, hop);
        return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
    }
    const void* ptrs[] = {ppg_ring, lft_ring, exc_ring};
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15) {
            snprintf(buf, sizeof buf, "%s: the rings must be 16-byte aligned", who);
            return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
        }
    return FASTSVC_OK;
}

}  // namespace

extern "C" {

int fastsvc_stream_launch_count(int32_t R) { return R < 1 ? 0 : (R + SP_MAX - 1) / SP_MAX; }

int fastsvc_stream_push(const float* upload, int64_t upload_elems, int32_t S, const int32_t* stream, const int32_t* n,
                        const int64_t* up_off, const int64_t* pos, const int32_t* first, const int32_t* parity,
                        const uint64_t* seed, float* ppg_ring, float* lft_ring, float* exc_ring, double* phase,
                        int32_t n_streams, int32_t cap, int32_t max_push, int32_t C, int32_t hop,
                        float sample_rate, float sine_amp, float noise_amp, void* stream_) {
    // a null exc_ring: no f0 in the slices and no synthesis (phase and seed are then not read and may be null)
    const bool synth = exc_ring != nullptr;
    if (!upload || !stream || !n || !up_off || !pos || !first || !parity || (synth && (!seed || !phase)))
        return invalid("fastsvc_stream_push: null pointer");
    if (const int rc = check_rings("fastsvc_stream_push", ppg_ring, lft_ring, synth ? exc_ring : lft_ring, n_streams, cap, C, hop)) return rc;
    if (S < 1 || upload_elems < 0 || max_push < 1 || max_push > SP_MAX_PUSH || max_push > cap || !(sample_rate > 0.f))
        return invalid("fastsvc_stream_push: size out of range (S %ld, max_push %ld: at most %ld and at most cap %ld)", S, max_push,
                       SP_MAX_PUSH, cap);
    if ((reinterpret_cast<uintptr_t>(upload) & 3) || (synth && (reinterpret_cast<uintptr_t>(phase) & 7)))
        return invalid("fastsvc_stream_push: misaligned pointer");
    int64_t most = 0;
    for (int i = 0; i < S; ++i) {
        const int64_t s = stream[i], k = n[i];
        if (s < 0 || s >= n_streams) return invalid("fastsvc_stream_push: entry %ld: stream %ld outside [0, %ld)", i, s, n_streams);
        for (int j = 0; j < i; ++j)
            if (stream[j] == s) return invalid("fastsvc_stream_push: stream %ld is pushed twice in one call", s);
        if (k < 0 || k > max_push) return invalid("fastsvc_stream_push: stream %ld: %ld frames, outside [0, max_push %ld]", s, k, max_push);
        const int64_t need = k * ((int64_t)C + (synth ? 1 : 0) + hop);
        if (up_off[i] < 0 || up_off[i] > upload_elems || need > upload_elems - up_off[i])
            return invalid("fastsvc_stream_push: stream %ld: its slice [%ld, +%ld) leaves the upload buffer of %ld elements", s, up_off[i],
                           need, upload_elems);
        if (pos[i] < 0 || pos[i] > ((int64_t)1 << 40)) return invalid("fastsvc_stream_push: stream %ld: position %ld out of range", s, pos[i]);
        if ((first[i] & ~1) || (parity[i] & ~1)) return invalid("fastsvc_stream_push: stream %ld: first and parity are 0 or 1", s);
        most = k > most ? k : most;
    }
    if (most == 0) return FASTSVC_OK;               // (nothing to append: no launch)
    const int64_t groups = (most * C + 3) / 4 + (synth ? 2 : 1) * ((most * hop + 3) / 4);
    int64_t gx = (groups + 255) / 256;
    gx = gx > SP_MAX_BLOCKS ? SP_MAX_BLOCKS : gx;
    PushDims d;
    d.C = C; d.hop = hop; d.cap = cap; d.sr = sample_rate; d.sine_amp = sine_amp; d.noise_amp = noise_amp;
    hipStream_t hs = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < S; b0 += SP_MAX) {
        const int nb = S - b0 < SP_MAX ? S - b0 : SP_MAX;
        PushArgs a;
        for (int i = 0; i < SP_MAX; ++i) {
            const bool on = i < nb;
            a.n[i] = on ? n[b0 + i] : 0;
            a.slot[i] = on ? stream[b0 + i] : 0;
            a.flags[i] = on ? (first[b0 + i] | (parity[b0 + i] << 1)) : 0;
            a.up_off[i] = on ? (long)up_off[b0 + i] : 0;
            a.pos[i] = on ? (long)pos[b0 + i] : 0;
            a.seed[i] = on && synth ? (unsigned long long)seed[b0 + i] : 0ull;
        }
        if (!synth) {
            hipLaunchKernelGGL(stream_append_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, hs, a, d, upload, ppg_ring, lft_ring);
            continue;
        }
        hipLaunchKernelGGL(stream_push_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, hs, a, d, upload, ppg_ring, lft_ring,
                           exc_ring, phase);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK
                                           : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_stream_push: launch failed");
}

int fastsvc_stream_assemble(const float* ppg_ring, const float* lft_ring, const float* exc_ring, int32_t n_streams, int32_t cap,
                            const int64_t* pos, const int32_t* stream, const int64_t* first_frame, const int32_t* n_frames,
                            float* ppg_out, float* lft_out, float* sine_out,
                            int32_t R, int32_t C, int32_t hop, int32_t width, void* stream_) {
    if (!pos || !stream || !first_frame || !n_frames || !ppg_out || !lft_out || !sine_out)
        return invalid("fastsvc_stream_assemble: null pointer");
    if (const int rc = check_rings("fastsvc_stream_assemble", ppg_ring, lft_ring, exc_ring, n_streams, cap, C, hop)) return rc;
    if (R < 1 || width < 1) return invalid("fastsvc_stream_assemble: size out of range (R %ld, width %ld)", R, width);
    if ((int64_t)width * hop > INT32_MAX || (int64_t)width * C > INT32_MAX)
        return invalid("fastsvc_stream_assemble: row too large (width %ld, hop %ld, C %ld)", width, hop, C);
    const void* outs[] = {ppg_out, lft_out, sine_out};
    for (const void* p : outs)
        if (reinterpret_cast<uintptr_t>(p) & 3) return invalid("fastsvc_stream_assemble: pointers must be 4-byte aligned");
    for (int r = 0; r < R; ++r) {
        const int64_t s = stream[r], k = n_frames[r], f = first_frame[r];
        if (s < 0 || s >= n_streams) return invalid("fastsvc_stream_assemble: row %ld: stream %ld outside [0, %ld)", r, s, n_streams);
        if (k < 0 || k > width || k > cap)
            return invalid("fastsvc_stream_assemble: row %ld has %ld frames, outside [0, min(width %ld, cap %ld)]", r, k, width, cap);
        if (pos[s] < 0 || f < 0 || f < pos[s] - cap || f > pos[s] || k > pos[s] - f)
            return invalid("fastsvc_stream_assemble: row %ld: frames [%ld, +%ld) are not retained by its stream, which holds the %ld before its position",
                           r, f, k, cap);
    }
    const int64_t W = (int64_t)width * hop;
    RowDims d;
    d.C = C; d.hop = hop; d.width = width; d.cap = cap;
    d.sig_chunks = row_chunks(W);
    d.tiles_t = (width + SP_TILE - 1) / SP_TILE;
    d.tiles_c = (C + SP_TILE - 1) / SP_TILE;
    const int64_t per_row = 2 * (int64_t)d.sig_chunks + (int64_t)d.tiles_t * d.tiles_c;
    if (per_row * (R < SP_MAX ? R : SP_MAX) > INT32_MAX) return invalid("fastsvc_stream_assemble: grid too large");
    hipStream_t hs = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < R; b0 += SP_MAX) {
        const int nb = R - b0 < SP_MAX ? R - b0 : SP_MAX;
        RowArgs a;
        for (int i = 0; i < SP_MAX; ++i) {
            const bool on = i < nb;
            a.frames[i] = on ? n_frames[b0 + i] : 0;
            a.slot[i] = on ? stream[b0 + i] : 0;
            a.first[i] = on ? (int)(first_frame[b0 + i] % cap) : 0;
        }
        d.n_sig = (unsigned)nb * (unsigned)d.sig_chunks;
        hipLaunchKernelGGL(stream_assemble_kernel, dim3((unsigned)(per_row * nb)), dim3(256), 0, hs,
                           a, d, ppg_ring, lft_ring, exc_ring, ppg_out + (long)b0 * C * width, lft_out + (long)b0 * W, sine_out + (long)b0 * W);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK
                                           : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_stream_assemble: launch failed");
}

}  // extern "C"
