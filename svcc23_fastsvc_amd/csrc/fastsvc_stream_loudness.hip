// fastsvc_stream_loudness.hip - the loudness of live streams from their raw audio, on gfx950
// (decode.StreamSession(loudness="audio")): the frames of a stream that have become FINAL are turned into the A-weighted
// log loudness of fastsvc_loudness.hip, straight into the stream's lft ring.
//
// The function.  A stream is an utterance of F frames whose audio is y[0, T), T = F hop, known only at
// the end.  P_f[k] is frame f's power as loudness_extract computes it on the whole audio (periodic Hann, 2048 samples
// centred on f hop, reflection at 0 and at T); the 80 dB floor of frame f hangs under the RUNNING maximum M_f = max over
// g <= f and all k of P_g[k] - the one departure from the whole-file function, which uses M_{F-1} everywhere; the rest
// (clamp, A-weighting, 10^(dB/20), mean over the bins, log(. + 1e-5), repeated hop times) is fastsvc_loudness.inc, shared
// with the whole-file kernels.  Frame f reads samples up to f hop + 1023: it is final once that many have arrived, and at
// the end every frame is final, with reflection at T.
//
//   stream_loudness_power    one block per (stream, newly final frame): reads the AUDIO ring (sample p at p % (cap hop),
//                            appended by stream_push) and writes the 1025-bin power row and the frame's maximum to scratch
//   stream_loudness_reduce   one block per (stream, newly final frame): M_f = max(carried maximum, maxima of this call's
//                            frames <= f) - a maximum of floats is exact, the order does not matter - then the value, hop
//                            samples of it into the lft ring at frame index f % cap
//
// Frame f's floor needs the maxima of earlier frames of the same call, so these are two launches (no grid barrier).  The
// carried maximum lives in a float pair, peak[slot][2]: a call READS entry `parity` and the block of the call's last
// frame WRITES entry `parity ^ 1`, because the blocks of one stream all read the carried maximum and are not ordered
// against the one that stores the new one - phase[slot][2]'s rule in fastsvc_stream.hip.  `first` starts the maximum at
// 0 without reading: opening a slot needs no memset.
//
// Descriptors travel IN the kernel arguments, 64 streams per launch.  Plain vector stores, no atomics, no tunables.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "fastsvc_hip.h"

namespace fastsvc {
int set_last_error(int code, const char* msg);      // fastsvc_plan.cpp: the text fastsvc_last_error() returns
}

namespace {

#include "fastsvc_loudness.inc"

constexpr int SL_MAX = 64;                          // streams per launch (the arguments hold their descriptors)
constexpr int SL_MAX_FRAMES = 2048;                 // frames of one stream a call finalises (a chunk of 1024 and the lag)

struct LoudArgs {
    long first[SL_MAX];                             // the stream's first frame of this call
    long samples[SL_MAX];                           // samples the stream's audio ring has received
    int n[SL_MAX];                                  // frames of this call
    int slot[SL_MAX];
    int flags[SL_MAX];                              // bit 0: the stream's first frame is among them (no carried maximum);
};                                                  // bit 1: the peak entry to read; bit 2: the stream has ended

struct LoudDims {
    int hop, cap, max_frames;
    float sr;
};

__global__ __launch_bounds__(256)
void stream_loudness_power_kernel(LoudArgs a, LoudDims d, const float* __restrict__ audio_ring, float* __restrict__ power,
                                  float* __restrict__ fmax) {
    __shared__ float re[LD_NFFT], im[LD_NFFT];
    __shared__ float wmax[4];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (j >= a.n[b]) return;                        // (uniform per block)
    const int slot = a.slot[b];
    const long ring_len = (long)d.cap * d.hop, T = a.samples[b];
    const bool ended = (a.flags[b] & 4) != 0;
    const float* ring = audio_ring + slot * ring_len;
    const long base = (a.first[b] + j) * d.hop - LD_NFFT / 2;
    loudness_frame_fft(re, im, tid, [&](int k) {
        long i = base + k;
        if (ended) i = reflect_index<long>(i, T);
        else if (i < 0) i = -i;
        // (a frame that is final before the end reads [f hop - 1024, f hop + 1024) < T; only frame 0's element 0 mirrors
        // to sample 1024, which may not have arrived when hop divides 1024 - its window weight is exactly 0)
        return i < T ? ring[i % ring_len] : 0.f;
    });
    const long row = (long)slot * d.max_frames + j;
    const float m = loudness_power_row(re, im, power + row * LD_NBINS, wmax, tid);
    if (tid == 0) fmax[row] = m;
}

__global__ __launch_bounds__(256)
void stream_loudness_reduce_kernel(LoudArgs a, LoudDims d, const float* __restrict__ power, const float* __restrict__ fmax,
                                   float* __restrict__ peak, float* __restrict__ lft_ring) {
    __shared__ float part[4];
    __shared__ float result;
    __shared__ float wmax[4];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = a.n[b];
    if (j >= n) return;                             // (uniform per block)
    const int slot = a.slot[b], flags = a.flags[b];
    const long row0 = (long)slot * d.max_frames;
    // the running maximum up to and including this frame
    float m = 0.f;
    if (tid == 0 && !(flags & 1)) m = peak[2 * slot + ((flags >> 1) & 1)];
    for (int g = tid; g <= j; g += 256) m = fmaxf(m, fmax[row0 + g]);
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (tid == 0 && j == n - 1) peak[2 * slot + (((flags >> 1) & 1) ^ 1)] = m;
    const float v = loudness_frame_value(power + (row0 + j) * LD_NBINS, m, d.sr, part, &result, tid);
    const long f = a.first[b] + j;
    float* orow = lft_ring + ((long)slot * d.cap + f % d.cap) * d.hop;
    for (int k = tid; k < d.hop; k += 256) orow[k] = v;
}

int invalid(const char* fmt, long a = 0, long b = 0, long c = 0, long e = 0) {
    char buf[240];
    snprintf(buf, sizeof buf, fmt, a, b, c, e);
    return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
}

}  // namespace

extern "C" {

size_t fastsvc_stream_loudness_scratch_bytes(int32_t n_streams, int32_t max_frames) {
    if (n_streams < 1 || max_frames < 1 || max_frames > SL_MAX_FRAMES) return 0;
    return (size_t)n_streams * max_frames * (LD_NBINS + 1) * sizeof(float);
}

int fastsvc_stream_loudness(const float* audio_ring, float* lft_ring, float* peak, void* scratch, int32_t S,
                            const int32_t* stream, const int64_t* first_frame, const int32_t* n, const int64_t* seen,
                            const int32_t* ended, const int32_t* parity, int32_t n_streams, int32_t cap, int32_t max_frames,
                            int32_t hop, float sample_rate, void* stream_) {
    if (!audio_ring || !lft_ring || !peak || !scratch || !stream || !first_frame || !n || !seen || !ended || !parity)
        return invalid("fastsvc_stream_loudness: null pointer");
    if (S < 1 || n_streams < 1 || cap < 4 || (cap & 3) || hop < 1 || (int64_t)cap * hop > INT32_MAX || max_frames < 1 ||
            max_frames > SL_MAX_FRAMES || max_frames > cap || !(sample_rate > 0.f) ||
            (int64_t)n_streams * cap * hop > ((int64_t)1 << 40))
        return invalid("fastsvc_stream_loudness: size out of range (S %ld, cap %ld: a multiple of 4, hop %ld, max_frames %ld: at most cap)",
                       S, cap, hop, max_frames);
    if ((reinterpret_cast<uintptr_t>(audio_ring) & 3) || (reinterpret_cast<uintptr_t>(lft_ring) & 3) ||
            (reinterpret_cast<uintptr_t>(peak) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 3))
        return invalid("fastsvc_stream_loudness: misaligned pointer");
    const int64_t ring_len = (int64_t)cap * hop;
    int64_t most = 0;
    for (int i = 0; i < S; ++i) {
        const int64_t s = stream[i], k = n[i], f = first_frame[i], p = seen[i];
        if (s < 0 || s >= n_streams) return invalid("fastsvc_stream_loudness: entry %ld: stream %ld outside [0, %ld)", i, s, n_streams);
        for (int j = 0; j < i; ++j)
            if (stream[j] == s) return invalid("fastsvc_stream_loudness: stream %ld is listed twice in one call", s);
        if (k < 0 || k > max_frames)
            return invalid("fastsvc_stream_loudness: stream %ld: %ld frames, outside [0, max_frames %ld]", s, k, max_frames);
        if (f < 0 || p < 0 || p > ((int64_t)1 << 40) || f + k > p)
            return invalid("fastsvc_stream_loudness: stream %ld: frames [%ld, +%ld) of %ld seen", s, f, k, p);
        if ((ended[i] & ~1) || (parity[i] & ~1)) return invalid("fastsvc_stream_loudness: stream %ld: ended and parity are 0 or 1", s);
        if (k == 0) continue;
        // every frame is final: it reads up to (f + k - 1) hop + 1023, or the stream has ended and these are its last frames
        if (ended[i] ? f + k != p : (f + k - 1) * hop + LD_NFFT / 2 > p * hop)
            return invalid("fastsvc_stream_loudness: stream %ld: frames [%ld, +%ld) are not final with %ld frames seen", s, f, k, p);
        // ... and the ring still holds what the first of them reads: from sample max(0, f hop - 1024) on
        const int64_t lowest = f * hop > LD_NFFT / 2 ? f * hop - LD_NFFT / 2 : 0;
        if (lowest < p * hop - ring_len)
            return invalid("fastsvc_stream_loudness: stream %ld: frame %ld reads samples the ring of %ld no longer holds (%ld frames seen)",
                           s, f, ring_len, p);
        most = k > most ? k : most;
    }
    if (most == 0) return FASTSVC_OK;               // (nothing became final: no launch)
    LoudDims d;
    d.hop = hop; d.cap = cap; d.max_frames = max_frames; d.sr = sample_rate;
    float* power = static_cast<float*>(scratch);
    float* fmax = power + (size_t)n_streams * max_frames * LD_NBINS;
    hipStream_t hs = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < S; b0 += SL_MAX) {
        const int nb = S - b0 < SL_MAX ? S - b0 : SL_MAX;
        LoudArgs a;
        int grid = 0;
        for (int i = 0; i < SL_MAX; ++i) {
            const bool on = i < nb;
            a.n[i] = on ? n[b0 + i] : 0;
            a.slot[i] = on ? stream[b0 + i] : 0;
            a.first[i] = on ? (long)first_frame[b0 + i] : 0;
            a.samples[i] = on ? (long)seen[b0 + i] * hop : 0;
            a.flags[i] = on ? ((first_frame[b0 + i] == 0 ? 1 : 0) | (parity[b0 + i] << 1) | (ended[b0 + i] << 2)) : 0;
            grid = a.n[i] > grid ? a.n[i] : grid;
        }
        if (grid == 0) continue;
        hipLaunchKernelGGL(stream_loudness_power_kernel, dim3((unsigned)grid, (unsigned)nb), dim3(256), 0, hs, a, d, audio_ring, power, fmax);
        hipLaunchKernelGGL(stream_loudness_reduce_kernel, dim3((unsigned)grid, (unsigned)nb), dim3(256), 0, hs, a, d, power, fmax, peak,
                           lft_ring);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK
                                           : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_stream_loudness: launch failed");
}

}  // extern "C"
