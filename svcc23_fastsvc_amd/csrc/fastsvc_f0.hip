// fastsvc_f0.hip - F0 of whole files by YIN on gfx950 (svcc23_fastsvc_amd/f0.py: f0_extract), the whole-file counterpart
// of the live streams' F0 (fastsvc_stream_f0.hip).  The recipe takes F0 from pyworld.harvest, a whole-file CPU algorithm
// with no frame-by-frame form; this is a DEFINITION of its own, per frame and causal up to the frame's
// look-ahead, so that a live stream can compute the same function.
//
// Frames and conventions are fastsvc_loudness_extract's: frames = 1 + T / hop, frame f is the 2048 samples centred on
// f hop with np.pad reflection at both ends (no window function).  One workgroup per (frame, utterance): the frame goes
// to LDS, fastsvc_f0.inc does the rest, lane 0 stores one float.  No scratch, no atomics, no tunables.
//
// With decode.F0Track (f0_extract(track=...)) the pick is replaced by two launches: f0_candidates_kernel, the same frame and
// d' and then the frame's four candidates (one workgroup per frame), and f0_track_kernel, fixed-lag Viterbi over them (one
// workgroup per row: one lane runs the recurrence, all lanes trace back; 8 bytes of scratch a frame).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "fastsvc_hip.h"

namespace fastsvc {
int set_last_error(int code, const char* msg);      // fastsvc_plan.cpp: the text fastsvc_last_error() returns
}

namespace {

#include "fastsvc_loudness.inc"    // LD_NFFT, reflect_index
#include "fastsvc_f0.inc"          // the per-frame arithmetic, shared with fastsvc_stream_f0.hip

__global__ __launch_bounds__(256)
void f0_extract_kernel(const float* __restrict__ audio, float* __restrict__ out, int T, int hop, int frames, F0Params p) {
    __shared__ __attribute__((aligned(16))) float x[LD_NFFT];
    __shared__ float dn[F0_MAX_LAG + 2];
    __shared__ float res;
    __shared__ int wmin[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* y = audio + (long)b * T;
    const long base = (long)f * hop - LD_NFFT / 2;
    for (int k = tid; k < LD_NFFT; k += 256) x[k] = y[reflect_index<long>(base + k, (long)T)];
    const float v = f0_frame_value(x, dn, &res, wmin, p, tid);
    if (tid == 0) out[(long)b * frames + f] = v;
}

// The candidates of every frame (fastsvc_f0.inc): one workgroup per (frame, utterance), 8 floats a frame.
__global__ __launch_bounds__(256)
void f0_candidates_kernel(const float* __restrict__ audio, float* __restrict__ out, int T, int hop, int frames, F0Params p,
                          float cand_threshold) {
    __shared__ __attribute__((aligned(16))) float x[LD_NFFT];
    __shared__ float dn[F0_MAX_LAG + 2];
    __shared__ unsigned long long kmin[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* y = audio + (long)b * T;
    const long base = (long)f * hop - LD_NFFT / 2;
    for (int k = tid; k < LD_NFFT; k += 256) x[k] = y[reflect_index<long>(base + k, (long)T)];
    f0_frame_dn(x, dn, p, tid);
    f0_frame_candidates(dn, kmin, cand_threshold, p, tid, out + ((long)b * frames + f) * 2 * F0_CANDS);
}

// The tracked F0 of every row: one workgroup per row.  One lane runs the recurrence in frame order and leaves 5 backpointers
// and the best state per frame in `scratch` (F0_BP_BYTES a frame); then every lane traces its frames back from frame
// min(f + lag, frames - 1), at most `lag` steps each.
__global__ __launch_bounds__(256)
void f0_track_kernel(const float* __restrict__ cands, float* __restrict__ out, unsigned char* __restrict__ scratch, int frames,
                     F0Track t) {
    #pragma clang fp contract(off)
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* cd = cands + (long)b * frames * 2 * F0_CANDS;
    unsigned char* bp = scratch + (long)b * frames * F0_BP_BYTES;
    if (tid == 0) {
        double C[F0_STATES], tau[F0_CANDS], ptau[F0_CANDS] = {0.0, 0.0, 0.0, 0.0}, local[F0_STATES];
        for (int f = 0; f < frames; ++f) {
            unsigned char back[F0_STATES];
            f0_track_local(cd + (long)f * 2 * F0_CANDS, t, tau, local);
            const int best = f0_track_step(C, ptau, tau, local, f == 0, t, back);
            #pragma unroll
            for (int j = 0; j < F0_STATES; ++j) bp[(long)f * F0_BP_BYTES + j] = back[j];
            bp[(long)f * F0_BP_BYTES + F0_STATES] = (unsigned char)best;
            #pragma unroll
            for (int k = 0; k < F0_CANDS; ++k) ptau[k] = tau[k];
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int f = tid; f < frames; f += 256) {
        const int e = f + t.lag < frames - 1 ? f + t.lag : frames - 1;
        int s = bp[(long)e * F0_BP_BYTES + F0_STATES];
        for (int g = e; g > f; --g) s = bp[(long)g * F0_BP_BYTES + s];
        out[(long)b * frames + f] = s < F0_CANDS ? t.sr / cd[(long)f * 2 * F0_CANDS + 2 * s] : 0.f;
    }
}

bool track_ok(int lag, double lag_bias, double jump, double sw, double unvoiced) {
    const double v[4] = {lag_bias, jump, sw, unvoiced};
    for (double c : v)
        if (!(c >= 0.0 && c < 1e300)) return false;
    return lag >= 0 && lag <= F0_TRACK_MAX_LAG;
}

}  // namespace

extern "C" {

int fastsvc_f0_lags(float sample_rate, float f0_floor, float f0_ceil, int32_t* tau_min, int32_t* tau_max) {
    if (!(sample_rate > 0.f) || !(f0_floor > 0.f) || !(f0_ceil >= f0_floor) || !(sample_rate / f0_floor < 1e6f))
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_lags: needs sample_rate > 0 and 0 < f0_floor <= f0_ceil");
    const int lo = (int)floor((double)sample_rate / (double)f0_ceil), hi = (int)ceil((double)sample_rate / (double)f0_floor);
    if (lo < 1 || hi > F0_MAX_LAG || lo > hi) {
        char buf[200];
        snprintf(buf, sizeof buf, "fastsvc_f0_lags: lags [%d, %d] outside [1, %d] (f0_ceil above the sample rate, or f0_floor too low)",
                 lo, hi, F0_MAX_LAG);
        return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
    }
    if (tau_min) *tau_min = lo;
    if (tau_max) *tau_max = hi;
    return FASTSVC_OK;
}

int fastsvc_f0_extract(const float* audio, float* out, int32_t B, int32_t T, int32_t hop, float sample_rate, float f0_floor,
                       float f0_ceil, float threshold, void* stream_) {
    if (!audio || !out || B < 1 || T < 2 || hop < 1 || B > 65535)
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_extract: null pointer or size out of range (B in [1, 65535], T >= 2, hop >= 1)");
    if ((reinterpret_cast<uintptr_t>(audio) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_extract: misaligned pointer");
    if (!(threshold > 0.f)) return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_extract: threshold must be > 0");
    F0Params p;
    if (const int rc = fastsvc_f0_lags(sample_rate, f0_floor, f0_ceil, &p.tau_min, &p.tau_max)) return rc;
    p.sr = sample_rate; p.threshold = threshold;
    const int frames = fastsvc_loudness_frames(T, hop);
    hipLaunchKernelGGL(f0_extract_kernel, dim3((unsigned)frames, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       audio, out, T, hop, frames, p);
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_f0_extract: launch failed");
}

int fastsvc_f0_candidates(const float* audio, float* out, int32_t B, int32_t T, int32_t hop, float sample_rate, float f0_floor,
                          float f0_ceil, float cand_threshold, void* stream_) {
    if (!audio || !out || B < 1 || T < 2 || hop < 1 || B > 65535)
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_candidates: null pointer or size out of range (B in [1, 65535], T >= 2, hop >= 1)");
    if ((reinterpret_cast<uintptr_t>(audio) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_candidates: misaligned pointer");
    if (!(cand_threshold > 0.f)) return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_candidates: cand_threshold must be > 0");
    F0Params p;
    if (const int rc = fastsvc_f0_lags(sample_rate, f0_floor, f0_ceil, &p.tau_min, &p.tau_max)) return rc;
    p.sr = sample_rate; p.threshold = cand_threshold;
    const int frames = fastsvc_loudness_frames(T, hop);
    hipLaunchKernelGGL(f0_candidates_kernel, dim3((unsigned)frames, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       audio, out, T, hop, frames, p, cand_threshold);
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_f0_candidates: launch failed");
}

int64_t fastsvc_f0_track_scratch_bytes(int32_t B, int32_t frames) {
    return B < 1 || frames < 1 ? 0 : (int64_t)B * frames * F0_BP_BYTES;
}

int fastsvc_f0_track(const float* cands, float* out, void* scratch, int32_t B, int32_t frames, int32_t tau_max, float sample_rate,
                     int32_t lag, double lag_bias, double jump, double switch_cost, double unvoiced, void* stream_) {
    if (!cands || !out || !scratch || B < 1 || frames < 1 || (int64_t)B * frames > ((int64_t)1 << 31) / F0_BP_BYTES)
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_track: null pointer or size out of range (B >= 1, frames >= 1)");
    if ((reinterpret_cast<uintptr_t>(cands) & 3) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_track: misaligned pointer");
    if (tau_max < 1 || tau_max > F0_MAX_LAG || !(sample_rate > 0.f) || !track_ok(lag, lag_bias, jump, switch_cost, unvoiced))
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_f0_track: needs tau_max in [1, 1024], sample_rate > 0, lag in [0, 64] "
                                                         "and finite costs >= 0");
    F0Track t;
    t.lag_bias = lag_bias; t.jump = jump; t.sw = switch_cost; t.unvoiced = unvoiced; t.tau_max = (double)tau_max;
    t.sr = sample_rate; t.lag = lag;
    hipLaunchKernelGGL(f0_track_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream_), cands, out,
                       static_cast<unsigned char*>(scratch), frames, t);
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_f0_track: launch failed");
}

}  // extern "C"
