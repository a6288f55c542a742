// fastsvc_f0.hip - F0 of whole files by YIN on gfx950 (svcc23_fastsvc_amd/f0.py: f0_extract), the whole-file counterpart
// of the live streams' F0 (fastsvc_stream_f0.hip).  The recipe takes F0 from pyworld.harvest, a whole-file CPU algorithm
// with no frame-by-frame form; this is a DEFINITION of its own, per frame and causal up to the frame's
// look-ahead, so that a live stream can compute the same function.
//
// Frames and conventions are fastsvc_loudness_extract's: frames = 1 + T / hop, frame f is the 2048 samples centred on
// f hop with np.pad reflection at both ends (no window function).  One workgroup per (frame, utterance): the frame goes
// to LDS, fastsvc_f0.inc does the rest, lane 0 stores one float.  No scratch, no atomics, no tunables.
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

}  // extern "C"
