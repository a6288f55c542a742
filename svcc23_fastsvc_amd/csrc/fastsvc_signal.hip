// fastsvc_signal.hip - sine-excitation synthesis on gfx950.
//
// Replaces harana/utils/features.py:111-213 `SignalGenerator.__call__` (the step right before the
// generator forward inside `FastSVCGenerator.inference`, fastsvc.py:381):
//   sinusoid(f0):  vuv = (f0 > 0) nearest-upsampled x hop;  rad = (f0_up / sr) % 1;
//                  sine = sine_amp * vuv * sin(2 pi cumsum(rad)) + randn * (noise_amp voiced, noise_amp/3 unvoiced)
//   random_noise:  randn;    vuv_binary:  vuv
// rad is constant inside a frame, so cumsum[f*hop + j] = C_f + (j+1) * rad_f with the frame prefix
// C_f = hop * sum_{g<f} rad_g: a scan over F frames (f64, reduced mod 1 so the sin argument stays
// small - the reference's fp32 cumsum reaches ~2e3 cycles at 10 s) and a closed form per sample.
// Noise: counter-based hash + Box-Muller (the reference's torch.randn stream is not reproducible
// anyway); deterministic for a given seed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fastsvc_hip.h"

namespace {

#include "fastsvc_signal.inc"      // mix64, gauss, frame_rad, phase_step, sine_sample: shared with fastsvc_stream.hip

// one workgroup per utterance: exclusive scan of hop * rad_f over the frames, kept mod 1 in f64
__global__ __launch_bounds__(256)
void frame_phase_kernel(const float* __restrict__ f0, double* __restrict__ cf, int F, int hop, float sr) {
    __shared__ double part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* f = f0 + (long)b * F;
    double* c = cf + (long)b * F;
    const int per = (F + 255) / 256;
    const int lo = tid * per, hi = min(F, lo + per);
    double s = 0.0;
    for (int i = lo; i < hi; ++i) {
        s += (double)hop * (double)frame_rad(f[i], sr);
    }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {                                            // 256 partials: serial scan is fine
        double run = 0.0;
        for (int i = 0; i < 256; ++i) { const double v = part[i]; part[i] = run; run += v; run -= floor(run); }
    }
    __syncthreads();
    double run = part[tid];
    for (int i = lo; i < hi; ++i) {
        c[i] = run;
        run = phase_step(run, frame_rad(f[i], sr), hop);
    }
}

struct SigArgs {
    int types[4];      // 0 noise, 1 sine, 2 uv  (channel order of the output)
    int ntypes;
};

__global__ __launch_bounds__(256)
void synth_kernel(const float* __restrict__ f0, const double* __restrict__ cf, float* __restrict__ out,
                  int F, int hop, float sr, float sine_amp, float noise_amp, SigArgs a, uint64_t seed) {
    const int b = blockIdx.y;
    const long T = (long)F * hop;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int fr = (int)(t / hop);
    const int j = (int)(t - (long)fr * hop);
    const float f0v = f0[(long)b * F + fr];
    const float vuv = f0v > 0.f ? 1.f : 0.f;
    for (int k = 0; k < a.ntypes; ++k) {
        float v;
        const uint64_t ctr = ((uint64_t)(b * 4 + k) << 40) + (uint64_t)t;
        if (a.types[k] == 1) {
            v = sine_sample(f0v, cf[(long)b * F + fr], j, sr, sine_amp, noise_amp, seed, ctr);
        } else if (a.types[k] == 0) {
            v = gauss(seed ^ 0x5851F42D4C957F2Dull, ctr);
        } else {
            v = vuv;
        }
        out[((long)b * a.ntypes + k) * T + t] = v;
    }
}

thread_local char g_sig_err[160];

}  // namespace

extern "C" {

size_t fastsvc_signal_scratch_bytes(int32_t B, int32_t F) { return (size_t)B * F * sizeof(double); }

int fastsvc_signal_generate(const float* f0, float* out, void* scratch, int32_t B, int32_t F, int32_t hop,
                            float sample_rate, float sine_amp, float noise_amp,
                            const int32_t* types, int32_t ntypes, uint64_t seed, void* stream_) {
    if (!f0 || !out || !scratch || !types || B < 1 || F < 1 || hop < 1 || ntypes < 1 || ntypes > 4 || sample_rate <= 0.f)
        return FASTSVC_E_INVALID;
    SigArgs a;
    a.ntypes = ntypes;
    for (int i = 0; i < 4; ++i) a.types[i] = i < ntypes ? types[i] : 0;
    for (int i = 0; i < ntypes; ++i)
        if (types[i] < 0 || types[i] > 2) return FASTSVC_E_INVALID;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    double* cf = static_cast<double*>(scratch);
    hipLaunchKernelGGL(frame_phase_kernel, dim3(B), dim3(256), 0, stream, f0, cf, F, hop, sample_rate);
    const long T = (long)F * hop;
    hipLaunchKernelGGL(synth_kernel, dim3((unsigned)((T + 255) / 256), B), dim3(256), 0, stream,
                       f0, cf, out, F, hop, sample_rate, sine_amp, noise_amp, a, seed);
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : FASTSVC_E_HIP;
}

}  // extern "C"
