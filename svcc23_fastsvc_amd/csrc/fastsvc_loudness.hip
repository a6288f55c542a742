// fastsvc_loudness.hip - A-weighted log loudness feature on gfx950.
//
// Replaces `loudness_extract(audio, sampling_rate, hop_length)` of harana/bin/preprocess_fastsvc.py:60-75,
// the producer of the generator's `l` input.  The reference composes librosa 0.8.1 (setup.py:30) calls:
//   stft = librosa.stft(audio, hop_length=hop)                   n_fft 2048, periodic Hann, center=True, reflect pad
//   P    = |stft|^2
//   dB   = perceptual_weighting(P, fft_frequencies(sr))          power_to_db(P, ref 1, amin 1e-10, top_db 80: floor
//                                                                 at (max over the WHOLE spectrogram) - 80 dB) + A-weighting
//   amp  = db_to_amplitude(dB) = 10^(dB/20);   loudness[f] = log(mean_bins(amp) + 1e-5)
//   Stretch2d(hop, 1): every frame value repeated hop times      -> (1 + T // hop) * hop samples
// Here: one workgroup per frame runs a 2048-point radix-2 FFT in LDS (f32; bins below max - 80 dB are clamped
// anyway), writes the 1025-bin power spectrum and folds the utterance maximum with an atomic; a second
// kernel applies floor / A-weighting / mean / log and writes the stretched rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fastsvc_hip.h"

namespace {

#include "fastsvc_loudness.inc"    // the per-frame arithmetic, shared with fastsvc_stream_loudness.hip

constexpr int NBINS = LD_NBINS;

__global__ __launch_bounds__(256)
void loudness_power_kernel(const float* __restrict__ audio, float* __restrict__ power, unsigned* __restrict__ pmax_bits,
                           int T, int hop, int frames) {
    __shared__ float re[LD_NFFT], im[LD_NFFT];
    __shared__ float wmax[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* y = audio + (long)b * T;
    loudness_frame_fft(re, im, tid, [&](int k) { return y[reflect_index<int>(f * hop - LD_NFFT / 2 + k, T)]; });
    const float m = loudness_power_row(re, im, power + ((long)b * frames + f) * NBINS, wmax, tid);
    if (tid == 0) atomicMax(&pmax_bits[b], __float_as_uint(m));
}

__global__ __launch_bounds__(256)
void loudness_reduce_kernel(const float* __restrict__ power, const unsigned* __restrict__ pmax_bits,
                            float* __restrict__ out, int hop, int frames, float sample_rate) {
    __shared__ float part[4];
    __shared__ float result;
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float v = loudness_frame_value(power + ((long)b * frames + f) * NBINS, __uint_as_float(pmax_bits[b]), sample_rate,
                                         part, &result, tid);
    float* orow = out + ((long)b * frames + f) * hop;
    for (int j = tid; j < hop; j += 256) orow[j] = v;
}

}  // namespace

extern "C" {

int32_t fastsvc_loudness_frames(int32_t T, int32_t hop) { return (T < 1 || hop < 1) ? 0 : 1 + T / hop; }

size_t fastsvc_loudness_scratch_bytes(int32_t B, int32_t T, int32_t hop) {
    if (B < 1 || T < 1 || hop < 1) return 0;
    return (size_t)B * fastsvc_loudness_frames(T, hop) * NBINS * sizeof(float) + 256 * (size_t)((B + 63) / 64);
}

int fastsvc_loudness_extract(const float* audio, float* out, void* scratch, int32_t B, int32_t T, int32_t hop,
                             float sample_rate, void* stream_) {
    if (!audio || !out || !scratch || B < 1 || T < 2 || hop < 1) return FASTSVC_E_INVALID;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int frames = fastsvc_loudness_frames(T, hop);
    float* power = static_cast<float*>(scratch);
    unsigned* pmax = reinterpret_cast<unsigned*>(power + (size_t)B * frames * NBINS);
    if (hipMemsetAsync(pmax, 0, sizeof(unsigned) * B, stream) != hipSuccess) return FASTSVC_E_HIP;
    hipLaunchKernelGGL(loudness_power_kernel, dim3(frames, B), dim3(256), 0, stream, audio, power, pmax, T, hop, frames);
    hipLaunchKernelGGL(loudness_reduce_kernel, dim3(frames, B), dim3(256), 0, stream, power, pmax, out, hop, frames, sample_rate);
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : FASTSVC_E_HIP;
}

}  // extern "C"
