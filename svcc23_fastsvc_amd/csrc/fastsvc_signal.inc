// fastsvc_signal.inc - the per-sample arithmetic of the sine excitation, shared by the whole-utterance synthesis
// (fastsvc_signal.hip) and the streamed one (fastsvc_stream.hip): both must give the same bits for the same frame
// prefix, so the expressions exist once.  Included inside the including file's anonymous namespace.
//
//   rad_f   = (f0_f / sample_rate) % 1                       float32, as the reference
//   C_{f+1} = frac(C_f + hop * rad_f)                        float64: the frame prefix (phase_step)
//   sample j of frame f:  sine_amp * vuv * sin(2 pi frac(C_f + (j + 1) rad_f)) + gauss * (noise_amp voiced, / 3 unvoiced)

constexpr double TWO_PI = 6.283185307179586476925286766559;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ float gauss(uint64_t seed, uint64_t idx) {
    const uint64_t h = mix64(mix64(idx ^ seed) + seed);
    const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777216.0f);   // (0, 1]
    const float u2 = (float)(uint32_t)((h >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.2831853f * u2);
}

// (f0 / sample_rate) % 1 in fp32, as the reference
__device__ __forceinline__ float frame_rad(float f0v, float sr) { return fmodf(f0v / sr, 1.0f); }

// the frame prefix one frame on: frac(run + hop * rad)
__device__ __forceinline__ double phase_step(double run, float rad, int hop) {
    run += (double)hop * (double)rad;
    run -= floor(run);
    return run;
}

// sample j of a frame whose prefix is cf; ctr is the noise counter of the sample
__device__ __forceinline__ float sine_sample(float f0v, double cf, int j, float sr, float sine_amp, float noise_amp,
                                             uint64_t seed, uint64_t ctr) {
    const float vuv = f0v > 0.f ? 1.f : 0.f;
    const float rad = frame_rad(f0v, sr);
    double ph = cf + (double)(j + 1) * (double)rad;
    ph -= floor(ph);
    float v = vuv * (float)sin(ph * TWO_PI) * sine_amp;
    if (noise_amp > 0.f) v += gauss(seed, ctr) * (vuv * noise_amp + (1.0f - vuv) * noise_amp / 3.0f);
    return v;
}
