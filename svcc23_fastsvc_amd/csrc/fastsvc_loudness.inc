// fastsvc_loudness.inc - one frame of the A-weighted log loudness, shared by the whole-file kernels (fastsvc_loudness.hip)
// and the live-stream kernels (fastsvc_stream_loudness.hip).  Included inside an anonymous namespace; 256 lanes per block.
// The two callers differ only in where sample i of the frame comes from - a flat row, or a ring modulo its length - and
// in which maximum the 80 dB floor hangs under; the arithmetic below is one text, so that the two give the same bits
// wherever they are given the same samples and the same maximum.

constexpr int LD_NFFT = 2048;
constexpr int LD_NBINS = LD_NFFT / 2 + 1;
constexpr int LD_LOGN = 11;

template <typename I>
__device__ __forceinline__ I reflect_index(I i, I T) {
    // np.pad(..., mode="reflect"): ... y[2] y[1] | y[0] y[1] ... y[T-1] | y[T-2] y[T-3] ...
    if (T == 1) return 0;
    const I period = 2 * (T - 1);
    i %= period;
    if (i < 0) i += period;
    return i < T ? i : period - i;
}

// The windowed frame into re / im (LD_NFFT floats of LDS each), then the 2048-point FFT in place.  sample(k) is element
// k of the frame, k in [0, 2048): the caller resolves padding.
template <typename Sample>
__device__ __forceinline__ void loudness_frame_fft(float* re, float* im, int tid, Sample sample) {
    // windowed frame, written in bit-reversed order (decimation in time)
    for (int k = tid; k < LD_NFFT; k += 256) {
        const float w = 0.5f - 0.5f * cospif(2.0f * (float)k / (float)LD_NFFT);     // scipy get_window("hann", fftbins=True)
        const int r = (int)(__brev((unsigned)k) >> (32 - LD_LOGN));
        re[r] = sample(k) * w;
        im[r] = 0.f;
    }
    __syncthreads();
    for (int s = 1; s <= LD_LOGN; ++s) {
        const int half = 1 << (s - 1);
        for (int i = tid; i < LD_NFFT / 2; i += 256) {
            const int j = i & (half - 1);
            const int lo = ((i >> (s - 1)) << s) + j, hi = lo + half;
            float sn, cs;
            sincospif(-(float)j / (float)half, &sn, &cs);                           // exp(-i pi j / half)
            // (which product of a sum of two is rounded before the fused multiply-add is the compiler's choice, and it
            // chooses by context: spelled out, so that every kernel that includes this text rounds alike)
            const float xr = fmaf(re[hi], cs, -(im[hi] * sn)), xi = fmaf(re[hi], sn, im[hi] * cs);
            const float ar = re[lo], ai = im[lo];
            re[lo] = ar + xr; im[lo] = ai + xi;
            re[hi] = ar - xr; im[hi] = ai - xi;
        }
        __syncthreads();
    }
}

// The 1025-bin power row of the transformed frame -> prow; returns the row's maximum (to every lane).  wmax: 4 floats of LDS.
__device__ __forceinline__ float loudness_power_row(const float* re, const float* im, float* __restrict__ prow, float* wmax, int tid) {
    float m = 0.f;
    for (int k = tid; k < LD_NBINS; k += 256) {
        float p;
        {
            #pragma clang fp contract(off)      // (both squares rounded, then their sum: in every kernel that includes this)
            p = re[k] * re[k] + im[k] * im[k];
        }
        prow[k] = p;
        m = fmaxf(m, p);
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

__device__ __forceinline__ float a_weighting_db(float freq) {
    // librosa.A_weighting (min_db = -80): IEC 61672 A curve
    const float f2 = freq * freq;
    const float c0 = 12200.f * 12200.f, c1 = 20.6f * 20.6f, c2 = 107.7f * 107.7f, c3 = 737.9f * 737.9f;
    if (f2 <= 0.f) return -80.f;
    const float w = 2.0f + 20.0f * (log10f(c0) + 2.0f * log10f(f2) - log10f(f2 + c0) - log10f(f2 + c1)
                                    - 0.5f * log10f(f2 + c2) - 0.5f * log10f(f2 + c3));
    return fmaxf(w, -80.f);
}

// The frame's value from its power row: every bin clamped 80 dB below `pmax` (top_db = 80), A-weighted, turned into an
// amplitude; log(mean over bins + 1e-5), returned to every lane.  part: 4 floats of LDS, result: 1.
__device__ __forceinline__ float loudness_frame_value(const float* __restrict__ prow, float pmax, float sample_rate, float* part,
                                                      float* result, int tid) {
    const float floor_db = 10.f * log10f(fmaxf(1e-10f, pmax)) - 80.f;
    float sum = 0.f;
    for (int k = tid; k < LD_NBINS; k += 256) {
        float db = fmaxf(10.f * log10f(fmaxf(1e-10f, prow[k])), floor_db);
        db += a_weighting_db((float)k * sample_rate / (float)LD_NFFT);
        sum += exp10f(db * 0.05f);
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) *result = logf(((part[0] + part[1]) + (part[2] + part[3])) / (float)LD_NBINS + 1e-5f);
    __syncthreads();
    return *result;
}
