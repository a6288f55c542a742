// fastsvc_f0.inc - one frame of the YIN F0 estimator (de Cheveigne & Kawahara 2002), shared by the whole-file kernel
// (fastsvc_f0.hip) and the live-stream kernel (fastsvc_stream_f0.hip).  Included inside an anonymous namespace, after
// fastsvc_loudness.inc (the frame is the loudness frame: LD_NFFT samples centred on f hop, reflect_index padding); 256
// lanes per block.  The two callers differ only in where sample k of the frame comes from - a flat row, or a ring modulo
// its length; the arithmetic below is one text with every fused multiply-add spelled out and contraction off elsewhere,
// so that the two give the same bits wherever they are given the same samples.
//
// The function (DESIGN.md 4.10), all float32, x[k] the frame's sample k, k in [0, 2048):
//   tau_min = floor(sr / f0_ceil), tau_max = ceil(sr / f0_floor) <= 1024, W = 2048 - tau_max
//   d(tau)  = sum over 1 <= j < W of (x[j] - x[j + tau])^2,  tau = 1 .. tau_max: four partial sums, j mod 4, each in
//             ascending j, added as (p0 + p1) + (p2 + p3).  j = 0 is left out: x[0] of frame 0 is sample 1024 by reflection,
//             which a live stream whose hop divides 1024 has not received when the frame is final (the loudness weights
//             that sample by a Hann zero)
//   c(tau)  = d(1) + ... + d(tau), added in ascending tau;  d'(tau) = (d(tau) * tau) / c(tau)
//   d(1) == 0 (a zero denominator: the frame is constant) -> unvoiced
//   tau     = the smallest lag in [tau_min, tau_max] with d'(tau) < threshold, walked right while tau + 1 <= tau_max and
//             d'(tau + 1) < d'(tau);  none -> unvoiced, f0 = 0
//   parabola over s0, s1, s2 = d'(tau - 1), d'(tau), d'(tau + 1) when both neighbours lie in [1, tau_max], s1 <= s0,
//             s1 <= s2 and den = (s0 - s1) + (s2 - s1) > 0:  tau_hat = tau + 0.5 (s0 - s2) / den, else tau_hat = tau
//   f0      = sr / tau_hat

constexpr int F0_MAX_LAG = LD_NFFT / 2;             // tau_max is at most this: W >= 1024

struct F0Params {
    int tau_min, tau_max;
    float sr, threshold;
};

// d(tau) of the frame x (LDS, 16-byte aligned) for one lag.  x[j .. j + 3] is one 16-byte broadcast read; x[j + tau] is
// stride-1 across the lanes of a wave (their lags are consecutive): no bank conflicts.
__device__ __forceinline__ float f0_difference(const float* x, int tau, int W) {
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    const float* y = x + tau;
    {                                                // j = 1, 2, 3: the head of the first group of four
        const float e1 = x[1] - y[1], e2 = x[2] - y[2], e3 = x[3] - y[3];
        p1 = fmaf(e1, e1, p1); p2 = fmaf(e2, e2, p2); p3 = fmaf(e3, e3, p3);
    }
    int j = 4;
    #pragma unroll 4
    for (; j + 4 <= W; j += 4) {
        const float4 v = *reinterpret_cast<const float4*>(x + j);
        const float e0 = v.x - y[j], e1 = v.y - y[j + 1], e2 = v.z - y[j + 2], e3 = v.w - y[j + 3];
        p0 = fmaf(e0, e0, p0); p1 = fmaf(e1, e1, p1); p2 = fmaf(e2, e2, p2); p3 = fmaf(e3, e3, p3);
    }
    if (j < W) { const float e = x[j] - y[j]; p0 = fmaf(e, e, p0); ++j; }
    if (j < W) { const float e = x[j] - y[j]; p1 = fmaf(e, e, p1); ++j; }
    if (j < W) { const float e = x[j] - y[j]; p2 = fmaf(e, e, p2); }
    float d;
    {
        #pragma clang fp contract(off)
        d = (p0 + p1) + (p2 + p3);
    }
    return d;
}

// The frame's F0 from its samples, to every lane.  x: LD_NFFT floats of LDS holding the frame (the caller filled it and
// has NOT yet synchronised); dn: F0_MAX_LAG + 2 floats of LDS (d, then d', at index tau); wmin: 4 ints, res: one float.
__device__ __forceinline__ float f0_frame_value(const float* x, float* dn, float* res, int* wmin, const F0Params& p, int tid) {
    #pragma clang fp contract(off)
    const int tau_max = p.tau_max, W = LD_NFFT - tau_max;
    __syncthreads();
    for (int tau = tid + 1; tau <= tau_max; tau += 256) dn[tau] = f0_difference(x, tau, W);
    __syncthreads();
    if (tid == 0) {                                  // the cumulative mean normalisation, in ascending tau by one lane
        float c = 0.f;
        const bool flat = dn[1] == 0.f;
        for (int tau = 1; tau <= tau_max; ++tau) {
            const float d = dn[tau];
            c = c + d;
            dn[tau] = flat ? 1.f : (d * (float)tau) / c;
        }
    }
    __syncthreads();
    int mine = tau_max + 1;                          // the smallest lag of this lane under the threshold
    for (int tau = p.tau_min + tid; tau <= tau_max; tau += 256)
        if (dn[tau] < p.threshold) { mine = tau; break; }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o));
    if ((tid & 63) == 0) wmin[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        int tau = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
        float f0 = 0.f;
        if (tau <= tau_max) {
            while (tau + 1 <= tau_max && dn[tau + 1] < dn[tau]) ++tau;
            float tau_hat = (float)tau;
            if (tau - 1 >= 1 && tau + 1 <= tau_max) {
                const float s0 = dn[tau - 1], s1 = dn[tau], s2 = dn[tau + 1];
                const float den = (s0 - s1) + (s2 - s1);
                if (s1 <= s0 && s1 <= s2 && den > 0.f) tau_hat = tau_hat + (0.5f * (s0 - s2)) / den;
            }
            f0 = p.sr / tau_hat;
        }
        *res = f0;
    }
    __syncthreads();
    return *res;
}
