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
// f0_frame_dn fills d'; f0_frame_pick is the decision above; f0_frame_candidates and the f0_track_* functions at the end of
// the file are the tracker's (decode.F0Track): the local minima of d' and the Viterbi recurrence over them.

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

// d' of the frame, at dn[1 .. tau_max], for every lane to read.  x: LD_NFFT floats of LDS holding the frame (the caller
// filled it and has NOT yet synchronised); dn: F0_MAX_LAG + 2 floats of LDS (d, then d', at index tau).
__device__ __forceinline__ void f0_frame_dn(const float* x, float* dn, const F0Params& p, int tid) {
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
}

// The per-frame pick from d' (f0_frame_dn has run), to every lane.  wmin: 4 ints, res: one float.
__device__ __forceinline__ float f0_frame_pick(const float* dn, float* res, int* wmin, const F0Params& p, int tid) {
    #pragma clang fp contract(off)
    const int tau_max = p.tau_max;
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

// The frame's F0 from its samples, to every lane: d', then the pick.
__device__ __forceinline__ float f0_frame_value(const float* x, float* dn, float* res, int* wmin, const F0Params& p, int tid) {
    f0_frame_dn(x, dn, p, tid);
    return f0_frame_pick(dn, res, wmin, p, tid);
}

// ---- candidates for the tracker (DESIGN.md 4.10: decode.F0Track) ----
// A lag t in [max(tau_min, 2), tau_max] is a candidate when d'(t) < cand_threshold, d'(t) < d'(t - 1) and t == tau_max or
// d'(t) <= d'(t + 1): a local minimum of d' under the threshold.  The four with the smallest d' are kept (ties: the smaller
// lag), ordered by ascending lag, each refined by the pick's parabola under the pick's conditions: (tau_hat, s = d'(t)).
// Absent entries are (0, inf).  A flat frame has d' = 1 everywhere: nothing falls, no candidates.

constexpr int F0_CANDS = 4;                         // K: candidates per frame, a constant of the definition
constexpr unsigned long long F0_NO_KEY = ~0ull;

__device__ __forceinline__ unsigned long long f0_key_min_wave(unsigned long long k) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(k >> 32), o), lo = (unsigned)__shfl_xor((int)(k & 0xffffffffull), o);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        k = other < k ? other : k;
    }
    return k;
}

// f0_frame_dn has run.  out: F0_CANDS pairs (tau_hat, s), written by lane 0 (global or LDS); kmin: 4 keys of LDS.
// d' >= 0, so its float bits order as it does: the key (bits of d', lag) orders by d', then by lag.
__device__ __forceinline__ void f0_frame_candidates(const float* dn, unsigned long long* kmin, float cand_threshold,
                                                    const F0Params& p, int tid, float* out) {
    #pragma clang fp contract(off)
    const int tau_max = p.tau_max, lo = p.tau_min > 2 ? p.tau_min : 2;
    unsigned long long mine[F0_MAX_LAG / 256];      // this lane's local minima: lags lo + tid + 256 i
    #pragma unroll
    for (int i = 0; i < F0_MAX_LAG / 256; ++i) {
        const int t = lo + tid + 256 * i;
        mine[i] = F0_NO_KEY;
        if (t <= tau_max) {
            const float s = dn[t];
            if (s < cand_threshold && s < dn[t - 1] && (t == tau_max || s <= dn[t + 1]))
                mine[i] = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned)t;
        }
    }
    unsigned long long won[F0_CANDS];
    unsigned long long last = 0ull;                  // (no key is 0: a lag is >= 2)
    for (int r = 0; r < F0_CANDS; ++r) {            // four rounds of a block-wide minimum over the keys above the last winner
        unsigned long long k = F0_NO_KEY;
        #pragma unroll
        for (int i = 0; i < F0_MAX_LAG / 256; ++i) k = (mine[i] > last && mine[i] < k) ? mine[i] : k;
        k = f0_key_min_wave(k);
        if ((tid & 63) == 0) kmin[tid >> 6] = k;
        __syncthreads();
        const unsigned long long a = kmin[0] < kmin[1] ? kmin[0] : kmin[1], b = kmin[2] < kmin[3] ? kmin[2] : kmin[3];
        won[r] = a < b ? a : b;
        last = won[r];
        __syncthreads();                             // (the next round overwrites kmin)
    }
    if (tid == 0) {
        int lag[F0_CANDS];
        #pragma unroll
        for (int r = 0; r < F0_CANDS; ++r) lag[r] = won[r] == F0_NO_KEY ? INT32_MAX : (int)(won[r] & 0xffffffffull);
        #pragma unroll
        for (int i = 1; i < F0_CANDS; ++i) {         // ascending lag, the absent ones last
            #pragma unroll
            for (int j = F0_CANDS - 1; j >= i; --j)
                if (lag[j] < lag[j - 1]) { const int t = lag[j]; lag[j] = lag[j - 1]; lag[j - 1] = t; }
        }
        #pragma unroll
        for (int r = 0; r < F0_CANDS; ++r) {
            float tau_hat = 0.f, s = INFINITY;
            if (lag[r] != INT32_MAX) {
                const int tau = lag[r];
                s = dn[tau];
                tau_hat = (float)tau;
                if (tau - 1 >= 1 && tau + 1 <= tau_max) {
                    const float s0 = dn[tau - 1], s1 = s, s2 = dn[tau + 1];
                    const float den = (s0 - s1) + (s2 - s1);
                    if (s1 <= s0 && s1 <= s2 && den > 0.f) tau_hat = tau_hat + (0.5f * (s0 - s2)) / den;
                }
            }
            out[2 * r] = tau_hat;
            out[2 * r + 1] = s;
        }
    }
}

// ---- the tracker's recurrence: Viterbi over {4 candidates, unvoiced}, float64, every operation rounded separately ----
constexpr int F0_STATES = F0_CANDS + 1;             // state 4: unvoiced
constexpr int F0_TRACK_MAX_LAG = 64;
constexpr int F0_BP_BYTES = 8;                      // per frame: 5 backpointers, the best state, 2 unused

struct F0Track {
    double lag_bias, jump, sw, unvoiced, tau_max;
    float sr;
    int lag;
};

// The frame's candidates -> tau[k] (0: absent) and the local cost of every state.
__device__ __forceinline__ void f0_track_local(const float* cand, const F0Track& t, double* tau, double* local) {
    #pragma clang fp contract(off)
    const double tau0 = (double)cand[0];
    #pragma unroll
    for (int k = 0; k < F0_CANDS; ++k) {
        const float s = cand[2 * k + 1];
        const bool on = s < INFINITY;
        tau[k] = on ? (double)cand[2 * k] : 0.0;
        double c = INFINITY;
        if (on) {
            const double dt = tau[k] - tau0;
            const double rel = dt / t.tau_max;
            const double bias = t.lag_bias * rel;
            c = (double)s + bias;
        }
        local[k] = c;
    }
    local[F0_CANDS] = t.unvoiced;
}

// One frame of the recurrence: C (the frame before, normalised) -> C of this frame, the backpointers, and the best state.
// first: C = local.  ptau: the lags of the frame before.  Absent states cost inf and are never a transition's end.
__device__ __forceinline__ int f0_track_step(double* C, const double* ptau, const double* tau, const double* local, bool first,
                                             const F0Track& t, unsigned char* bp) {
    #pragma clang fp contract(off)
    double next[F0_STATES];
    if (first) {
        #pragma unroll
        for (int j = 0; j < F0_STATES; ++j) { next[j] = local[j]; bp[j] = 0; }
    } else {
        #pragma unroll
        for (int j = 0; j < F0_STATES; ++j) {
            double best = INFINITY;
            int from = 0;
            if (local[j] < INFINITY) {
                #pragma unroll
                for (int a = 0; a < F0_STATES; ++a) {
                    if (!(C[a] < INFINITY)) continue;
                    double tr;
                    if (a == F0_CANDS && j == F0_CANDS) tr = 0.0;
                    else if (a == F0_CANDS || j == F0_CANDS) tr = t.sw;
                    else {
                        const double ta = ptau[a], tb = tau[j];
                        const double diff = fabs(ta - tb);
                        const double rel = diff / (ta < tb ? ta : tb);
                        tr = t.jump * rel;
                    }
                    const double v = C[a] + tr;
                    if (v < best) { best = v; from = a; }
                }
            }
            next[j] = best + local[j];
            bp[j] = (unsigned char)from;
        }
        double m = next[0];
        #pragma unroll
        for (int j = 1; j < F0_STATES; ++j) m = next[j] < m ? next[j] : m;
        #pragma unroll
        for (int j = 0; j < F0_STATES; ++j) next[j] = next[j] - m;     // (inf stays inf: the unvoiced state is always finite)
    }
    int arg = 0;
    #pragma unroll
    for (int j = 0; j < F0_STATES; ++j) { C[j] = next[j]; if (next[j] < next[arg]) arg = j; }
    return arg;
}
