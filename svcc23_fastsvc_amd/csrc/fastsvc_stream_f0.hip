// fastsvc_stream_f0.hip - the F0 and the excitation of live streams from their raw audio, on gfx950
// (decode.StreamSession(f0="audio")): the frames of a stream that have become FINAL - the frames fastsvc_stream_loudness
// finalises in the same push - get their F0 by YIN from the stream's audio ring, the Gaussian log-F0 shift, and their
// excitation, straight into the stream's excitation ring.
//
// The function is fastsvc_f0_extract's, frame by frame: fastsvc_f0.inc is one text for both, and the value
// is a function of the frame's 2048 samples alone, so a streamed frame has the whole-file bits for every push schedule,
// slot and ring position.  There is no running state in the estimator.
//
//   stream_f0_frames    one block per (stream, newly final frame): reads the AUDIO ring (sample p at p % (cap hop)),
//                       writes the raw F0 to f0_ring[slot][f % cap], then the shifted F0 - F0Statistics.convert in float64
//                       for voiced frames of a stream that has statistics, else the raw value - to f0s_ring
//   stream_f0_excite    blocks per stream: one lane runs the phase recurrence C_{f+1} = frac(C_f + hop rad_f) over the
//                       call's frames from phase[slot][parity] into LDS (fastsvc_stream.hip's rule: reads entry `parity`,
//                       block 0 writes entry `parity ^ 1`; first_frame == 0 starts at 0 and reads nothing), then all lanes
//                       write the samples with fastsvc_signal.inc's closed form into exc_ring, the noise keyed by the seed
//                       and the ABSOLUTE sample index - stream_push_kernel's excitation part, from the shifted F0 ring
//
//   stream_f0_running   (fastsvc_stream_f0_running alone, between the two) one block per stream that runs SOURCE STATISTICS
//                       (decode.RunningF0Stats) and has frames in the call: all lanes read the call's raw F0 from f0_ring
//                       and take d = log f0 - m_p in float64, one lane runs the recurrence of the three sums (w, S1, S2) in
//                       frame order from rec[slot][parity] into LDS, all lanes shift their frame by the statistics up to
//                       and including it and overwrite f0s_ring; 256 frames a tile, the state carried from tile to tile,
//                       the block writes rec[slot][parity ^ 1] (first_frame == 0 starts from zeros and reads nothing)
//
//   With TRACKING (fastsvc_stream_f0_tracked alone; decode.F0Track) the frames launch runs in candidate mode
//   and a tracker launch follows it:
//   stream_f0_cands     one block per (stream, newly final frame): the frame and d' as above, then the frame's four
//                       candidates (fastsvc_f0.inc) into cand_ring[slot][f % cap] in place of the pick
//   stream_f0_track     one block per stream with new frames or frames to emit: one lane advances the Viterbi recurrence over
//                       the new frames from track_rec[slot][parity] (first_frame == 0 starts fresh and reads nothing) and
//                       leaves backpointers and best states in bp_ring, then all lanes trace the frames to emit - `lag`
//                       behind the final ones, all of them at the end - back at most `lag` steps and write the tracked raw F0
//                       to f0_ring and its static shift to f0s_ring.  stream_f0_running and stream_f0_excite then run over the
//                       EMITTED frames.
//
// Every launch reads what the one before wrote: two launches (three with running statistics, one more with tracking), ordered
// by the stream.
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

#include "fastsvc_loudness.inc"    // LD_NFFT, reflect_index
#include "fastsvc_f0.inc"          // the per-frame estimator, shared with fastsvc_f0.hip
#include "fastsvc_signal.inc"      // frame_rad, phase_step, sine_sample: shared with fastsvc_signal.hip and fastsvc_stream.hip

constexpr int SF_MAX = 64;                          // streams per launch (the arguments hold their descriptors)
constexpr int SF_MAX_FRAMES = 2048;                 // frames of one stream a call finalises (their prefixes: 16 KiB of LDS)
constexpr int SF_MAX_BLOCKS = 64;                   // blocks per stream of the excitation launch (grid-stride beyond)

struct F0Args {
    long first[SF_MAX];                             // the stream's first frame of this call
    long samples[SF_MAX];                           // samples the stream's audio ring has received
    int n[SF_MAX];                                  // frames of this call
    int slot[SF_MAX];
    int flags[SF_MAX];                              // bit 0: the stream's first frame is among them (the phase starts at 0);
};                                                  // bit 1: the phase entry to read; bit 2: ended; bit 3: has statistics

struct F0Seeds {                                    // (the excitation launch alone takes them: the arguments stay under 4 KiB)
    unsigned long long seed[SF_MAX];
};

struct F0Shift {                                    // F0Statistics.convert's constants: source mean, std ratio, target mean
    double m0[SF_MAX], ratio[SF_MAX], m1[SF_MAX];
};

struct F0Dims {
    int hop, cap;
    float sine_amp, noise_amp;
};

// F0Statistics.convert for one frame (fastsvc_fanout.hip's ShiftF0): every operation a separately rounded double operation
__device__ __forceinline__ float shift_f0(float f, double m0, double ratio, double m1) {
    #pragma clang fp contract(off)
    if (!(f > 0.f)) return 0.f;
    const double l = log((double)f);
    const double d = l - m0;
    const double q = ratio * d;
    const double s = q + m1;
    return (float)exp(s);
}

constexpr int SF_TILE = 256;                        // frames of one stream the running shift holds in LDS at a time

struct RunArgs {                                    // per BLOCK of the running shift: a stream that runs statistics and has frames
    double mp[SF_MAX], n0[SF_MAX], prior[SF_MAX];   // prior mean, prior weight in frames, n0 s_p s_p
    double g[SF_MAX], mt[SF_MAX], st[SF_MAX];       // decay per voiced frame, target mean and std
    int pos[SF_MAX];                                // the first frame's place in the rings: first % cap
    int slot[SF_MAX];
    int nf[SF_MAX];                                 // frames << 2 | bit 1: the record entry to read | bit 0: start from zeros
};
static_assert(sizeof(RunArgs) + 64 <= 4096, "a kernel takes at most 4 KiB of arguments");

// The running source statistics: a final voiced frame with d = log f0 - m_p updates w = w g + 1, S1 = S1 g + d,
// S2 = S2 g + d d and is shifted by mu = S1 / (n0 + w), var = (n0 s_p^2 + S2) / (n0 + w) - mu^2 - itself included; an unvoiced
// frame is 0 and leaves the state alone.  Every operation a separately rounded double operation, as in shift_f0.
__global__ __launch_bounds__(SF_TILE)
void stream_f0_running_kernel(RunArgs r, int cap, const float* __restrict__ f0_ring, float* __restrict__ f0s_ring,
                              double* __restrict__ rec) {
    #pragma clang fp contract(off)
    __shared__ double sd[SF_TILE], sw[SF_TILE], s1[SF_TILE], s2[SF_TILE];
    __shared__ unsigned char voiced[SF_TILE];
    __shared__ double state[4];                     // w, S1, S2, voiced frames: carried from tile to tile
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = r.nf[b] >> 2, flags = r.nf[b] & 3, slot = r.slot[b], pos = r.pos[b];
    const double mp = r.mp[b], n0 = r.n0[b], prior = r.prior[b], g = r.g[b], mt = r.mt[b], st = r.st[b];
    const float* raw = f0_ring + (long)slot * cap;
    float* out = f0s_ring + (long)slot * cap;
    double* mine = rec + (long)slot * 8;
    if (tid < 4) state[tid] = (flags & 1) ? 0.0 : mine[4 * (flags >> 1) + tid];
    for (int t0 = 0; t0 < n; t0 += SF_TILE) {       // (n is uniform per block)
        const int f = t0 + tid;
        const int at = (pos + f) % cap;
        const float v = f < n ? raw[at] : 0.f;
        const bool on = v > 0.f;
        const double d = on ? log((double)v) - mp : 0.0;
        sd[tid] = d;
        voiced[tid] = on ? 1 : 0;
        __syncthreads();
        if (tid == 0) {
            double w = state[0], a1 = state[1], a2 = state[2], count = state[3];
            const int m = n - t0 < SF_TILE ? n - t0 : SF_TILE;
            for (int j = 0; j < m; ++j) {
                if (voiced[j]) {
                    const double dj = sd[j];
                    const double wg = w * g, a1g = a1 * g, a2g = a2 * g, dd = dj * dj;
                    w = wg + 1.0;
                    a1 = a1g + dj;
                    a2 = a2g + dd;
                    count = count + 1.0;
                }
                sw[j] = w; s1[j] = a1; s2[j] = a2;
            }
            state[0] = w; state[1] = a1; state[2] = a2; state[3] = count;
        }
        __syncthreads();
        if (f < n) {
            float res = 0.f;
            if (on) {
                const double N = n0 + sw[tid];
                const double mu = s1[tid] / N;
                const double e2 = prior + s2[tid];
                const double m2 = e2 / N;
                const double mumu = mu * mu;
                const double var = m2 - mumu;       // >= n0 s_p^2 / N > 0 by Cauchy-Schwarz
                const double ratio = st / sqrt(var);
                const double c = d - mu;
                const double q = ratio * c;
                const double s = q + mt;
                res = (float)exp(s);
            }
            out[at] = res;
        }
        __syncthreads();                            // (the next tile overwrites the sums)
    }
    if (tid < 4) mine[4 * ((flags >> 1) ^ 1) + tid] = state[tid];
}

// Frame f of entry b's stream from its audio ring into x (LDS); the caller's estimator synchronises.
__device__ __forceinline__ void stream_frame_load(float* x, const float* __restrict__ audio_ring, const F0Args& a, const F0Dims& d,
                                                  int b, long f, int tid) {
    const long ring_len = (long)d.cap * d.hop, T = a.samples[b];
    const bool ended = (a.flags[b] & 4) != 0;
    const float* ring = audio_ring + a.slot[b] * ring_len;
    const long base = f * d.hop - LD_NFFT / 2;
    for (int k = tid; k < LD_NFFT; k += 256) {
        long i = base + k;
        if (ended) i = reflect_index<long>(i, T);
        else if (i < 0) i = -i;
        // (a frame that is final before the end reads [f hop - 1024, f hop + 1024) < T; only frame 0's element 0 mirrors
        // to sample 1024, which may not have arrived when hop divides 1024 - the estimator never reads x[0])
        x[k] = i < T ? ring[i % ring_len] : 0.f;
    }
}

// The frames kernel in CANDIDATE mode (a session with decode.F0Track): the same frame, the same d', and the frame's four
// candidates into the stream's candidate ring (frame f at f % cap, 8 floats) in place of the pick.
__global__ __launch_bounds__(256)
void stream_f0_cands_kernel(F0Args a, F0Dims d, F0Params p, float cand_threshold, const float* __restrict__ audio_ring,
                            float* __restrict__ cand_ring) {
    __shared__ __attribute__((aligned(16))) float x[LD_NFFT];
    __shared__ float dn[F0_MAX_LAG + 2];
    __shared__ unsigned long long kmin[4];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (j >= a.n[b]) return;                        // (uniform per block)
    const long f = a.first[b] + j;
    stream_frame_load(x, audio_ring, a, d, b, f, tid);
    f0_frame_dn(x, dn, p, tid);
    f0_frame_candidates(dn, kmin, cand_threshold, p, tid, cand_ring + ((long)a.slot[b] * d.cap + f % d.cap) * 2 * F0_CANDS);
}

struct TrackArgs {                                  // per entry of a tracked call
    long first[SF_MAX];                             // the first newly final frame: the recurrence advances over [first, first + n)
    long efirst[SF_MAX];                            // the first frame to emit: [efirst, efirst + en) get their tracked F0
    int n[SF_MAX], en[SF_MAX];
    int slot[SF_MAX];
    int flags[SF_MAX];                              // bit 0: the tracker record's entry to read; bit 3: has statistics
};
static_assert(sizeof(TrackArgs) + sizeof(F0Shift) + sizeof(F0Track) + 96 <= 4096, "a kernel takes at most 4 KiB of arguments");

// The tracker of live streams: one block per entry with new frames or frames to emit.  One lane advances the
// recurrence over the new frames from rec[slot][parity] (5 doubles: C of the last frame, normalised; first == 0 starts fresh
// and reads nothing) with the lags of frame first - 1 from the candidate ring, leaves backpointers and best state in
// bp_ring (frame f at f % cap, F0_BP_BYTES bytes) and C in rec[slot][parity ^ 1]; then every lane traces its frames to emit
// back from frame min(f + lag, first + n - 1) and writes the tracked raw F0 and its static shift.
__global__ __launch_bounds__(256)
void stream_f0_track_kernel(TrackArgs a, F0Shift sh, F0Track t, int cap, const float* __restrict__ cand_ring,
                            unsigned char* __restrict__ bp_ring, double* __restrict__ rec, float* __restrict__ f0_ring,
                            float* __restrict__ f0s_ring) {
    #pragma clang fp contract(off)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = a.n[b], en = a.en[b];
    if (n == 0 && en == 0) return;                  // (uniform per block)
    const int slot = a.slot[b], flags = a.flags[b];
    const long first = a.first[b], efirst = a.efirst[b];
    const float* cd = cand_ring + (long)slot * cap * 2 * F0_CANDS;
    unsigned char* bp = bp_ring + (long)slot * cap * F0_BP_BYTES;
    if (tid == 0 && n > 0) {
        double C[F0_STATES], tau[F0_CANDS], ptau[F0_CANDS] = {0.0, 0.0, 0.0, 0.0}, local[F0_STATES];
        double* mine = rec + (long)slot * 2 * 8;
        if (first > 0) {
            const double* from = mine + 8 * (flags & 1);
            #pragma unroll
            for (int j = 0; j < F0_STATES; ++j) C[j] = from[j];
            f0_track_local(cd + ((first - 1) % cap) * 2 * F0_CANDS, t, ptau, local);
        }
        for (int i = 0; i < n; ++i) {
            const long f = first + i, at = f % cap;
            unsigned char back[F0_STATES];
            f0_track_local(cd + at * 2 * F0_CANDS, t, tau, local);
            const int best = f0_track_step(C, ptau, tau, local, f == 0, t, back);
            #pragma unroll
            for (int j = 0; j < F0_STATES; ++j) bp[at * F0_BP_BYTES + j] = back[j];
            bp[at * F0_BP_BYTES + F0_STATES] = (unsigned char)best;
            #pragma unroll
            for (int k = 0; k < F0_CANDS; ++k) ptau[k] = tau[k];
        }
        double* to = mine + 8 * ((flags & 1) ^ 1);
        #pragma unroll
        for (int j = 0; j < F0_STATES; ++j) to[j] = C[j];
    }
    __threadfence_block();
    __syncthreads();
    const long last = first + n - 1;                // the newest final frame
    for (int i = tid; i < en; i += 256) {
        const long f = efirst + i;
        const long e = f + t.lag < last ? f + t.lag : last;
        int s = bp[(e % cap) * F0_BP_BYTES + F0_STATES] & 7;      // (& 7: a byte of the ring never indexes outside its frame)
        for (long g = e; g > f; --g) s = bp[(g % cap) * F0_BP_BYTES + s] & 7;
        const float v = s < F0_CANDS ? t.sr / cd[(f % cap) * 2 * F0_CANDS + 2 * s] : 0.f;
        const long at = (long)slot * cap + f % cap;
        f0_ring[at] = v;
        f0s_ring[at] = (flags & 8) ? shift_f0(v, sh.m0[b], sh.ratio[b], sh.m1[b]) : v;
    }
}

__global__ __launch_bounds__(256)
void stream_f0_frames_kernel(F0Args a, F0Shift sh, F0Dims d, F0Params p, const float* __restrict__ audio_ring,
                             float* __restrict__ f0_ring, float* __restrict__ f0s_ring) {
    __shared__ __attribute__((aligned(16))) float x[LD_NFFT];
    __shared__ float dn[F0_MAX_LAG + 2];
    __shared__ float res;
    __shared__ int wmin[4];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (j >= a.n[b]) return;                        // (uniform per block)
    const int slot = a.slot[b], flags = a.flags[b];
    const long f = a.first[b] + j;
    stream_frame_load(x, audio_ring, a, d, b, f, tid);
    const float v = f0_frame_value(x, dn, &res, wmin, p, tid);
    if (tid == 0) {
        const long at = (long)slot * d.cap + f % d.cap;
        f0_ring[at] = v;
        f0s_ring[at] = (flags & 8) ? shift_f0(v, sh.m0[b], sh.ratio[b], sh.m1[b]) : v;
    }
}

__global__ __launch_bounds__(256)
void stream_f0_excite_kernel(F0Args a, F0Seeds sd, F0Dims d, float sr, const float* __restrict__ f0s_ring, float* __restrict__ exc_ring,
                             double* __restrict__ phase) {
    __shared__ double pre[SF_MAX_FRAMES];
    __shared__ float f0v[SF_MAX_FRAMES];
    const int b = blockIdx.y;
    const int n = a.n[b];
    if (n == 0) return;                             // (uniform per block)
    const int slot = a.slot[b], flags = a.flags[b];
    const int hop = d.hop, cap = d.cap;
    const long first = a.first[b];
    const float* fr = f0s_ring + (long)slot * cap;
    for (int f = threadIdx.x; f < n; f += 256) f0v[f] = fr[(first + f) % cap];
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = (flags & 1) ? 0.0 : phase[2 * slot + ((flags >> 1) & 1)];
        for (int f = 0; f < n; ++f) {
            pre[f] = c;
            c = phase_step(c, frame_rad(f0v[f], sr), hop);
        }
        if (blockIdx.x == 0) phase[2 * slot + (((flags >> 1) & 1) ^ 1)] = c;
    }
    __syncthreads();
    const long ring_s = (long)cap * hop, ns = (long)n * hop;
    float* re = exc_ring + slot * ring_s;
    const long p0 = first % cap;
    const uint64_t t0 = (uint64_t)first * (uint64_t)hop;            // the call's first sample in the stream
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < (ns + 3) / 4; g += (long)gridDim.x * 256) {
        const long k0 = 4 * g;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long k = k0 + e;
            if (k >= ns) break;
            const int q = (int)(k / hop);
            const int i = (int)(k - (long)q * hop);
            v[e] = sine_sample(f0v[q], pre[q], i, sr, d.sine_amp, d.noise_amp, sd.seed[b], t0 + (uint64_t)k);
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

int invalid(const char* who, const char* fmt, long a = 0, long b = 0, long c = 0, long e = 0) {
    char buf[280];
    const int at = snprintf(buf, sizeof buf, "%s: ", who);
    snprintf(buf + at, sizeof buf - at, fmt, a, b, c, e);
    return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
}

bool is_finite(double v) { return v == v && v > -1e300 && v < 1e300; }

// What fastsvc_stream_f0_tracked adds to the other two entry points: the tracker's rings and record, per entry the record's
// parity and the frames to emit, and the tracker's constants.
struct TrackCall {
    float* cand_ring;
    unsigned char* bp_ring;
    double* rec;
    const int32_t* parity;
    const int64_t* emit_first;
    const int32_t* emit_n;
    float cand_threshold;
    F0Track t;
};

// All entry points: `who` names the one that was called.  fastsvc_stream_f0 passes no record, no running constants and no
// tracker, and then this validates, fills and launches exactly what it always did.
int stream_f0_run(const char* who, const TrackCall* tk, const float* audio_ring, float* f0_ring, float* f0s_ring, float* exc_ring, double* phase,
                  double* rec, int32_t S, const int32_t* stream, const int64_t* first_frame, const int32_t* n, const int64_t* seen,
                  const int32_t* ended, const int32_t* parity, const uint64_t* seed, const double* stats, const double* running,
                  int32_t n_streams, int32_t cap, int32_t max_frames, int32_t hop, float sample_rate, float f0_floor,
                  float f0_ceil, float threshold, float sine_amp, float noise_amp, void* stream_) {
    if (!audio_ring || !f0_ring || !f0s_ring || !exc_ring || !phase || !stream || !first_frame || !n || !seen || !ended ||
            !parity || !seed || !stats)
        return invalid(who, "null pointer");
    if (S < 1 || n_streams < 1 || cap < 4 || (cap & 3) || hop < 1 || (int64_t)cap * hop > INT32_MAX || max_frames < 1 ||
            max_frames > SF_MAX_FRAMES || max_frames > cap || !(sample_rate > 0.f) ||
            (int64_t)n_streams * cap * hop > ((int64_t)1 << 40))
        return invalid(who, "size out of range (S %ld, cap %ld: a multiple of 4, hop %ld, max_frames %ld: at most cap)",
                       S, cap, hop, max_frames);
    if ((reinterpret_cast<uintptr_t>(audio_ring) & 3) || (reinterpret_cast<uintptr_t>(f0_ring) & 3) ||
            (reinterpret_cast<uintptr_t>(f0s_ring) & 3) || (reinterpret_cast<uintptr_t>(exc_ring) & 15) ||
            (reinterpret_cast<uintptr_t>(phase) & 7))
        return invalid(who, "misaligned pointer (the excitation ring: 16 bytes, the phase: 8)");
    if (reinterpret_cast<uintptr_t>(rec) & 7) return invalid(who, "misaligned pointer (the statistics record: 8 bytes)");
    if (!(threshold > 0.f)) return invalid(who, "threshold must be > 0");
    F0Params p;
    if (const int rc = fastsvc_f0_lags(sample_rate, f0_floor, f0_ceil, &p.tau_min, &p.tau_max)) return rc;
    p.sr = sample_rate; p.threshold = threshold;
    const int64_t ring_len = (int64_t)cap * hop;
    int64_t most = 0;
    for (int i = 0; i < S; ++i) {
        const int64_t s = stream[i], k = n[i], f = first_frame[i], q = seen[i];
        if (s < 0 || s >= n_streams) return invalid(who, "entry %ld: stream %ld outside [0, %ld)", i, s, n_streams);
        for (int j = 0; j < i; ++j)
            if (stream[j] == s) return invalid(who, "stream %ld is listed twice in one call", s);
        if (k < 0 || k > max_frames)
            return invalid(who, "stream %ld: %ld frames, outside [0, max_frames %ld]", s, k, max_frames);
        if (f < 0 || q < 0 || q > ((int64_t)1 << 40) || f + k > q)
            return invalid(who, "stream %ld: frames [%ld, +%ld) of %ld seen", s, f, k, q);
        if ((ended[i] & ~1) || (parity[i] & ~1)) return invalid(who, "stream %ld: ended and parity are 0 or 1", s);
        const double* st = stats + 4 * i;               // (source mean, source std, target mean, target std), or four NaN: no shift
        const bool none = st[0] != st[0] && st[1] != st[1] && st[2] != st[2] && st[3] != st[3];
        if (!none && !(is_finite(st[0]) && is_finite(st[1]) && is_finite(st[2]) && is_finite(st[3]) && st[1] > 0.0))
            return invalid(who, "stream %ld: statistics are four finite values with a source std > 0, or four NaN for none", s);
        if (running) {                                  // (m_p, s_p, n0, g, m_t, s_t), or six NaN: the stream runs no statistics
            const double* ru = running + 6 * i;
            bool off = true, fin = true;
            for (int e = 0; e < 6; ++e) { off = off && ru[e] != ru[e]; fin = fin && is_finite(ru[e]); }
            if (!off && !(fin && ru[1] > 0.0 && ru[2] > 0.0 && ru[3] > 0.0 && ru[3] <= 1.0))
                return invalid(who, "stream %ld: running statistics are six finite values (prior mean, prior std > 0, prior frames "
                                    "> 0, decay in (0, 1], target mean, target std), or six NaN for none", s);
            if (!off && !none) return invalid(who, "stream %ld: given statistics and running statistics exclude each other", s);
        }
        if (tk) {                                       // the frames to emit: up to `lag` behind the final ones, all at the end
            const int64_t ef = tk->emit_first[i], en = tk->emit_n[i];
            const int64_t upto = ended[i] ? f + k : (f + k > tk->t.lag ? f + k - tk->t.lag : 0);
            if (tk->parity[i] & ~1) return invalid(who, "stream %ld: the tracker's parity is 0 or 1", s);
            if (ef < 0 || en < 0 || en > max_frames || ef + en != upto || f + k - ef > cap || (ended[i] && f + k != q))
                return invalid(who, "stream %ld: emits frames [%ld, +%ld), not up to frame %ld", s, ef, en, upto);
            most = en > most ? en : most;
        }
        if (k == 0) continue;
        // every frame is final: it reads up to (f + k - 1) hop + 1023, or the stream has ended and these are its last frames
        if (ended[i] ? f + k != q : (f + k - 1) * hop + LD_NFFT / 2 > q * hop)
            return invalid(who, "stream %ld: frames [%ld, +%ld) are not final with %ld frames seen", s, f, k, q);
        // ... and the ring still holds what the first of them reads: from sample max(0, f hop - 1024) on
        const int64_t lowest = f * hop > LD_NFFT / 2 ? f * hop - LD_NFFT / 2 : 0;
        if (lowest < q * hop - ring_len)
            return invalid(who, "stream %ld: frame %ld reads samples the ring of %ld no longer holds (%ld frames seen)",
                           s, f, ring_len, q);
        most = k > most ? k : most;
    }
    if (most == 0) return FASTSVC_OK;               // (nothing became final: no launch)
    F0Dims d;
    d.hop = hop; d.cap = cap; d.sine_amp = sine_amp; d.noise_amp = noise_amp;
    hipStream_t hs = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < S; b0 += SF_MAX) {
        const int nb = S - b0 < SF_MAX ? S - b0 : SF_MAX;
        F0Args a;
        F0Shift sh;
        F0Seeds sd;
        RunArgs ra;
        TrackArgs ta;
        int grid = 0, nrun = 0, gnew = 0;
        for (int i = 0; i < SF_MAX; ++i) {
            const bool on = i < nb;
            const double* st = stats + 4 * (b0 + (on ? i : 0));
            const bool shift = on && st[0] == st[0];
            a.n[i] = on ? n[b0 + i] : 0;
            a.slot[i] = on ? stream[b0 + i] : 0;
            a.first[i] = on ? (long)first_frame[b0 + i] : 0;
            a.samples[i] = on ? (long)seen[b0 + i] * hop : 0;
            sd.seed[i] = on ? (unsigned long long)seed[b0 + i] : 0ull;
            a.flags[i] = on ? ((first_frame[b0 + i] == 0 ? 1 : 0) | (parity[b0 + i] << 1) | (ended[b0 + i] << 2) | (shift ? 8 : 0)) : 0;
            sh.m0[i] = shift ? st[0] : 0.0;
            sh.ratio[i] = shift ? st[3] / st[1] : 1.0;      // (one double division, as numpy does it on the host)
            sh.m1[i] = shift ? st[2] : 0.0;
            if (tk) {
                // the tracker takes the newly final frames; everything behind it - the running shift, the excitation - the
                // emitted ones, as if they were the call's
                ta.first[i] = a.first[i]; ta.n[i] = a.n[i]; ta.slot[i] = a.slot[i];
                ta.efirst[i] = on ? (long)tk->emit_first[b0 + i] : 0;
                ta.en[i] = on ? tk->emit_n[b0 + i] : 0;
                ta.flags[i] = on ? (tk->parity[b0 + i] | (shift ? 8 : 0)) : 0;
                gnew = a.n[i] > gnew ? a.n[i] : gnew;
            }
            const long efirst = tk ? ta.efirst[i] : a.first[i];
            const int en = tk ? ta.en[i] : a.n[i];
            grid = en > grid ? en : grid;
            const double* ru = running ? running + 6 * (b0 + (on ? i : 0)) : nullptr;
            if (ru && on && en > 0 && ru[0] == ru[0]) {
                ra.mp[nrun] = ru[0]; ra.n0[nrun] = ru[2]; ra.prior[nrun] = ru[2] * ru[1] * ru[1];
                ra.g[nrun] = ru[3]; ra.mt[nrun] = ru[4]; ra.st[nrun] = ru[5];
                ra.pos[nrun] = (int)(efirst % cap);
                ra.slot[nrun] = a.slot[i];
                ra.nf[nrun] = (en << 2) | (parity[b0 + i] << 1) | (efirst == 0 ? 1 : 0);
                ++nrun;
            }
        }
        if (tk) {
            if (gnew == 0 && grid == 0) continue;
            if (gnew)
                hipLaunchKernelGGL(stream_f0_cands_kernel, dim3((unsigned)gnew, (unsigned)nb), dim3(256), 0, hs, a, d, p,
                                   tk->cand_threshold, audio_ring, tk->cand_ring);
            hipLaunchKernelGGL(stream_f0_track_kernel, dim3((unsigned)nb), dim3(256), 0, hs, ta, sh, tk->t, (int)cap, tk->cand_ring,
                               tk->bp_ring, tk->rec, f0_ring, f0s_ring);
            for (int i = 0; i < SF_MAX; ++i) {          // the excitation runs over the emitted frames
                a.first[i] = ta.efirst[i];
                a.n[i] = ta.en[i];
                a.flags[i] = (a.flags[i] & ~1) | (i < nb && ta.efirst[i] == 0 ? 1 : 0);
            }
        }
        if (grid == 0) continue;
        int64_t gx = (((int64_t)grid * hop + 3) / 4 + 255) / 256;
        gx = gx > SF_MAX_BLOCKS ? SF_MAX_BLOCKS : gx;
        if (!tk)
            hipLaunchKernelGGL(stream_f0_frames_kernel, dim3((unsigned)grid, (unsigned)nb), dim3(256), 0, hs, a, sh, d, p, audio_ring,
                               f0_ring, f0s_ring);
        if (nrun) {
            for (int i = nrun; i < SF_MAX; ++i) {       // (entries no block reads)
                ra.mp[i] = ra.n0[i] = ra.prior[i] = ra.g[i] = ra.mt[i] = ra.st[i] = 0.0;
                ra.pos[i] = ra.slot[i] = ra.nf[i] = 0;
            }
            hipLaunchKernelGGL(stream_f0_running_kernel, dim3((unsigned)nrun), dim3(SF_TILE), 0, hs, ra, (int)cap, f0_ring, f0s_ring, rec);
        }
        hipLaunchKernelGGL(stream_f0_excite_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, hs, a, sd, d, sample_rate, f0s_ring,
                           exc_ring, phase);
    }
    if (hipGetLastError() == hipSuccess) return FASTSVC_OK;
    char buf[80];
    snprintf(buf, sizeof buf, "%s: launch failed", who);
    return fastsvc::set_last_error(FASTSVC_E_HIP, buf);
}

}  // namespace

extern "C" {

int fastsvc_stream_f0(const float* audio_ring, float* f0_ring, float* f0s_ring, float* exc_ring, double* phase, int32_t S,
                      const int32_t* stream, const int64_t* first_frame, const int32_t* n, const int64_t* seen,
                      const int32_t* ended, const int32_t* parity, const uint64_t* seed, const double* stats,
                      int32_t n_streams, int32_t cap, int32_t max_frames, int32_t hop, float sample_rate, float f0_floor,
                      float f0_ceil, float threshold, float sine_amp, float noise_amp, void* stream_) {
    return stream_f0_run("fastsvc_stream_f0", nullptr, audio_ring, f0_ring, f0s_ring, exc_ring, phase, nullptr, S, stream, first_frame, n,
                         seen, ended, parity, seed, stats, nullptr, n_streams, cap, max_frames, hop, sample_rate, f0_floor,
                         f0_ceil, threshold, sine_amp, noise_amp, stream_);
}

int fastsvc_stream_f0_running(const float* audio_ring, float* f0_ring, float* f0s_ring, float* exc_ring, double* phase,
                              double* stats_record, int32_t S, const int32_t* stream, const int64_t* first_frame,
                              const int32_t* n, const int64_t* seen, const int32_t* ended, const int32_t* parity,
                              const uint64_t* seed, const double* stats, const double* running, int32_t n_streams, int32_t cap,
                              int32_t max_frames, int32_t hop, float sample_rate, float f0_floor, float f0_ceil, float threshold,
                              float sine_amp, float noise_amp, void* stream_) {
    const char* who = "fastsvc_stream_f0_running";
    if (!stats_record || !running) return invalid(who, "null pointer (the statistics record or the running constants)");
    return stream_f0_run(who, nullptr, audio_ring, f0_ring, f0s_ring, exc_ring, phase, stats_record, S, stream, first_frame, n, seen, ended,
                         parity, seed, stats, running, n_streams, cap, max_frames, hop, sample_rate, f0_floor, f0_ceil, threshold,
                         sine_amp, noise_amp, stream_);
}

int fastsvc_stream_f0_tracked(const float* audio_ring, float* cand_ring, void* bp_ring, float* f0_ring, float* f0s_ring,
                              float* exc_ring, double* phase, double* stats_record, double* track_record, int32_t S,
                              const int32_t* stream, const int64_t* first_frame, const int32_t* n, const int64_t* seen,
                              const int32_t* ended, const int32_t* parity, const int32_t* track_parity, const int64_t* emit_first,
                              const int32_t* emit_n, const uint64_t* seed, const double* stats, const double* running,
                              int32_t n_streams, int32_t cap, int32_t max_frames, int32_t hop, float sample_rate, float f0_floor,
                              float f0_ceil, float cand_threshold, int32_t lag, double lag_bias, double jump, double switch_cost,
                              double unvoiced, float sine_amp, float noise_amp, void* stream_) {
    const char* who = "fastsvc_stream_f0_tracked";
    if (!cand_ring || !bp_ring || !track_record || !track_parity || !emit_first || !emit_n)
        return invalid(who, "null pointer (the tracker's rings, record, parity or frames to emit)");
    if (running && !stats_record) return invalid(who, "null pointer (running constants without a statistics record)");
    if ((reinterpret_cast<uintptr_t>(cand_ring) & 3) || (reinterpret_cast<uintptr_t>(track_record) & 7))
        return invalid(who, "misaligned pointer (the candidate ring: 4 bytes, the tracker record: 8)");
    const double costs[4] = {lag_bias, jump, switch_cost, unvoiced};
    for (double c : costs)
        if (!(c >= 0.0 && is_finite(c))) return invalid(who, "the tracker's costs are finite and >= 0");
    if (lag < 0 || lag > F0_TRACK_MAX_LAG) return invalid(who, "lag %ld outside [0, %ld]", lag, F0_TRACK_MAX_LAG);
    TrackCall tk;
    tk.cand_ring = cand_ring; tk.bp_ring = static_cast<unsigned char*>(bp_ring); tk.rec = track_record;
    tk.parity = track_parity; tk.emit_first = emit_first; tk.emit_n = emit_n; tk.cand_threshold = cand_threshold;
    tk.t.lag_bias = lag_bias; tk.t.jump = jump; tk.t.sw = switch_cost; tk.t.unvoiced = unvoiced; tk.t.sr = sample_rate; tk.t.lag = lag;
    int32_t tau_min = 0, tau_max = 0;
    if (const int rc = fastsvc_f0_lags(sample_rate, f0_floor, f0_ceil, &tau_min, &tau_max)) return rc;
    tk.t.tau_max = (double)tau_max;
    // (the threshold of the per-frame pick has no part here: the unvoiced state's cost takes its place)
    return stream_f0_run(who, &tk, audio_ring, f0_ring, f0s_ring, exc_ring, phase, stats_record, S, stream, first_frame, n, seen,
                         ended, parity, seed, stats, running, n_streams, cap, max_frames, hop, sample_rate, f0_floor, f0_ceil,
                         cand_threshold, sine_amp, noise_amp, stream_);
}

}  // extern "C"
