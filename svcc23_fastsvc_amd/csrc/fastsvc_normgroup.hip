// fastsvc_normgroup.hip - InstanceNorm sums pooled over GROUPS of batch rows (fastsvc_forward_grouped; the windows of one
// utterance in decode.DecodeSession.convert_windowed(norm="utterance")).
//
// Every norm point of an up block reads, per (row, channel), sum u and sum u^2 of a FiLM-affined tensor and divides them
// by the row's own length (fastsvc_hx.hip / fastsvc_wx.hip / fastsvc_kernels.hip set-up).  Here the sums are taken over
// the columns each row OWNS, pooled over the rows of a group and written back scaled by (row length / owned columns of
// the group), so that those unchanged consumers normalise every row of a group by the GROUP's mean and variance
// (fastsvc_kernels.h has the contract of the two launches, DESIGN.md 4.9 the argument why that is the whole utterance's).
//
// partials: a streaming read, HBM-bound.  The unit of work is one WAVE on one (row, channel, chunk of NORMGROUP_CHUNK
// columns): 192 channels x 800 columns (block 0) are 192 waves a row, 24 x 64 000 (block 3) are 768 - no workgroup shape
// tied to the row length, four independent waves per workgroup, no LDS, no barrier.  16-byte requests (4 float32 / 8
// two-byte elements a lane) over the 16-byte aligned middle of the chunk, four in flight per lane; the up to 15 bytes in
// front and behind go element-wise, so own_lo * len_mul may sit anywhere (block 0: 8 bytes into a word for odd own_lo).
// Every element and every product in float64 (a float32 squared is exact there), lanes combined by a fixed butterfly:
// no atomics, the same bits on every run and in every batch.
//
// RUNNING sums (fastsvc_forward_running; decode.StreamSession(norm="running")): the rows are windows of live streams, and
// the sums of a stream's earlier windows come out of a carry that survives from forward to forward.  The same wave per
// chunk over two ranges a row, core and look-ahead, and a PREFIX pool in place of the group pool: carry, earlier cores of
// the slot in the batch, own core (the new carry), look-ahead (the statistics) - one left fold in float64, so the bits do
// not depend on how windows fall into forwards.  The carry is a pair of entries per slot: a launch reads entry `parity` and
// writes entry `parity ^ 1`, no workgroup reads what another writes (fastsvc_kernels.h).  With a forgetting
// horizon (fastsvc_forward_running_decay) the fold multiplies the running sum by a per-row decay in front of every core.
// Compiled three times (build.py): float32, bfloat16 and binary16 activation storage; the pools are defined once.
#include "fastsvc_kernels.h"

namespace fastsvc {
#ifdef FASTSVC_ACT_2B
namespace FASTSVC_ACT_NS {
#endif

#include "fastsvc_device.inc"

namespace {

// the row's valid frames, its owned frames clamped into them, and whether it is a pass-through row (wave-uniform; every
// lane looks at B / 64 entries of group[])
struct NgRow { int len, lo, hi; bool pass; };
__device__ __forceinline__ NgRow ng_row(int b, int B, int ld, const int* __restrict__ lens, int len_mul,
                                        const int* __restrict__ group, const int* __restrict__ own_lo,
                                        const int* __restrict__ own_hi, int lane) {
    NgRow r;
    const int F = ld / len_mul;
    r.len = lens ? min(max(lens[b], 0), F) : F;
    r.lo = min(max(own_lo[b], 0), r.len);
    r.hi = min(max(own_hi[b], r.lo), r.len);
    const int g = group[b];
    bool other = false;
    for (int q = lane; q < B; q += 64) other |= (q != b && group[q] == g);
    r.pass = g == b && !__any(other) && r.lo == 0 && r.hi == r.len;
    return r;
}

constexpr int NG_VEC = 16 / (int)sizeof(act_t);      // elements of one 16-byte request

__device__ __forceinline__ void ng_acc(double& s1, double& s2, float v) {
    const double d = (double)v;
    s1 += d; s2 += d * d;
}
// one 16-byte request: 8 two-byte elements as four dwords, or four float32
#ifdef FASTSVC_ACT_2B
typedef u32x4 ng_vec_t;
#else
typedef f32x4 ng_vec_t;
#endif
__device__ __forceinline__ void ng_acc16(double& s1, double& s2, const ng_vec_t w) {
#ifdef FASTSVC_ACT_2B
    ng_acc(s1, s2, a16_lo(w.x)); ng_acc(s1, s2, a16_hi(w.x));
    ng_acc(s1, s2, a16_lo(w.y)); ng_acc(s1, s2, a16_hi(w.y));
    ng_acc(s1, s2, a16_lo(w.z)); ng_acc(s1, s2, a16_hi(w.z));
    ng_acc(s1, s2, a16_lo(w.w)); ng_acc(s1, s2, a16_hi(w.w));
#else
    ng_acc(s1, s2, w.x); ng_acc(s1, s2, w.y); ng_acc(s1, s2, w.z); ng_acc(s1, s2, w.w);
#endif
}
__device__ __forceinline__ float ng_elem(const act_t* p) {
#ifdef FASTSVC_ACT_2B
    return a16_lo((unsigned)*p);
#else
    return *p;
#endif
}

// one wave's float64 sums of u and u^2 over the n <= NORMGROUP_CHUNK elements at p, every lane holding them afterwards:
// [0, head) element-wise up to the next 16-byte boundary, nvec 16-byte requests, then the rest element-wise
__device__ __forceinline__ void ng_chunk_sums(const act_t* p, int n, int lane, double& s1, double& s2) {
    const int head = min(n, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(act_t)));
    const int nvec = (n - head) / NG_VEC;
    const int tail0 = head + nvec * NG_VEC;
    s1 = 0.0; s2 = 0.0;
    if (lane < head) ng_acc(s1, s2, ng_elem(p + lane));
    const ng_vec_t* pv = reinterpret_cast<const ng_vec_t*>(p + head);
    int j = lane;
    for (; j + 192 < nvec; j += 256) {                               // four requests in flight per lane
        const ng_vec_t w0 = pv[j], w1 = pv[j + 64], w2 = pv[j + 128], w3 = pv[j + 192];
        ng_acc16(s1, s2, w0); ng_acc16(s1, s2, w1); ng_acc16(s1, s2, w2); ng_acc16(s1, s2, w3);
    }
    for (; j < nvec; j += 64) ng_acc16(s1, s2, pv[j]);
    if (tail0 + lane < n) ng_acc(s1, s2, ng_elem(p + tail0 + lane));
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { s1 += __shfl_xor(s1, d); s2 += __shfl_xor(s2, d); }
}

__global__ __launch_bounds__(256)
void norm_group_partials_kernel(const act_t* __restrict__ u, double* __restrict__ part, int B, int C, int ld,
                                const int* __restrict__ lens, int len_mul, const int* __restrict__ group,
                                const int* __restrict__ own_lo, const int* __restrict__ own_hi, int chunks) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);          // (chunk, channel) of row b, channel fastest
    const int b = blockIdx.y;
    const int k = item / C, c = item - k * C;
    if (k >= chunks) return;
    const NgRow r = ng_row(b, B, ld, lens, len_mul, group, own_lo, own_hi, lane);
    if (r.pass) return;
    const long lo = (long)r.lo * len_mul + (long)k * NORMGROUP_CHUNK;
    const long end = (long)r.hi * len_mul;
    if (lo >= end) return;                                           // (the pool reads only the chunks a row has)
    const int n = (int)min((long)NORMGROUP_CHUNK, end - lo);
    double s1, s2;
    ng_chunk_sums(u + ((long)b * C + c) * ld + lo, n, lane, s1, s2);
    if (lane == 0) {
        double* o = part + (((long)b * chunks + k) * C + c) * 2;
        o[0] = s1; o[1] = s2;
    }
}

// ---- running statistics (fastsvc_forward_running): the rows are windows of live streams, see fastsvc_kernels.h ----
// the row's valid frames, its core [lo, hi) clamped into them (the look-ahead is [hi, len)), the frames of its stream
// in front of the core, and whether it is a pass-through row: the first window of a stream, which owns its whole row
struct NrRow { int len, lo, hi; long prior; bool pass; };
__device__ __forceinline__ NrRow nr_row(int b, int ld, const int* __restrict__ lens, int len_mul,
                                        const int* __restrict__ own_lo, const int* __restrict__ own_hi,
                                        const int* __restrict__ prior, const int* __restrict__ reset) {
    NrRow r;
    const int F = ld / len_mul;
    r.len = lens ? min(max(lens[b], 0), F) : F;
    r.lo = min(max(own_lo[b], 0), r.len);
    r.hi = min(max(own_hi[b], r.lo), r.len);
    r.prior = max(prior[b], r.lo);
    r.pass = reset[b] != 0 && r.lo == 0;
    return r;
}

// the partials kernel with two ranges a row (blockIdx.z): 0 the core, 1 the look-ahead, each cut into chunks from its
// own start -> part[((b * 2 + range) * chunks + k) * C + c][2]
__global__ __launch_bounds__(256)
void norm_running_partials_kernel(const act_t* __restrict__ u, double* __restrict__ part, int C, int ld,
                                  const int* __restrict__ lens, int len_mul, const int* __restrict__ own_lo,
                                  const int* __restrict__ own_hi, const int* __restrict__ prior,
                                  const int* __restrict__ reset, int chunks) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);          // (chunk, channel) of row b, channel fastest
    const int b = blockIdx.y, range = blockIdx.z;
    const int k = item / C, c = item - k * C;
    if (k >= chunks) return;
    const NrRow r = nr_row(b, ld, lens, len_mul, own_lo, own_hi, prior, reset);
    if (range == 1 && r.pass) return;                                // (its statistics stay the producer's)
    const long lo = (long)(range ? r.hi : r.lo) * len_mul + (long)k * NORMGROUP_CHUNK;
    const long end = (long)(range ? r.len : r.hi) * len_mul;
    if (lo >= end) return;                                           // (the pool reads only the chunks a range has)
    const int n = (int)min((long)NORMGROUP_CHUNK, end - lo);
    double s1, s2;
    ng_chunk_sums(u + ((long)b * C + c) * ld + lo, n, lane, s1, s2);
    if (lane == 0) {
        double* o = part + ((((long)b * 2 + range) * chunks + k) * C + c) * 2;
        o[0] = s1; o[1] = s2;
    }
}

#ifndef FASTSVC_ACT_2B
// one thread per (row, channel): the partials are (row, chunk, channel) with the channel fastest, so a wave's reads are
// one contiguous run per (row, chunk)
__global__ __launch_bounds__(64)
void norm_group_pool_kernel(const double* __restrict__ part, double* __restrict__ st, int B, int C, int ld,
                            const int* __restrict__ lens, int len_mul, const int* __restrict__ group,
                            const int* __restrict__ own_lo, const int* __restrict__ own_hi, int chunks,
                            float* __restrict__ amax_raise) {
    const int lane = threadIdx.x;
    const int c = blockIdx.x * 64 + lane, b = blockIdx.y;
    const NgRow me = ng_row(b, B, ld, lens, len_mul, group, own_lo, own_hi, lane);
    if (me.pass) return;
    const int F = ld / len_mul;
    const int g = group[b];
    double s1 = 0.0, s2 = 0.0;
    long N = 0;
    for (int q = 0; q < B; ++q) {
        if (group[q] != g) continue;
        const int len = lens ? min(max(lens[q], 0), F) : F;
        const int lo = min(max(own_lo[q], 0), len), hi = min(max(own_hi[q], lo), len);
        const long cols = (long)(hi - lo) * len_mul;
        N += cols;
        const int nk = (int)((cols + NORMGROUP_CHUNK - 1) / NORMGROUP_CHUNK);
        if (c < C)
            for (int k = 0; k < nk; ++k) {
                const double* o = part + (((long)q * chunks + k) * C + c) * 2;
                s1 += o[0]; s2 += o[1];
            }
    }
    const double L = (double)((long)me.len * len_mul);
    if (c < C && N > 0) {
        st[((long)b * C + c) * 2 + 0] = s1 * L / (double)N;
        st[((long)b * C + c) * 2 + 1] = s2 * L / (double)N;
    }
    // the consumer bounds the normalised row by max |p| + sqrt(L); with the group's statistics it is sqrt(N): slot 0 of the
    // entry takes the entry's maximum plus the difference, rounded up (readers take the maximum of the slots)
#ifndef FASTSVC_EXP_NG_NORAISE      // (A/B builds: what tests/test_decode_window_norm_gpu.py's loud window does without the adjustment)
    if (amax_raise && c == 0 && (double)N > L) {
        float* e = amax_raise + (long)b * AMAX_ENTRY;
        float m = 0.f;
        #pragma unroll
        for (int s = 0; s < AMAX_W; ++s) m = fmaxf(m, e[s * AMAX_STRIDE]);
        const float d = (float)(sqrt((double)N) - sqrt(L));
        e[0] = (m + d) * 1.00001f;
    }
#endif
}
// one thread per (row, channel), as the group pool.  carry: entry e (0 / 1) of slot s at carry + s * slot_stride + e *
// parity_stride, C x 2 doubles.  A launch READS entry parity[b] and WRITES entry parity[b] ^ 1 of the slots it touches;
// all rows of a slot carry the same parity, so no workgroup of the launch reads what another writes.
// DECAY (fastsvc_forward_running_decay): the running sum is multiplied by decay[q] in front of every row q's core - one
// rounding at a fixed place of the fold (__dmul_rn: never contracted into the addition behind it) - the population is
// weight[b] frames, a double, and the raise comes from bound[b] frames (fastsvc_kernels.h).
template <bool DECAY>
__device__ __forceinline__ void nr_pool(const double* __restrict__ part, double* __restrict__ st, int B, int C, int ld,
                                        const int* __restrict__ lens, int len_mul, const int* __restrict__ slot,
                                        const int* __restrict__ own_lo, const int* __restrict__ own_hi,
                                        const int* __restrict__ prior, const int* __restrict__ reset,
                                        const int* __restrict__ parity, double* carry, long slot_stride, long parity_stride,
                                        int chunks, float* __restrict__ amax_raise, const double* __restrict__ decay,
                                        const double* __restrict__ weight, const double* __restrict__ bound) {
    const int c = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    const NrRow me = nr_row(b, ld, lens, len_mul, own_lo, own_hi, prior, reset);
    const int sl = slot[b], par = parity[b] & 1;
    const double L = (double)((long)me.len * len_mul);
    double N, NB;                                                    // columns of the population; of the row's bound
    if constexpr (DECAY) {
        N = weight[b] * (double)len_mul;
        NB = bound[b] * (double)len_mul;
    } else {
        N = (double)((me.prior + me.len - me.lo) * len_mul);
        NB = N;
    }
    if (c < C) {
        double* rec = carry + (long)sl * slot_stride + (long)c * 2;
        double s1 = 0.0, s2 = 0.0;
        bool first = true;
        for (int q = 0; q <= b; ++q) {                               // the cores of the slot's rows up to this one
            if (slot[q] != sl) continue;
            // (in front of them the carry - unless the slot's first row of the batch starts a stream: zero, nothing read)
            if (first && !reset[q]) { s1 = rec[par * parity_stride]; s2 = rec[par * parity_stride + 1]; }
            first = false;
            if constexpr (DECAY) {
                const double d = decay[q];
                s1 = __dmul_rn(s1, d); s2 = __dmul_rn(s2, d);
            }
            const NrRow r = nr_row(q, ld, lens, len_mul, own_lo, own_hi, prior, reset);
            const int nk = (int)(((long)(r.hi - r.lo) * len_mul + NORMGROUP_CHUNK - 1) / NORMGROUP_CHUNK);
            for (int k = 0; k < nk; ++k) {
                const double* o = part + ((((long)q * 2) * chunks + k) * C + c) * 2;
                s1 += o[0]; s2 += o[1];
            }
        }
        bool last = true;
        for (int q = b + 1; q < B; ++q) last = last && slot[q] != sl;
        if (last) { rec[(par ^ 1) * parity_stride] = s1; rec[(par ^ 1) * parity_stride + 1] = s2; }
        if (!me.pass) {
            const int nk = (int)(((long)(me.len - me.hi) * len_mul + NORMGROUP_CHUNK - 1) / NORMGROUP_CHUNK);
            for (int k = 0; k < nk; ++k) {
                const double* o = part + ((((long)b * 2 + 1) * chunks + k) * C + c) * 2;
                s1 += o[0]; s2 += o[1];
            }
            if (N > 0) {
                st[((long)b * C + c) * 2 + 0] = s1 * L / N;
                st[((long)b * C + c) * 2 + 1] = s2 * L / N;
            }
        }
    }
    // (the group pool's raise: the bound of a normalised row is sqrt(N) here too - every column of the row is a member;
    // under a horizon a column of the left context weighs less than one, and the bound is sqrt(bound[b] * len_mul))
    if (amax_raise && c == 0 && !me.pass && NB > L) {
        float* e = amax_raise + (long)b * AMAX_ENTRY;
        float m = 0.f;
        #pragma unroll
        for (int s = 0; s < AMAX_W; ++s) m = fmaxf(m, e[s * AMAX_STRIDE]);
        const float d = (float)(sqrt(NB) - sqrt(L));
        e[0] = (m + d) * 1.00001f;
    }
}
__global__ __launch_bounds__(64)
void norm_running_pool_kernel(const double* __restrict__ part, double* __restrict__ st, int B, int C, int ld,
                              const int* __restrict__ lens, int len_mul, const int* __restrict__ slot,
                              const int* __restrict__ own_lo, const int* __restrict__ own_hi,
                              const int* __restrict__ prior, const int* __restrict__ reset,
                              const int* __restrict__ parity, double* carry, long slot_stride, long parity_stride,
                              int chunks, float* __restrict__ amax_raise) {
    nr_pool<false>(part, st, B, C, ld, lens, len_mul, slot, own_lo, own_hi, prior, reset, parity, carry, slot_stride,
                   parity_stride, chunks, amax_raise, nullptr, nullptr, nullptr);
}
__global__ __launch_bounds__(64)
void norm_running_decay_pool_kernel(const double* __restrict__ part, double* __restrict__ st, int B, int C, int ld,
                                    const int* __restrict__ lens, int len_mul, const int* __restrict__ slot,
                                    const int* __restrict__ own_lo, const int* __restrict__ own_hi,
                                    const int* __restrict__ prior, const int* __restrict__ reset,
                                    const int* __restrict__ parity, double* carry, long slot_stride, long parity_stride,
                                    int chunks, float* __restrict__ amax_raise, const double* __restrict__ decay,
                                    const double* __restrict__ weight, const double* __restrict__ bound) {
    nr_pool<true>(part, st, B, C, ld, lens, len_mul, slot, own_lo, own_hi, prior, reset, parity, carry, slot_stride,
                  parity_stride, chunks, amax_raise, decay, weight, bound);
}
#endif

}  // namespace

hipError_t launch_norm_group_partials(const float* u, double* part, int B, int C, int ld, const int* lens, int len_mul,
                                      const int* group, const int* own_lo, const int* own_hi, hipStream_t stream) {
    const int chunks = norm_group_chunks(ld);
    const unsigned gx = (unsigned)(((long)chunks * C + 3) / 4);
    hipLaunchKernelGGL(norm_group_partials_kernel, dim3(gx, (unsigned)B), dim3(256), 0, stream,
                       reinterpret_cast<const act_t*>(u), part, B, C, ld, lens, len_mul, group, own_lo, own_hi, chunks);
    return hipGetLastError();
}

hipError_t launch_norm_running_partials(const float* u, double* part, int B, int C, int ld, const int* lens, int len_mul,
                                        const int* own_lo, const int* own_hi, const int* prior, const int* reset,
                                        hipStream_t stream) {
    const int chunks = norm_group_chunks(ld);
    const unsigned gx = (unsigned)(((long)chunks * C + 3) / 4);
    hipLaunchKernelGGL(norm_running_partials_kernel, dim3(gx, (unsigned)B, 2), dim3(256), 0, stream,
                       reinterpret_cast<const act_t*>(u), part, C, ld, lens, len_mul, own_lo, own_hi, prior, reset, chunks);
    return hipGetLastError();
}

#ifndef FASTSVC_ACT_2B
hipError_t launch_norm_group_pool(const double* part, double* st, int B, int C, int ld, const int* lens, int len_mul,
                                  const int* group, const int* own_lo, const int* own_hi, float* amax_raise, hipStream_t stream) {
    hipLaunchKernelGGL(norm_group_pool_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)B), dim3(64), 0, stream,
                       part, st, B, C, ld, lens, len_mul, group, own_lo, own_hi, norm_group_chunks(ld), amax_raise);
    return hipGetLastError();
}
hipError_t launch_norm_running_pool(const double* part, double* st, int B, int C, int ld, const int* lens, int len_mul,
                                    const int* slot, const int* own_lo, const int* own_hi, const int* prior,
                                    const int* reset, const int* parity, double* carry, long slot_stride,
                                    long parity_stride, float* amax_raise, hipStream_t stream, const double* decay,
                                    const double* weight, const double* bound) {
    const dim3 grid((unsigned)((C + 63) / 64), (unsigned)B);
    if (decay)
        hipLaunchKernelGGL(norm_running_decay_pool_kernel, grid, dim3(64), 0, stream, part, st, B, C, ld, lens, len_mul, slot,
                           own_lo, own_hi, prior, reset, parity, carry, slot_stride, parity_stride, norm_group_chunks(ld),
                           amax_raise, decay, weight, bound);
    else
        hipLaunchKernelGGL(norm_running_pool_kernel, grid, dim3(64), 0, stream, part, st, B, C, ld, lens, len_mul, slot,
                           own_lo, own_hi, prior, reset, parity, carry, slot_stride, parity_stride, norm_group_chunks(ld),
                           amax_raise);
    return hipGetLastError();
}
#endif

#ifdef FASTSVC_ACT_2B
}  // namespace FASTSVC_ACT_NS
#endif
}  // namespace fastsvc
