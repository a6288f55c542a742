// fastsvc_pack.hip - the device twin of fastsvc_pack_weights (fastsvc_plan.cpp): parameters that are already on the
// GPU -> the kernel-layout weight blob, byte for byte what the host packer writes, asynchronously on the caller's stream.
//
// A training step re-packs after every optimizer update; through the host that is an 11 MB download, 30 ms of packing on a
// thread pool and a 65 MB upload, on the critical path of a step that is bound by the host already.  Here it is a dozen
// launches that read 11 MB and write 65 MB of device memory.
//
// BYTE IDENTITY is the contract, so the arithmetic is the host's, operation for operation:
//   - this unit is compiled with -ffp-contract=off (build.py): fastsvc_plan.cpp is plain x86-64 code without a single
//     fused multiply-add, so `ss += v * v`, `sa += m * a[ci]` must stay a multiply and an add here too;
//   - every sum runs sequentially in the host's index order, one thread per row (float32 for the weight-norm fold,
//     float64 for the l1 sums and the (alpha, beta) recurrences); rows are a few hundred, terms a few thousand;
//   - sqrt and the division of the fold are the correctly rounded forms (a build flag of this unit, see build.py); ldexp, rint, the float64 -> float32 casts are
//     exact / round-to-nearest-even as on the host; float32 denormals are kept (gfx950 code objects preserve them by
//     default, the host sets no flush mode: the square of a 1e-20 weight_v IS a denormal);
//   - comparisons are written as std::max has them (`m < x ? x : m`: a NaN never replaces the running maximum);
//   - the binary16 / bfloat16 conversions are the host's bit manipulation (own NaN, subnormal and carry behaviour), not
//     the hardware's converts.
// One difference survives, outside anything a finite parameter set produces: an invalid operation (inf - inf in the
// lo piece of an infinite weight, 0 / 0 in the fold of an all-zero weight_v row) yields x86's negative default NaN on the
// host and the positive one here.  NaNs that come IN with the parameters propagate identically.
//
// Layout of the work: the destination index is the thread index (the blob is written in fragment order with 16-byte or
// consecutive 4-byte stores), the 11 MB of folded sources are gathered through the caches.  No LDS, no matrix
// instructions, no atomics: two packs of the same parameters give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fastsvc_pack.h"

namespace fastsvc_pack {
namespace {

// ---- the host's conversions (fastsvc_plan.cpp: f32_to_f16, f16_to_f32, f32_to_bf16), as written there ----
__device__ inline uint32_t f32_to_f16(float f) {
    uint32_t x = __float_as_uint(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return sign | 0x7e00u;                             // NaN
    if (x >= 0x47800000u) return sign | 0x7c00u;                            // >= 65536: inf
    if (x < 0x38800000u) {                                                  // below 2^-14: subnormal, n * 2^-24
        const float a = __uint_as_float(x);
        return sign | (uint32_t)(int)rintf(a * 16777216.0f);                // nearest even, as lrintf
    }
    const uint32_t mant = x & 0x7fffffu;
    uint32_t h = (((x >> 23) - 112u) << 10) | (mant >> 13);
    const uint32_t rem = mant & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
    return (sign | h) & 0xffffu;
}

__device__ inline float f16_to_f32(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t x;
    if (e == 0) x = __float_as_uint(ldexpf((float)m, -24));
    else if (e == 31) x = 0x7f800000u | (m << 13);
    else x = ((e + 112u) << 23) | (m << 13);
    return __uint_as_float(x | sign);
}

__device__ inline uint32_t f32_to_bf16(float f) {
    const uint32_t x = __float_as_uint(f);
    if ((x & 0x7fffffffu) > 0x7f800000u) return ((x >> 16) | 0x40u) & 0xffffu;
    return ((x + 0x7fffu + ((x >> 16) & 1u)) >> 16) & 0xffffu;
}

__device__ inline float max_keep(float m, float x) { return m < x ? x : m; }        // std::max(m, x)

// job whose [work0, next work0) holds `idx` (work0 ascending, jobs[0].work0 == 0)
template <typename J>
__device__ inline int find_job(const J* jobs, int n, uint32_t idx) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].work0 <= idx) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <typename T>
__device__ inline const T* table_at(const void* scratch, uint32_t byte_off) {
    return reinterpret_cast<const T*>(static_cast<const char*>(scratch) + byte_off);
}

// The row sums below are chains of dependent adds in the host's order; what they wait for is memory (a thread walks its
// own row, nothing is coalesced), so the loads of PK_AHEAD terms are issued together in front of their adds: same
// operations, same order, an eighth of the round trips.
constexpr int PK_AHEAD = 8;

__device__ inline double abs_sum_f64(const float* w, uint32_t n) {         // sum += fabs((double)w[i]), i ascending
    double sum = 0.0;
    uint32_t i = 0;
    for (; i + PK_AHEAD <= n; i += PK_AHEAD) {
        float t[PK_AHEAD];
#pragma unroll
        for (int j = 0; j < PK_AHEAD; ++j) t[j] = w[i + j];
#pragma unroll
        for (int j = 0; j < PK_AHEAD; ++j) sum += fabs((double)t[j]);
    }
    for (; i < n; ++i) sum += fabs((double)w[i]);
    return sum;
}

// W0 + W1 + W2 of the polyphase middle tap, in float64 (MODE_POLY)
__device__ inline float poly_mid(const float* w) { return (float)((double)w[0] + (double)w[1] + (double)w[2]); }

// ---- 1. weight-norm scale per output channel: sc = g / sqrt(sum v^2), the sum in index order ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_rowscale_kernel(PkPtrs ptrs, float* __restrict__ scratch, uint32_t layers_off, int layer0) {
    const PkLayer L = table_at<PkLayer>(scratch, layers_off)[layer0 + blockIdx.y];
    const uint32_t co = blockIdx.x * PK_BLOCK + threadIdx.x;
    const float* g = ptrs.p[3 * blockIdx.y + 2];
    if (co >= L.cout || g == nullptr) return;
    const float* v = ptrs.p[3 * blockIdx.y + 1] + (size_t)co * L.per;
    float ss = 0.f;
    uint32_t i = 0;
    for (; i + PK_AHEAD <= L.per; i += PK_AHEAD) {
        float t[PK_AHEAD];
#pragma unroll
        for (int j = 0; j < PK_AHEAD; ++j) t[j] = v[i + j];
#pragma unroll
        for (int j = 0; j < PK_AHEAD; ++j) ss += t[j] * t[j];
    }
    for (; i < L.per; ++i) ss += v[i] * v[i];
    // sqrtf and `/` ARE the correctly rounded forms in this unit (-fhip-fp32-correctly-rounded-divide-sqrt, build.py);
    // __fsqrt_rn is not - this toolchain's headers map it to the native, 1-ulp square root
    scratch[L.s_sc + co] = g[co] / sqrtf(ss);
}

// ---- 2. fold: w = v * sc (or the tensor as it is), and the bias copy ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_fold_kernel(PkPtrs ptrs, float* __restrict__ scratch, uint32_t layers_off, int layer0) {
    const PkLayer L = table_at<PkLayer>(scratch, layers_off)[layer0 + blockIdx.y];
    const uint32_t i = blockIdx.x * PK_BLOCK + threadIdx.x;
    if (i >= L.cout * L.per) return;
    const float* w = ptrs.p[3 * blockIdx.y + 1];
    float v = w[i];
    if (ptrs.p[3 * blockIdx.y + 2] != nullptr) v = v * scratch[L.s_sc + i / L.per];
    scratch[L.s_w + i] = v;
    if (i < L.cout) scratch[L.s_bias + i] = ptrs.p[3 * blockIdx.y][i];
}

// ---- 3. dense matrices assembled from several layers ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_virt_kernel(float* __restrict__ scratch, PkHeader h) {
    const uint32_t idx = blockIdx.x * PK_BLOCK + threadIdx.x;
    const PkVirt* jobs = table_at<PkVirt>(scratch, h.virts);
    const PkVirt& J = jobs[find_job(jobs, (int)h.n_virt, idx)];
    const uint32_t i = idx - J.work0;
    if (i >= J.rows * J.cin * J.ntaps) return;
    const uint32_t t = i % J.ntaps, ci = (i / J.ntaps) % J.cin, co = i / (J.ntaps * J.cin);
    float v = 0.f;
    for (uint32_t p = 0; p < J.npieces; ++p) {
        const uint32_t r = co - J.piece[p].co_off, c = ci - J.piece[p].ci_off;      // (unsigned: below the offset wraps past rows)
        if (r < J.piece[p].rows && c < J.piece[p].cin) v = scratch[J.piece[p].s_src + ((size_t)r * J.piece[p].cin + c) * J.ntaps + t];
    }
    scratch[J.s_dst + i] = v;
}

// ---- 4. float32 fragments: value of [group][q][lane][m] ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_frag_kernel(const float* __restrict__ scratch, float* __restrict__ blob, PkHeader h) {
    const uint32_t idx = blockIdx.x * PK_BLOCK + threadIdx.x;
    const PkFrag* jobs = table_at<PkFrag>(scratch, h.frags);
    const PkFrag& J = jobs[find_job(jobs, (int)h.n_frag, idx)];
    const uint32_t i = idx - J.work0;
    if (i >= J.ngroups * J.Q * 64 * J.MW) return;
    const uint32_t m = i % J.MW, lane = (i / J.MW) & 63, q = (i / (J.MW * 64)) % J.Q, grp = i / (J.MW * 64 * J.Q);
    const uint32_t co = (grp * J.MW + m) * 16 + (lane & 15);
    uint32_t ci, comp;
    if (J.kind == PK_FRAG_PLAIN || J.kind == PK_FRAG_POLY) {
        // q = (chunk * ntaps + tap) * (KC / 4) + g
        const uint32_t kg = J.KC / 4, g = q % kg, ch = q / (kg * J.ntaps);
        comp = (q / kg) % J.ntaps;
        ci = ch * J.KC + 4 * g + (lane >> 4);
    } else {
        // q = chunk * 24 + (half * 4 + component) * 3 + k-group-in-half
        const uint32_t ch = q / 24, r = q % 24, jj = r % 3, hh = r / 12;
        comp = (r / 3) & 3;
        ci = ch * J.KC + 4 * (3 * hh + jj) + (lane >> 4);
    }
    float v = 0.f;
    if (co < J.cout && ci < J.cin) {
        const float* w = scratch + J.s_src + ((size_t)co * J.cin + ci) * J.ntaps;
        if (J.kind == PK_FRAG_PLAIN) {
            v = w[comp];
        } else if (J.kind == PK_FRAG_POLY) {
            v = comp == 1 ? poly_mid(w) : w[comp];
        } else if (J.kind == PK_FRAG_WINO) {                                // G w of F(2,3), in float64
            const double w0 = w[0], w1 = w[1], w2 = w[2];
            v = comp == 0 ? (float)w0 : comp == 1 ? (float)(0.5 * (w0 + w1 + w2)) : comp == 2 ? (float)(0.5 * (w0 - w1 + w2)) : (float)w2;
        } else {
            v = comp < 3 ? w[comp] : scratch[J.s_src1 + (size_t)co * J.cin + ci];
        }
    }
    blob[J.d_dst + i] = v;
}

// virtual weight Wt[co][unit * 32 + k][slot] of a half-precision job
__device__ inline float hx_value(const float* scratch, const PkHxUnit& U, uint32_t co, uint32_t k, uint32_t slot) {
    const uint32_t cj = U.cj0 + k;
    if (cj >= U.lim) return 0.f;
    if (U.kind == PK_HX_DEC2 && slot == 3) return scratch[U.s_src1 + (size_t)co * U.ld + cj];
    const float* w = scratch + U.s_src + ((size_t)co * U.ld + cj) * 3;
    if (U.kind == PK_HX_POLY && slot == 1) return poly_mid(w);
    return w[slot];
}

// ---- 5. per-channel exponents of the split-binary16 sets and their inverse tables ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_hx_exp_kernel(float* __restrict__ scratch, float* __restrict__ blob, PkHeader h) {
    const uint32_t idx = blockIdx.x * PK_BLOCK + threadIdx.x;
    const PkHx* jobs = table_at<PkHx>(scratch, h.hxs);
    int lo = 0, hi = (int)h.n_hx - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].row0 <= idx) lo = mid; else hi = mid - 1;
    }
    const PkHx& J = jobs[lo];
    const uint32_t n16 = J.ngroups * 16 * J.MW, i = idx - J.row0;
    if (i >= J.ntables * n16 || J.d_inv == 0) return;
    const uint32_t t = i / n16, co = i % n16;
    const PkHxUnit* units = table_at<PkHxUnit>(scratch, h.hx_units) + J.unit0;
    // largest magnitude of the table's weights of this channel.  (The host walks them channel by channel, tap by tap;
    // a running maximum that NaNs never replace does not depend on the order, so each unit's 32 x 3 consecutive floats
    // are read as they lie, several in flight.)
    float m = 0.f;
    if (co < J.cout)
        for (uint32_t u = 0; u < J.nch; ++u) {
            const PkHxUnit U = units[u];
            const uint32_t n = U.lim > U.cj0 ? min(32u, U.lim - U.cj0) : 0u;
            if (U.kind == PK_HX_DEC2 && t == 1) {                           // slot 3: the 1x1 conv
                const float* w = scratch + U.s_src1 + (size_t)co * U.ld + U.cj0;
#pragma unroll 8
                for (uint32_t k = 0; k < n; ++k) m = max_keep(m, fabsf(w[k]));
            } else if (U.table == t) {
                const float* w = scratch + U.s_src + ((size_t)co * U.ld + U.cj0) * 3;
#pragma unroll 4
                for (uint32_t k = 0; k < n; ++k) {
                    const float w0 = w[3 * k], w1 = w[3 * k + 1], w2 = w[3 * k + 2];
                    const float mid = U.kind == PK_HX_POLY ? (float)((double)w0 + (double)w1 + (double)w2) : w1;
                    m = max_keep(max_keep(max_keep(m, fabsf(w0)), fabsf(mid)), fabsf(w2));
                }
            }
        }
    int e = 0;
    const uint32_t mb = __float_as_uint(m);
    if (m > 0.f && mb < 0x7f800000u) {                                      // finite: 14 - ilogb(m), clamped (a denormal's ilogb is < -126)
        const int ef = (int)(mb >> 23);
        e = ef == 0 ? 60 : min(60, max(-60, 14 - (ef - 127)));
    }
    reinterpret_cast<int*>(scratch)[J.s_ex + i] = e;
    blob[J.d_inv + i] = ldexpf(1.0f, -e);
}

// ---- 6. half-precision fragments: one thread per (fragment, lane) = 8 consecutive input channels, 16-byte stores ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_hx_kernel(const float* __restrict__ scratch, float* __restrict__ blob, PkHeader h) {
    const uint32_t idx = blockIdx.x * PK_BLOCK + threadIdx.x;
    const PkHx* jobs = table_at<PkHx>(scratch, h.hxs);
    const PkHx& J = jobs[find_job(jobs, (int)h.n_hx, idx)];
    const uint32_t i = idx - J.work0;
    if (i >= J.ngroups * J.nch * J.nslots * J.MW * 64) return;
    const uint32_t lane = i & 63, f = i >> 6;                               // f = ((grp * nch + ch) * nslots + slot) * MW + m
    const uint32_t m = f % J.MW, slot = (f / J.MW) % J.nslots, ch = (f / (J.MW * J.nslots)) % J.nch, grp = f / (J.MW * J.nslots * J.nch);
    const uint32_t co = (grp * J.MW + m) * 16 + (lane & 15), k0 = 8 * (lane >> 4);
    const PkHxUnit U = (table_at<PkHxUnit>(scratch, h.hx_units) + J.unit0)[ch];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = co < J.cout ? hx_value(scratch, U, co, k0 + e, slot) : 0.f;
    if (J.d_off[0]) {
        int ex = 0;
        if (J.d_inv) {
            const uint32_t n16 = J.ngroups * 16 * J.MW, t = U.table + (U.kind == PK_HX_DEC2 && slot == 3 ? 1u : 0u);
            ex = reinterpret_cast<const int*>(scratch)[J.s_ex + t * n16 + co];
        }
        uint32_t hi[8], lo[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float s = J.d_inv ? ldexpf(v[e], ex) : v[e];
            hi[e] = f32_to_f16(s);
            lo[e] = f32_to_f16(s - f16_to_f32(hi[e]));
        }
        uint4* dst = reinterpret_cast<uint4*>(blob + J.d_off[0]) + (size_t)f * 128 + lane;      // 2 pieces x 1 KB per fragment
        dst[0] = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
        dst[64] = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
    }
    if (J.d_off[1]) {
        uint32_t b[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] = f32_to_bf16(v[e]);
        reinterpret_cast<uint4*>(blob + J.d_off[1])[(size_t)f * 64 + lane] =
            make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
    }
    if (J.d_off[2]) {
        uint32_t b[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] = f32_to_f16(v[e]);
        reinterpret_cast<uint4*>(blob + J.d_off[2])[(size_t)f * 64 + lane] =
            make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
    }
}

// ---- 7. plain rows: raw weights, biases, the heads' bias sums ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_copy_kernel(const float* __restrict__ scratch, float* __restrict__ blob, PkHeader h) {
    const uint32_t idx = blockIdx.x * PK_BLOCK + threadIdx.x;
    const PkCopy* jobs = table_at<PkCopy>(scratch, h.copies);
    const PkCopy& J = jobs[find_job(jobs, (int)h.n_copy, idx)];
    const uint32_t i = idx - J.work0;
    if (i >= J.n) return;
    float v = scratch[J.s_a + i];
    if (J.mode >= 1) v = 0.f + v;                                           // (the host accumulates into a zeroed row: -0 becomes +0)
    if (J.mode == 2) v = v + scratch[J.s_b + i];
    blob[J.d_dst + i] = v;
}

// ---- 8. (l1, bmax) pairs: one block per pair, a thread per row, then the maximum over the rows ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_bound_kernel(const float* __restrict__ scratch, float* __restrict__ blob, PkHeader h) {
    __shared__ float red[2][PK_BLOCK];
    const PkBound J = table_at<PkBound>(scratch, h.bounds)[blockIdx.x];
    float l1 = 0.f, bmax = 0.f;
    for (uint32_t r = threadIdx.x; r < J.rows; r += PK_BLOCK) {
        l1 = max_keep(l1, (float)abs_sum_f64(scratch + J.s_w + (size_t)r * J.per, J.per));
        const uint32_t hh = r >= J.half ? 1u : 0u, rr = r - hh * J.half;
        float b = scratch[J.s_a[hh] + rr];
        if (J.s_b[hh] != PK_NONE) b = (0.f + b) + scratch[J.s_b[hh] + rr];
        bmax = max_keep(bmax, fabsf(b));
    }
    // (every partial maximum is a non-NaN value >= 0: the maximum of the partials is the host's sequential one)
    red[0][threadIdx.x] = l1;
    red[1][threadIdx.x] = bmax;
    __syncthreads();
    for (int s = PK_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] = max_keep(red[0][threadIdx.x], red[0][threadIdx.x + s]);
            red[1][threadIdx.x] = max_keep(red[1][threadIdx.x], red[1][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        blob[J.d_dst] = red[0][0];
        blob[J.d_dst + 1] = red[1][0];
    }
}

// ---- 9. (alpha, beta) recurrences of a conditioning stage: one block per (stage, signal), a thread per channel ----
__global__ __launch_bounds__(PK_BLOCK)
void pack_cond_kernel(float* __restrict__ scratch, float* __restrict__ blob, PkHeader h) {
    const PkCond J = table_at<PkCond>(scratch, h.conds)[blockIdx.x];
    const uint32_t C = J.C, Cin = J.Cin;
    double* a = reinterpret_cast<double*>(scratch + J.s_tmp);
    double* b = a + C;
    double* a2 = b + C;
    double* b2 = a2 + C;
    float* out = blob + J.d_dst;
    auto emit = [&](uint32_t t, const double* pa, const double* pb) {
        for (uint32_t c = threadIdx.x; c < C; c += PK_BLOCK) {
            out[(t * 2 + 0) * C + c] = (float)(pa[c] * 1.0000005);
            out[(t * 2 + 1) * C + c] = (float)(pb[c] * 1.0000005);
        }
    };
    auto through = [&](int layer, const double* pa, const double* pb, double* qa, double* qb) {
        const float* W = scratch + J.s_w[layer];
        const float* B = scratch + J.s_b[layer];
        for (uint32_t co = threadIdx.x; co < C; co += PK_BLOCK) {
            double sa = 0.0, sb = 0.0;
            for (uint32_t ci = 0; ci < C; ++ci) {
                const float* w = W + ((size_t)co * C + ci) * 3;
                const double m = fabs((double)w[0]) + fabs((double)w[1]) + fabs((double)w[2]);
                sa += m * pa[ci];
                sb += m * pb[ci];
            }
            qa[co] = sa;
            qb[co] = sb + fabs((double)B[co]);
        }
    };
    for (uint32_t c = threadIdx.x; c < C; c += PK_BLOCK) {
        a[c] = abs_sum_f64(scratch + J.s_w[0] + (size_t)c * Cin * 3, Cin * 3);
        b[c] = fabs((double)scratch[J.s_b[0] + c]);
    }
    __syncthreads();
    emit(0, a, b);
    through(2, a, b, a2, b2);
    __syncthreads();
    emit(1, a2, b2);
    through(3, a2, b2, a, b);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < C; c += PK_BLOCK) {                  // + the 1x1 residual conv of the stage's input
        a[c] += abs_sum_f64(scratch + J.s_w[1] + (size_t)c * Cin, Cin);
        b[c] += fabs((double)scratch[J.s_b[1] + c]);
    }
    __syncthreads();
    emit(2, a, b);
    through(4, a, b, a2, b2);
    __syncthreads();
    emit(3, a2, b2);
}

inline unsigned blocks_of(uint32_t work) { return (work + PK_BLOCK - 1) / PK_BLOCK; }

}  // namespace

int launch_pack(const PkHeader& h, const void* pinned_table, const float* const* ptrs, void* dev_blob, size_t blob_bytes,
                void* scratch_, void* stream_, int* n_launches) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float* scratch = static_cast<float*>(scratch_);
    float* blob = static_cast<float*>(dev_blob);
    int n = 0;
    hipError_t rc = hipMemcpyAsync(static_cast<char*>(scratch_) + h.table_off, pinned_table, h.table_bytes, hipMemcpyHostToDevice, stream);
    ++n;
    if (rc != hipSuccess) return (int)rc;
    rc = hipMemsetAsync(dev_blob, 0, blob_bytes, stream);                    // padding granules, absent formats
    ++n;
    if (rc != hipSuccess) return (int)rc;
    for (uint32_t l0 = 0; l0 < h.n_layers; l0 += PK_PTR_LAYERS) {
        const uint32_t nl = h.n_layers - l0 < (uint32_t)PK_PTR_LAYERS ? h.n_layers - l0 : (uint32_t)PK_PTR_LAYERS;
        PkPtrs a;
        for (uint32_t i = 0; i < 3u * PK_PTR_LAYERS; ++i) a.p[i] = i < 3 * nl ? ptrs[3 * l0 + i] : nullptr;
        hipLaunchKernelGGL(pack_rowscale_kernel, dim3(blocks_of(h.max_rows), nl), dim3(PK_BLOCK), 0, stream, a, scratch, h.layers, (int)l0);
        hipLaunchKernelGGL(pack_fold_kernel, dim3(blocks_of(h.max_w), nl), dim3(PK_BLOCK), 0, stream, a, scratch, h.layers, (int)l0);
        n += 2;
    }
    if (h.n_virt) { hipLaunchKernelGGL(pack_virt_kernel, dim3(blocks_of(h.virt_work)), dim3(PK_BLOCK), 0, stream, scratch, h); ++n; }
    if (h.n_frag) { hipLaunchKernelGGL(pack_frag_kernel, dim3(blocks_of(h.frag_work)), dim3(PK_BLOCK), 0, stream, scratch, blob, h); ++n; }
    if (h.n_hx) {
        hipLaunchKernelGGL(pack_hx_exp_kernel, dim3(blocks_of(h.hx_rows)), dim3(PK_BLOCK), 0, stream, scratch, blob, h);
        hipLaunchKernelGGL(pack_hx_kernel, dim3(blocks_of(h.hx_work)), dim3(PK_BLOCK), 0, stream, scratch, blob, h);
        n += 2;
    }
    if (h.n_copy) { hipLaunchKernelGGL(pack_copy_kernel, dim3(blocks_of(h.copy_work)), dim3(PK_BLOCK), 0, stream, scratch, blob, h); ++n; }
    if (h.n_bound) { hipLaunchKernelGGL(pack_bound_kernel, dim3(h.n_bound), dim3(PK_BLOCK), 0, stream, scratch, blob, h); ++n; }
    if (h.n_cond) { hipLaunchKernelGGL(pack_cond_kernel, dim3(h.n_cond), dim3(PK_BLOCK), 0, stream, scratch, blob, h); ++n; }
    if (n_launches) *n_launches = n;
    return (int)hipGetLastError();
}

}  // namespace fastsvc_pack
