// fastsvc_stream_check.hip - the per-window output check of live streams on gfx950 (decode.StreamSession(checked=True)).
//
// A forward of a stream session holds window rows of several streams.  Before anything downstream consumes it - the
// stitch, which stages a fade zone for the NEXT push, and the flip of the running InstanceNorm carry, which every later
// window of the stream reads - the session decides per row whether the row has to run again in a wider activation storage.
// fastsvc_output_check does not fit, for two reasons:
//
//   the span   a row is judged on the samples it contributes, y[r, lo:hi) - its emitted run plus the fade zones it stages
//              or a neighbour row reads - not on its first len samples: context that is never emitted must not cost a
//              fallback.  lo and hi are arbitrary sample offsets, so the span's first byte is in general not 16-byte
//              aligned: the body [first 16-byte boundary at or after lo, last one at or before hi) is read with 16-byte
//              loads, the up to 3 + 3 samples of head and tail with element loads by six lanes, and no lane reads a
//              sample outside [lo, hi) into the report;
//   the carry  the fourth word of the report counts the non-finite doubles of the carry entry the forward just wrote for
//              the row's stream (entry_doubles doubles, a few KB): a poisoned carry is what kills a stream for good.
//
// One workgroup of 256 lanes per row, one launch per 64 rows (the rows' descriptors travel in the kernel arguments, like
// PcmArgs in fastsvc_decodeio.hip).  The largest span of the recipe is (32 + 2 * 10) frames * 320 = 16 640 samples, 65 KB:
// 16 or 17 16-byte loads per lane, independent of each other (the loop is unrolled so that several are in flight).  The
// kernel is latency-bound by construction - 64 rows are 4 MB, a few microseconds of HBM time - and what it must not do
// is add a second pass: lanes reduce in registers (wave64 shuffles), waves through 64 bytes of LDS, and lane 0 stores
// the row's 16 bytes.  Plain stores, no atomics and no memset: every call overwrites, and sums of counts and a maximum of
// bit patterns do not depend on any order, so two calls give the same bits.  The per-sample rules are pcm16_tally's
// (fastsvc_report.inc), the ones fastsvc_output_check applies.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "fastsvc_hip.h"

namespace fastsvc {
int set_last_error(int code, const char* msg);      // fastsvc_plan.cpp: the text fastsvc_last_error() returns
}

namespace {

#include "fastsvc_report.inc"

constexpr int CHECK_MAX = 64;                       // rows per launch (the arguments hold their descriptors)

struct CheckArgs {
    long carry_off[CHECK_MAX];                      // first double of row b's carry entry in `carry`, -1: none
    int lo[CHECK_MAX];                              // the span [lo, hi) of row b, in samples of the row
    int hi[CHECK_MAX];
};

__device__ __forceinline__ void tally4(const float4 q, unsigned& nonfinite, unsigned& clipped, unsigned& maxbits) {
    unsigned c = 0;                                 // (pcm16_tally packs two 16-bit counts: unpacked every four samples)
    pcm16_tally(q.x, c, maxbits);
    pcm16_tally(q.y, c, maxbits);
    pcm16_tally(q.z, c, maxbits);
    pcm16_tally(q.w, c, maxbits);
    nonfinite += c & 0xffffu;
    clipped += c >> 16;
}

__global__ __launch_bounds__(256)
void stream_check_kernel(CheckArgs a, const float* __restrict__ y, const unsigned long long* __restrict__ carry,
                         fastsvc_row_report* __restrict__ report, int width, int entry_doubles) {
    __shared__ unsigned red[4][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lo = a.lo[b], hi = a.hi[b];
    const float* row = y + (long)b * width;
    // [lo, body) head, [body, tail) whole 16-byte pieces, [tail, hi) tail; a span shorter than its head has no body
    const int mis = (int)((reinterpret_cast<uintptr_t>(row + lo) >> 2) & 3);
    const int head_end = lo + ((4 - mis) & 3);
    const int body = head_end < hi ? head_end : hi;
    const int nvec = (hi - body) >> 2;
    const int tail = body + 4 * nvec;
    unsigned nonfinite = 0, clipped = 0, maxbits = 0, carry_bad = 0;
    {
        // lanes 0..2 of wave 0 own the head, lanes 0..2 of wave 1 the tail (each at most 3 samples)
        int k = -1;
        if (tid < body - lo) k = lo + tid;
        else if (tid >= 64 && tid - 64 < hi - tail) k = tail + (tid - 64);
        if (k >= 0) {
            unsigned c = 0;
            pcm16_tally(row[k], c, maxbits);
            nonfinite += c & 0xffffu;
            clipped += c >> 16;
        }
    }
    const float4* piece = reinterpret_cast<const float4*>(row + body);
    #pragma unroll 4
    for (int v = tid; v < nvec; v += 256) tally4(piece[v], nonfinite, clipped, maxbits);
    const long coff = a.carry_off[b];               // (uniform per workgroup)
    if (coff >= 0) {
        const unsigned long long* c = carry + coff;
        #pragma unroll 2
        for (int i = tid; i < entry_doubles; i += 256)
            carry_bad += ((c[i] >> 52) & 0x7ffu) == 0x7ffu ? 1u : 0u;       // (exponent all ones: inf or NaN)
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nonfinite += __shfl_down(nonfinite, o);
        clipped += __shfl_down(clipped, o);
        carry_bad += __shfl_down(carry_bad, o);
        const unsigned m = __shfl_down(maxbits, o);
        maxbits = m > maxbits ? m : maxbits;
    }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        red[0][w] = nonfinite;
        red[1][w] = clipped;
        red[2][w] = maxbits;
        red[3][w] = carry_bad;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned n = 0, c = 0, m = 0, k = 0;
        #pragma unroll
        for (int w = 0; w < 4; ++w) {
            n += red[0][w];
            c += red[1][w];
            m = red[2][w] > m ? red[2][w] : m;
            k += red[3][w];
        }
        fastsvc_row_report r;
        r.nonfinite = (int)n;
        r.clipped = (int)c;
        r.max_abs = __uint_as_float(m);
        r.reserved = (int)k;
        report[b] = r;
    }
}

int bad_row(int r, const char* what) {
    char buf[160];
    snprintf(buf, sizeof buf, "fastsvc_stream_check: row %d: %s", r, what);
    return fastsvc::set_last_error(FASTSVC_E_INVALID, buf);
}

}  // namespace

extern "C" int fastsvc_stream_check(const float* y, int32_t B, int32_t width, const int32_t* span_lo, const int32_t* span_hi,
                                    const void* carry, int64_t carry_bytes, int32_t entry_doubles, int32_t n_slots,
                                    const int32_t* slot, const int32_t* entry, fastsvc_row_report* report, void* stream_) {
    if (!y || !report || !span_lo || !span_hi || B < 1 || width < 1)
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_stream_check: null pointer or size < 1");
    if ((reinterpret_cast<uintptr_t>(y) & 3) || (reinterpret_cast<uintptr_t>(report) & 3))
        return fastsvc::set_last_error(FASTSVC_E_INVALID, "fastsvc_stream_check: y or report not 4-byte aligned");
    for (int r = 0; r < B; ++r) {
        if (span_lo[r] < 0 || span_hi[r] < 0) return bad_row(r, "negative span bound");
        if (span_lo[r] > span_hi[r]) return bad_row(r, "span_lo > span_hi");
        if (span_hi[r] > width) return bad_row(r, "span_hi > width");
        const int e = entry ? entry[r] : -1;
        if (e < -1 || e > 1) return bad_row(r, "entry outside {-1, 0, 1}");
        if (e < 0) continue;
        if (!carry || (reinterpret_cast<uintptr_t>(carry) & 7)) return bad_row(r, "a carry entry with a null or misaligned carry");
        if (!slot) return bad_row(r, "a carry entry without slots");
        if (entry_doubles < 1 || carry_bytes < 2 * (int64_t)entry_doubles * 8 || (carry_bytes & 7))
            return bad_row(r, "carry_bytes < 2 * entry_doubles * 8, or not a multiple of 8");
        if (slot[r] < 0 || slot[r] >= n_slots) return bad_row(r, "slot outside [0, n_slots)");
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int b0 = 0; b0 < B; b0 += CHECK_MAX) {
        const int nb = B - b0 < CHECK_MAX ? B - b0 : CHECK_MAX;
        CheckArgs a;
        for (int i = 0; i < CHECK_MAX; ++i) {
            const int r = b0 + i;
            const int e = (i < nb && entry) ? entry[r] : -1;
            a.lo[i] = i < nb ? span_lo[r] : 0;
            a.hi[i] = i < nb ? span_hi[r] : 0;
            a.carry_off[i] = e < 0 ? -1 : (long)slot[r] * (long)(carry_bytes / 8) + (long)e * entry_doubles;
        }
        hipLaunchKernelGGL(stream_check_kernel, dim3((unsigned)nb), dim3(256), 0, stream,
                           a, y + (long)b0 * width, static_cast<const unsigned long long*>(carry), report + b0, width,
                           entry_doubles);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK
                                           : fastsvc::set_last_error(FASTSVC_E_HIP, "fastsvc_stream_check: launch failed");
}
