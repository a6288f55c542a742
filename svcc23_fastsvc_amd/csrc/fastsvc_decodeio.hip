// fastsvc_decodeio.hip - the two ends of a resident decode session on gfx950 (decode.DecodeSession):
//
//   gather_time_major   the dump's own layout, utterance b a contiguous time-major (len_b, C) float32 block of ONE packed
//                       device buffer, into the zero-padded channel-major (B, C, width) batch the forward reads;
//   pcm16_pack          the forward's (B, width) float32 waveforms into ONE packed, unpadded int16 buffer - exactly
//                       decode.to_pcm16's values, so that 2 bytes per valid sample cross the bus instead of 4 per padded one;
//   pcm16_check         the same pass with a per-row report of what the conversion hides (non-finite and saturating
//                       samples, the largest magnitude), with or without the int16 destination.
//
// The reference decodes one utterance at a time on the host (decode_fastsvc.py:150-200: numpy transpose, sf.write's
// PCM_16 conversion) and has no counterpart.  Both kernels are pure data movement, priced like fastsvc_stage.hip:
// (bytes read + bytes written) / HBM bandwidth.
//
// Descriptors (block offsets, lengths) travel IN the kernel arguments, 64 utterances per launch, like GatherArgs in
// fastsvc_stage.hip: a session assembles a different subset of its utterances for every batch, so a device table would
// be one more small upload per batch and one more buffer to keep alive until the launch has run; 12 bytes per utterance
// fit the argument segment, and a batch of more than 64 utterances is simply several launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fastsvc_hip.h"

namespace {

constexpr int IO_MAX = 64;                          // utterances per launch (the arguments hold their descriptors)

struct TimeMajorArgs {
    long off[IO_MAX];                               // first element of utterance b's (len, C) block in `packed`
    int len[IO_MAX];                                // its time steps
};

// One block transposes a tile of 64 time steps x 64 channels through LDS.
//   global read   along C (the source's unit stride): 16 lanes x 16 bytes = one 256-byte piece of a time row when C % 4 == 0
//                 and the block starts on a 16-byte boundary, else 64 lanes x 4 bytes;
//   global write  along time (the destination's unit stride): 16 bytes per lane where the destination row allows.
// LDS image: tile[c][t] with a row pitch of TM_PITCH = 65 dwords.  Banks are (addr / 4) % 32 for ds_write_b32 and
// ds_read_b32, only lanes of the same 32-lane half conflict, and the paired forms the compiler emits here (ds_write2_b32,
// ds_read2_b32) are serviced as their two dwords one after the other.  With pitch = 65 = 1 (mod 32) the bank of (c, t) is
// (c + t) % 32:
//   element-wise fill   a half holds 32 consecutive c at one t: 32 different banks, conflict-free;
//   16-byte fill        a half holds c = 4 cl + e (cl = 0..15) at two consecutive t, one e per ds_write_b32: banks
//                       (4 cl + e + t) % 32 - cl and cl + 8 meet, the two t do not: 2-way;
//   drain               a half holds two consecutive c and t = 4 tq + e (tq = 0..15), one e per read: banks
//                       (c + 4 tq + e) % 32 - tq and tq + 8 meet, the two c do not: 2-way.
// An even pitch (64, 68) would put the 16 cl of a fill on 8 (64: on ONE) banks per t and both t on the same ones: 4-way or
// worse.  Any odd pitch gives the same 2-way picture; 65 is the smallest.
constexpr int TM_TILE = 64;
constexpr int TM_PITCH = 65;

__global__ __launch_bounds__(256)
void gather_time_major_kernel(TimeMajorArgs a, const float* __restrict__ packed, float* __restrict__ dst, int C, int width) {
    __shared__ float tile[TM_TILE * TM_PITCH];
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * TM_TILE, t0 = blockIdx.x * TM_TILE;
    const int len = a.len[b];
    const int tid = threadIdx.x;
    const bool live = t0 < len;                     // (uniform per block) a tile past the utterance's end is all padding
    if (live) {
        const float* s = packed + a.off[b];
        if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
            const int cl = tid & 15, tl = tid >> 4;
            const int c = c0 + 4 * cl;
            #pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int tt = tl + 16 * p, t = t0 + tt;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (t < len && c < C) v = *reinterpret_cast<const float4*>(s + (long)t * C + c);   // (C % 4 == 0: c + 3 < C)
                float* w = tile + (4 * cl) * TM_PITCH + tt;
                w[0] = v.x; w[TM_PITCH] = v.y; w[2 * TM_PITCH] = v.z; w[3 * TM_PITCH] = v.w;
            }
        } else {
            const int cc = tid & 63, tl = tid >> 6;
            const int c = c0 + cc;
            #pragma unroll 4
            for (int p = 0; p < 16; ++p) {
                const int tt = tl + 4 * p, t = t0 + tt;
                tile[cc * TM_PITCH + tt] = (t < len && c < C) ? s[(long)t * C + c] : 0.f;
            }
        }
        __syncthreads();
    }
    const int tq = tid & 15, cr = tid >> 4;
    const int t = t0 + 4 * tq;
    if (t >= width) return;
    #pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int cc = cr + 16 * p, c = c0 + cc;
        if (c >= C) break;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const float* r = tile + cc * TM_PITCH + 4 * tq;         // (the fill wrote zeros at t >= len)
            #pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = r[e];
        }
        float* d = dst + ((long)b * C + c) * width + t;
        if (t + 3 < width && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
            *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            #pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < width) d[e] = v[e];
        }
    }
}

struct PcmArgs {
    long off[IO_MAX];                               // first int16 element of row b in `dst`
    int len[IO_MAX];                                // its valid samples
};

typedef short short8 __attribute__((ext_vector_type(8)));

// decode.to_pcm16 for one sample: rint(double(y) * 32767.0) saturated to [-32768, 32767].  The product is exact in
// float64 (24 + 15 significant bits), rint is round-half-to-even (v_rndne_f64); +-inf saturate, NaN gives 0.
__device__ __forceinline__ short pcm16_of(float y) {
    if (y != y) return 0;
    double r = __builtin_rint((double)y * 32767.0);
    r = r < -32768.0 ? -32768.0 : (r > 32767.0 ? 32767.0 : r);
    return (short)(int)r;
}

// A lane owns the 8 samples of one 16-byte aligned piece of dst: with s = elements between the previous 16-byte boundary
// and row b's first sample, lane g owns samples [8 g - s, 8 g - s + 8) of the row, clipped to [0, len).  A whole piece is
// one 16-byte store; the clipped head and tail pieces go out sample by sample, so nothing outside the row is touched.
__global__ __launch_bounds__(256)
void pcm16_pack_kernel(PcmArgs a, const float* __restrict__ y, short* __restrict__ dst, int width) {
    const int b = blockIdx.y;
    const int len = a.len[b];
    short* d = dst + a.off[b];
    const int s = (int)((reinterpret_cast<uintptr_t>(d) >> 1) & 7);
    const long k0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8 - s;
    if (k0 >= len) return;
    const float* src = y + (long)b * width;
    if (k0 >= 0 && k0 + 8 <= len) {
        float v[8];
        if ((reinterpret_cast<uintptr_t>(src + k0) & 15) == 0) {
            const float4 lo = *reinterpret_cast<const float4*>(src + k0), hi = *reinterpret_cast<const float4*>(src + k0 + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        } else {
            #pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = src[k0 + e];
        }
        short8 o;
        #pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = pcm16_of(v[e]);
        *reinterpret_cast<short8*>(d + k0) = o;
    } else {
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long k = k0 + e;
            if (k >= 0 && k < len) d[k] = pcm16_of(src[k]);
        }
    }
}

// What pcm16_of hides, for one sample: pcm16_tally (shared with fastsvc_stream_check.hip).
#include "fastsvc_report.inc"

// pcm16_pack_kernel's geometry and ownership (PACK: the same pieces, the same stores; otherwise no destination and no
// alignment shift), plus the report: every lane tallies the samples it converts - the clipped head and tail pieces sample by
// sample, like their stores, so each valid sample is counted by exactly one lane - then the block reduces in registers
// (wave64 shuffles), through 32 bytes of LDS (one slot per wave), and its first lane issues at most one integer atomic per
// field into report[b]: sums of counts and a maximum of bit patterns do not depend on the order the blocks arrive in.
// Only whole blocks past the row leave before the barrier (a block-uniform test); a lane whose piece starts past `len` in a
// block that still holds valid samples carries zeros through the reduction.
template <bool PACK>
__global__ __launch_bounds__(256)
void pcm16_check_kernel(PcmArgs a, const float* __restrict__ y, short* __restrict__ dst,
                        fastsvc_row_report* __restrict__ report, int width) {
    __shared__ unsigned red[2][4];
    const int b = blockIdx.y;
    const int len = a.len[b];
    short* d = PACK ? dst + a.off[b] : nullptr;
    const int s = PACK ? (int)((reinterpret_cast<uintptr_t>(d) >> 1) & 7) : 0;
    if ((long)blockIdx.x * 2048 - s >= len) return;                 // (uniform: the block's first piece starts past the row)
    const long k0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8 - s;
    unsigned counts = 0, maxbits = 0;
    if (k0 < len) {
        const float* src = y + (long)b * width;
        if (k0 >= 0 && k0 + 8 <= len) {
            float v[8];
            if ((reinterpret_cast<uintptr_t>(src + k0) & 15) == 0) {
                const float4 lo = *reinterpret_cast<const float4*>(src + k0), hi = *reinterpret_cast<const float4*>(src + k0 + 4);
                v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
            } else {
                #pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = src[k0 + e];
            }
            #pragma unroll
            for (int e = 0; e < 8; ++e) pcm16_tally(v[e], counts, maxbits);
            if (PACK) {
                short8 o;
                #pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = pcm16_of(v[e]);
                *reinterpret_cast<short8*>(d + k0) = o;
            }
        } else {
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                const long k = k0 + e;
                if (k >= 0 && k < len) {
                    const float v = src[k];
                    pcm16_tally(v, counts, maxbits);
                    if (PACK) d[k] = pcm16_of(v);
                }
            }
        }
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        counts += __shfl_down(counts, o);
        const unsigned m = __shfl_down(maxbits, o);
        maxbits = m > maxbits ? m : maxbits;
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = counts;
        red[1][threadIdx.x >> 6] = maxbits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0, m = 0;
        #pragma unroll
        for (int w = 0; w < 4; ++w) {
            c += red[0][w];
            m = red[1][w] > m ? red[1][w] : m;
        }
        fastsvc_row_report* r = report + b;
        if (c & 0xffffu) atomicAdd(&r->nonfinite, (int)(c & 0xffffu));
        if (c >> 16) atomicAdd(&r->clipped, (int)(c >> 16));
        if (m) atomicMax(reinterpret_cast<unsigned*>(&r->max_abs), m);
    }
}

// Host side of both checked entry points: the arguments of fastsvc_pcm16_pack checked the same way (nothing is enqueued
// when one is bad), the report cleared by one memset on the stream, then one launch per 64 rows with its reports at
// report + b0.
template <bool PACK>
int pcm16_check_launch(const float* y, const int32_t* lens, const int64_t* offsets, int16_t* dst, int64_t dst_elems,
                       fastsvc_row_report* report, int32_t B, int32_t width, void* stream_) {
    if (!y || !lens || !report || B < 1 || width < 1) return FASTSVC_E_INVALID;
    if (PACK && (!offsets || !dst || dst_elems < 0 || (reinterpret_cast<uintptr_t>(dst) & 1))) return FASTSVC_E_INVALID;
    int maxlen = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0 || lens[b] > width) return FASTSVC_E_INVALID;
        if (PACK && (offsets[b] < 0 || offsets[b] + (int64_t)lens[b] > dst_elems)) return FASTSVC_E_INVALID;
        maxlen = lens[b] > maxlen ? lens[b] : maxlen;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (hipMemsetAsync(report, 0, sizeof(fastsvc_row_report) * (size_t)B, stream) != hipSuccess) return FASTSVC_E_HIP;
    if (maxlen == 0) return FASTSVC_OK;
    const unsigned gx = (unsigned)(((long)maxlen + 7 + 2047) / 2048);      // (up to 7 samples of alignment shift per row)
    for (int b0 = 0; b0 < B; b0 += IO_MAX) {
        const int nb = B - b0 < IO_MAX ? B - b0 : IO_MAX;
        PcmArgs a;
        for (int i = 0; i < IO_MAX; ++i) {
            a.off[i] = (PACK && i < nb) ? (long)offsets[b0 + i] : 0;
            a.len[i] = i < nb ? lens[b0 + i] : 0;
        }
        hipLaunchKernelGGL(pcm16_check_kernel<PACK>, dim3(gx, (unsigned)nb), dim3(256), 0, stream,
                           a, y + (long)b0 * width, reinterpret_cast<short*>(dst), report + b0, width);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : FASTSVC_E_HIP;
}

}  // namespace

extern "C" {

int fastsvc_gather_time_major(const float* packed, int64_t packed_elems, const int64_t* offsets, const int32_t* lens,
                              float* dst, int32_t B, int32_t C, int32_t width, void* stream_) {
    if (!packed || !offsets || !lens || !dst || packed_elems < 0 || B < 1 || C < 1 || width < 1 || C > 65535)
        return FASTSVC_E_INVALID;
    for (int b = 0; b < B; ++b)
        if (lens[b] < 0 || lens[b] > width || offsets[b] < 0 || offsets[b] + (int64_t)lens[b] * C > packed_elems)
            return FASTSVC_E_INVALID;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 tiles((unsigned)((width + TM_TILE - 1) / TM_TILE), (unsigned)((C + TM_TILE - 1) / TM_TILE));
    for (int b0 = 0; b0 < B; b0 += IO_MAX) {
        const int nb = B - b0 < IO_MAX ? B - b0 : IO_MAX;
        TimeMajorArgs a;
        for (int i = 0; i < IO_MAX; ++i) {
            a.off[i] = i < nb ? (long)offsets[b0 + i] : 0;
            a.len[i] = i < nb ? lens[b0 + i] : 0;
        }
        hipLaunchKernelGGL(gather_time_major_kernel, dim3(tiles.x, tiles.y, (unsigned)nb), dim3(256), 0, stream,
                           a, packed, dst + (long)b0 * C * width, C, width);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : FASTSVC_E_HIP;
}

int fastsvc_pcm16_pack(const float* y, const int32_t* lens, const int64_t* offsets, int16_t* dst, int64_t dst_elems,
                       int32_t B, int32_t width, void* stream_) {
    if (!y || !lens || !offsets || !dst || dst_elems < 0 || B < 1 || width < 1 || (reinterpret_cast<uintptr_t>(dst) & 1))
        return FASTSVC_E_INVALID;
    int maxlen = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 0 || lens[b] > width || offsets[b] < 0 || offsets[b] + (int64_t)lens[b] > dst_elems)
            return FASTSVC_E_INVALID;
        maxlen = lens[b] > maxlen ? lens[b] : maxlen;
    }
    if (maxlen == 0) return FASTSVC_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned gx = (unsigned)(((long)maxlen + 7 + 2047) / 2048);      // (up to 7 samples of alignment shift per row)
    for (int b0 = 0; b0 < B; b0 += IO_MAX) {
        const int nb = B - b0 < IO_MAX ? B - b0 : IO_MAX;
        PcmArgs a;
        for (int i = 0; i < IO_MAX; ++i) {
            a.off[i] = i < nb ? (long)offsets[b0 + i] : 0;
            a.len[i] = i < nb ? lens[b0 + i] : 0;
        }
        hipLaunchKernelGGL(pcm16_pack_kernel, dim3(gx, (unsigned)nb), dim3(256), 0, stream,
                           a, y + (long)b0 * width, reinterpret_cast<short*>(dst), width);
    }
    return hipGetLastError() == hipSuccess ? FASTSVC_OK : FASTSVC_E_HIP;
}

int fastsvc_output_check(const float* y, const int32_t* lens, fastsvc_row_report* report, int32_t B, int32_t width,
                         void* stream) {
    return pcm16_check_launch<false>(y, lens, nullptr, nullptr, 0, report, B, width, stream);
}

int fastsvc_pcm16_pack_checked(const float* y, const int32_t* lens, const int64_t* offsets, int16_t* dst, int64_t dst_elems,
                               fastsvc_row_report* report, int32_t B, int32_t width, void* stream) {
    return pcm16_check_launch<true>(y, lens, offsets, dst, dst_elems, report, B, width, stream);
}

}  // extern "C"
