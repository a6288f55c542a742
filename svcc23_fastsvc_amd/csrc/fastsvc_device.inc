// fastsvc_device.inc - device helpers shared by the convolution kernel files (fastsvc_kernels.hip: f32-input
// MFMA kernels; fastsvc_hx.hip: f16 split-product / bf16 MFMA kernels).  Included INSIDE namespace fastsvc
// (and fastsvc::bf16 / fastsvc::f16 for the 2-byte-storage compilations): buffer-descriptor loads / stores, the activation
// storage type, and the tile epilogues (bias, LeakyReLU, residual, FiLM affine + InstanceNorm partial sums).

typedef float f32x4 __attribute__((ext_vector_type(4)));

// compile-time epilogue kinds of the pipelined kernel (see ws_epilogue_kind)
enum : int { EPI_GENERIC = 0, EPI_PLAIN = 1, EPI_RES = 2, EPI_RANK1 = 3, EPI_AFF = 4 };

__device__ __forceinline__ float lrelu(float v) { return v >= 0.f ? v : LRELU_SLOPE * v; }

__device__ __forceinline__ int div_small(int t, int s) {
    // nearest-stretch source index; s in {2,4,5} for the yaml config - keep those divisions cheap
    switch (s) {
        case 2: return t >> 1;
        case 4: return t >> 2;
        case 5: return t / 5;
        case 1: return t;
        default: return t / s;
    }
}


template <int NT, int NTHREADS>
struct StageGeom {
    static constexpr int MAXW4 = (NT + 56) / 4;                       // halo <= 28 columns per side
    static constexpr int ITEMS = (24 * MAXW4 + NTHREADS - 1) / NTHREADS;
};


__device__ __forceinline__ unsigned udiv_small(unsigned t, int s) {
    switch (s) {
        case 1: return t;
        case 2: return t >> 1;
        case 4: return t >> 2;
        case 5: return __umulhi(t, 0xCCCCCCCDu) >> 2;
        default: return t / (unsigned)s;
    }
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Cache policy of the ACTIVATION tensors' loads / stores (the `aux` operand of the raw buffer instructions; gfx950: 1 = sc0,
// 2 = nt, 16 = sc1).  Most workspace tensors are written once and read once, and at 64 x 10 s they are several times the
// 256 MB Infinity Cache: A/B builds (FASTSVC_BUILD_FLAGS="-DFASTSVC_ST_AUX=2 ...", profiles/r6_cache_policy_ab.txt) decide.
// Weights, biases, scale / shift (read three times per block) and the statistics keep the default policy.
#ifndef FASTSVC_LD_AUX
#define FASTSVC_LD_AUX 0
#endif
#ifndef FASTSVC_ST_AUX
#define FASTSVC_ST_AUX 0
#endif

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* base, long nfloats) {
    // raw buffer over [base, base + nfloats): out-of-range loads return 0, stores are dropped
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)(nfloats * 4), 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void buf_store4(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, 0, FASTSVC_ST_AUX);
}
// Rows need not be a multiple of 4 long (T_k = 2F, F for odd frame counts): every float4 access is
// only dword-aligned then, and the float4 that straddles the end of a row is handled by element:
// nv = number of its elements that belong to the row (4 everywhere else, 0 for lanes off the tile).
__device__ __forceinline__ void buf_store4_n(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v, int nv) {
    // wave-uniform fast path: no lane of the wave is a partial float4 (rows that are a multiple of 4 long,
    // i.e. nearly always) -> ONE store instead of four; vmcnt counts every one of them, and the weight
    // ring's counted waits drain whatever stores are ahead of them
    if (__builtin_amdgcn_ballot_w64(nv > 0 && nv < 4) == 0) {
        buf_store4(r, nv > 0 ? voff : 0x7ffffff0, v);
    } else if (nv >= 4) {
        buf_store4(r, voff, v);
    } else {
        // element stores with the offset pushed out of range for the elements past the row end
        // (dropped by the descriptor); no per-element branches
        const float e0 = v[0], e1 = v[1], e2 = v[2];
        const int far = 0x7ffffff0;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, e0), r, nv >= 1 ? voff : far, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, e1), r, nv >= 2 ? voff + 4 : far, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, e2), r, nv >= 3 ? voff + 8 : far, 0, 0);
    }
}
__device__ __forceinline__ f32x4 keep_first(f32x4 v, int nv) {      // zero the elements past the row end
    if (nv < 4) v.w = 0.f;
    if (nv < 3) v.z = 0.f;
    if (nv < 2) v.y = 0.f;
    if (nv < 1) v.x = 0.f;
    return v;
}
__device__ __forceinline__ int row_valid(int t, int T) { return min(4, max(0, T - t)); }
// The variants that sit at the 128-VGPR limit are compiled WITHOUT the row-end handling (they are the
// full-rate shapes, whose rows are 160 F long); run_conv only launches them when T % 4 == 0.
// ---- activation storage type ------------------------------------------------------------------
// The file is compiled three times: as is (activations float32 in HBM: the parity path) and with
// -DFASTSVC_ACT_BF16 / -DFASTSVC_ACT_F16 (namespace fastsvc::bf16 / fastsvc::f16; both set FASTSVC_ACT_2B, see
// fastsvc_kernels.h: every workspace tensor - conv outputs, FiLM-affined tensors, scale / shift - is stored as
// bfloat16 / binary16, halving the traffic of the HBM-bound layers; the arithmetic, the LDS windows, the weights
// and the InstanceNorm sums stay float32 / float64).
// All offsets in the kernels are written in "float bytes" (elements * 4); the 2-byte helpers halve them.
// Sum over the wave's four 16-lane rows, every lane ending with a[l & 15] + a[(l & 15) + 16] + ... (the order of
// `a += __shfl_xor(a, 16); a += __shfl_xor(a, 32)`, bit for bit) on the VALU: gfx950's v_permlane{16,32}_swap instead of two
// ds_bpermute_b32 round trips through the LDS queue per value (the per-tile InstanceNorm sums of the narrow layers: 0.7k of
// 6.4k cycles per tile at up.3.d9 between the last store and the tile's end).  Inline assembly: this hipcc's
// __builtin_amdgcn_permlane*_swap reads its first result twice (v_add v1, v1, v1).  s_nop 1: the two wait states between
// a VALU write and the swap that reads it.
__device__ __forceinline__ float row_xsum(float a) {
    float b = a;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    a += b;
    b = a;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}
double row_xsum(double) = delete;                        // (float64 sums: __shfl_xor - a silent narrowing would cost the sums their precision)
#ifdef FASTSVC_ACT_2B
typedef unsigned short act_t;
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
// ---- the element format: the ONLY code that knows whether the 2-byte element is bfloat16 or binary16 ----
//   a16_lo / a16_hi : the low / high half of a dword as float       a16_bits : float -> the element's bits, round to nearest even
//   a16_pack2       : two floats -> one dword (low half first), round to nearest even
// Each is one VALU instruction per value in both formats (gfx950): shift / mask against v_cvt_f32_f16 (+ sdwa WORD_1),
// v_cvt_pk_bf16_f32 against v_cvt_pk_f16_f32 (NOT v_cvt_pkrtz: values pass through a dozen layers, a biased rounding adds up).
#ifdef FASTSVC_ACT_F16
__device__ __forceinline__ float a16_lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)w); }
__device__ __forceinline__ float a16_hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
__device__ __forceinline__ unsigned a16_bits(float x) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)x); }
__device__ __forceinline__ unsigned a16_pack2(float a, float b) {
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    typedef float f2v __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{a, b}, h2v));
}
#else
__device__ __forceinline__ float a16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float a16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
__device__ __forceinline__ unsigned a16_bits(float x) {                    // round to nearest even
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// ONE v_cvt_pk_bf16_f32 (gfx950) where the integer form above costs 3-4 instructions per value - the epilogues of the
// narrow layers are bound by their VALU instruction count (timeline of up.3.d9: 4.1k of 5.8k cycles per tile in the
// epilogue with four waves per SIMD)
__device__ __forceinline__ unsigned a16_pack2(float a, float b) {
    typedef __bf16 bf2v __attribute__((ext_vector_type(2)));
    typedef float f2v __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f2v{a, b}, bf2v));
}
#endif
__device__ __forceinline__ f32x4 a16_unpack4(unsigned lo, unsigned hi) { return f32x4{a16_lo(lo), a16_hi(lo), a16_lo(hi), a16_hi(hi)}; }
__device__ __forceinline__ f32x4 act_load4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    const u32x2v w = __builtin_amdgcn_raw_buffer_load_b64(r, voff >> 1, soff >> 1, FASTSVC_LD_AUX);
    return a16_unpack4(w.x, w.y);
}
__device__ __forceinline__ float act_load1(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    const unsigned short h = __builtin_amdgcn_raw_buffer_load_b16(r, voff >> 1, soff >> 1, 0);
    return a16_lo((unsigned)h);
}
// The same loads WITHOUT the conversion: what a prefetching wave keeps in registers between the request and the use.
// (A converted value is an instruction on the loaded register, i.e. a wait for the load where the conversion stands -
// the staging waves' window loads were waited for in the unit that issued them: the two-deep prefetch ran at depth 0.)
typedef u32x2v act4_t;                                                     // four elements
typedef unsigned act1_t;                                                   // one element (low half)
__device__ __forceinline__ act4_t act_load4_raw(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_amdgcn_raw_buffer_load_b64(r, voff >> 1, soff >> 1, FASTSVC_LD_AUX);
}
__device__ __forceinline__ f32x4 act_unpack4(act4_t w) {
    return a16_unpack4(w.x, w.y);
}
__device__ __forceinline__ act4_t act_pack4_raw(act1_t a, act1_t b, act1_t c, act1_t d) {
    return act4_t{(a & 0xffffu) | (b << 16), (c & 0xffffu) | (d << 16)};
}
__device__ __forceinline__ act1_t act_load1_raw(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return (unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, voff >> 1, soff >> 1, 0);
}
__device__ __forceinline__ float act_unpack1(act1_t h) { return a16_lo(h); }
__device__ __forceinline__ void act_store4(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v) {
    u32x2v w;
    w.x = a16_pack2(v.x, v.y);
    w.y = a16_pack2(v.z, v.w);
    __builtin_amdgcn_raw_buffer_store_b64(w, r, voff >> 1, 0, FASTSVC_ST_AUX);
}
__device__ __forceinline__ void act_store4_n(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v, int nv) {
    if (nv >= 4) {
        act_store4(r, voff, v);
    } else {
        const float e0 = v[0], e1 = v[1], e2 = v[2];
        const int far = 0x7ffffff0, o = voff >> 1;
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)a16_bits(e0), r, nv >= 1 ? o : far, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)a16_bits(e1), r, nv >= 2 ? o + 2 : far, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)a16_bits(e2), r, nv >= 3 ? o + 4 : far, 0, 0);
    }
}
#else
typedef float act_t;
__device__ __forceinline__ f32x4 act_load4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, FASTSVC_LD_AUX));
}
__device__ __forceinline__ float act_load1(__amdgpu_buffer_rsrc_t r, int voff, int soff) { return buf_load1(r, voff, soff); }
typedef f32x4 act4_t;
typedef float act1_t;
__device__ __forceinline__ act4_t act_load4_raw(__amdgpu_buffer_rsrc_t r, int voff, int soff) { return act_load4(r, voff, soff); }
__device__ __forceinline__ f32x4 act_unpack4(act4_t w) { return w; }
__device__ __forceinline__ act4_t act_pack4_raw(act1_t a, act1_t b, act1_t c, act1_t d) { return f32x4{a, b, c, d}; }
__device__ __forceinline__ act1_t act_load1_raw(__amdgpu_buffer_rsrc_t r, int voff, int soff) { return buf_load1(r, voff, soff); }
__device__ __forceinline__ float act_unpack1(act1_t h) { return h; }
__device__ __forceinline__ void act_store4(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v) { buf_store4(r, voff, v); }
__device__ __forceinline__ void act_store4_n(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v, int nv) { buf_store4_n(r, voff, v, nv); }
#endif
// descriptor over `nelems` activation elements starting `elem_off` elements after `base`
__device__ __forceinline__ __amdgpu_buffer_rsrc_t act_rsrc(const float* base, long elem_off, long nelems) {
    const act_t* q = reinterpret_cast<const act_t*>(base) + elem_off;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<act_t*>(q), 0, (int)(nelems * (long)sizeof(act_t)), 0x00020000);
}

template <bool TAIL>
__device__ __forceinline__ void store_row4(__amdgpu_buffer_rsrc_t r, int voff, f32x4 v, int nv) {
    if constexpr (TAIL) act_store4_n(r, voff, v, nv); else act_store4(r, voff, v);
}
template <bool TAIL>
__device__ __forceinline__ f32x4 keep_row(f32x4 v, int nv) {
    if constexpr (TAIL) return keep_first(v, nv); else return v;
}
template <int MW, int NW, int MODE, int EPI, int S>
constexpr bool ws_tail_ok() {
    if (MODE == MODE_POLY) return !(MW == 2 && S >= 4 && EPI == EPI_AFF);
    return !(MW == 2 && NW == 4);
}

// Tile epilogue of the wave-specialised kernel (T % 4 == 0).  Every tensor is addressed through a
// buffer descriptor (wave-uniform base in SGPRs) plus ONE 32-bit byte offset per (channel, time)
// position shared by y / y2 / residual / scale / shift: no 64-bit pointer arithmetic, few VGPRs.
struct EpiRsrc {
    __amdgpu_buffer_rsrc_t y, y2, res, ss, r1x;
    // running max |value| of the tensor y this launch hands to a later convolution (ConvParams::amax_out; residual
    // epilogues only, see ws_epilogue_kind).  Lanes off the tile contribute values computed from zero padding
    // (bias-sized, finite): harmless for a bound.  float32 storage only.
    mutable float amx = 0.f;
    // the wave's running max over the tiles it has finished: wave-uniform (an SGPR), so that `amx` is live only
    // inside a tile's epilogue - several variants sit exactly at their VGPR budget
    mutable unsigned wmax = 0u;
};
// An amax entry (one per tensor and utterance) is AMAX_W slots, each in its own 128-byte line: device-scope atomics
// on one line serialise at ~13 ns apiece (measured: +12 us on a 250-workgroup launch with one atomic per wave), so
// writers spread over the slots and readers take the max of the eight.
constexpr int AMAX_W = 8;
constexpr int AMAX_STRIDE = 32;          // floats between slots
constexpr int AMAX_ENTRY = AMAX_W * AMAX_STRIDE;
#if defined(FASTSVC_ACT_2B) || defined(FASTSVC_EXP_NOTRACK)
constexpr bool AMAX_TRACK = false;       // 2-byte storage: bf16 has float32's exponent range; binary16 storage is unscaled (range contract, fastsvc_hip.h)
#else
constexpr bool AMAX_TRACK = true;
#endif
__device__ __forceinline__ void amax_track(const EpiRsrc& R, const f32x4& v) {
    if constexpr (AMAX_TRACK)
        R.amx = fmaxf(fmaxf(R.amx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
// max over the wave with DPP moves (no LDS round trips: ds_bpermute shuffles cost the consumer wave ~100 cycles
// each, six in a row per tile were 5-15 % of the narrow layers); the result is valid in lane 63.  Non-negative
// floats order like their bit patterns, so the max runs on the integer pipe.
__device__ __forceinline__ unsigned wave_max_u32_lane63(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x111, 0xf, 0xf, false));    // row_shr:1
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x112, 0xf, 0xf, false));    // row_shr:2
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x114, 0xf, 0xf, false));    // row_shr:4
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x118, 0xf, 0xf, false));    // row_shr:8 -> lane 15 of each row
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xa, 0xf, false));    // row_bcast:15 -> rows 1, 3
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xc, 0xf, false));    // row_bcast:31 -> rows 2, 3
    return v;
}
// end of a TILE's epilogue (pipelined kernels): fold the lanes' running max into the wave's uniform one
__device__ __forceinline__ void amax_tile_flush(const EpiRsrc& R) {
    if constexpr (AMAX_TRACK) {
        const unsigned a = wave_max_u32_lane63(__builtin_bit_cast(unsigned, R.amx));
        R.wmax = max(R.wmax, (unsigned)__builtin_amdgcn_readlane((int)a, 63));
        R.amx = 0.f;
    }
}
// after a wave's last tile: the waves of a workgroup combine in LDS (s_amax; s_cnt counts arrivals - LDS operations
// of a CU execute in order, so the wave that sees the last arrival also sees every other wave's max) and that last
// wave issues ONE device-scope atomic max for the workgroup, in a slot picked by `spread`.  No barrier: the other
// waves are done.  nwaves = waves that call this (active or not).
__device__ __forceinline__ void amax_flush(const ConvParams& p, const EpiRsrc& R, unsigned* s_amax, unsigned* s_cnt, int nwaves,
                                           int sig, int b, int lane, int spread) {
    if constexpr (AMAX_TRACK) {
        if (!p.amax_out) return;
        const unsigned a = max(R.wmax, (unsigned)__builtin_amdgcn_readlane((int)wave_max_u32_lane63(__builtin_bit_cast(unsigned, R.amx)), 63));
        if (lane == 0) {
            atomicMax(s_amax, a);
            if (atomicAdd(s_cnt, 1u) == (unsigned)(nwaves - 1))
                atomicMax(reinterpret_cast<unsigned*>(p.amax_out) + (sig * p.amax_out_sig + b) * AMAX_ENTRY +
                              (spread & (AMAX_W - 1)) * AMAX_STRIDE, atomicMax(s_amax, 0u));
        }
    }
}
// largest magnitude recorded for (tensor, utterance): the max over the entry's slots (uniform address: scalar loads)
__device__ __forceinline__ float amax_read(const float* rows, int idx) {
    float m = 0.f;
    #pragma unroll
    for (int k = 0; k < AMAX_W; ++k) m = fmaxf(m, rows[idx * AMAX_ENTRY + k * AMAX_STRIDE]);
    return m;
}
// Power-of-two factor that moves a tensor bounded by `bound` into binary16's range with headroom: bound * s in
// [2^14, 2^15) (values down to 2^-17 of the bound keep all 22 bits of the hi + lo split).  0 / denormal bounds: 1;
// the exponent is clamped to +-80 so that every product of two such factors is a normal float32.
__device__ __forceinline__ float hx_scale_for(float bound) {
    const int e = (int)((__builtin_bit_cast(unsigned, bound) >> 23) & 0xffu);      // bound in [2^(e-127), 2^(e-126))
    if (e == 0) return 1.0f;
    const int se = min(127 + 80, max(127 - 80, 127 + 15 - (e - 126)));
    return __builtin_bit_cast(float, (unsigned)se << 23);
}
// Per-lane epilogue constants of the wave's MW channel tiles, loaded ONCE per workgroup: fetched inside
// the epilogue each costs an L2 round trip and a vmcnt(0) that also drains the previous item's stores.
// HOISTED false (variants already at their register budget): fetched per item as before.
// SCALED (split-binary16 kernels, float32 storage): the accumulators hold conv * (activation scale * weight scale
// of the channel); the exact power-of-two inverse is applied by the SAME instruction that adds the bias (one FMA
// instead of one add).
template <int MW, bool HOISTED, bool SCALED_ = false>
struct EpiConst {
    static constexpr bool SCALED = SCALED_;
    const float (&k_bias)[MW];
    const float (&k_bias2)[MW];
    const float (&k_r1w)[MW];
    const float (&k_r1b)[MW];
    // SCALED: this lane's inverse factors in LDS (read where they are used: no registers held across the tile loop) -
    // sinv[16 m] for channel tile m, sinv[inv2_off + 16 m] for the second output of MODE_DEC2
    const float* sinv;
    int inv2_off;
    // (read ONCE per channel tile and epilogue: callers keep the value for the tile's items)
    __device__ __forceinline__ float inv(int m) const { if constexpr (SCALED) return sinv[16 * m]; else return 1.f; }
    __device__ __forceinline__ float inv2(int m) const { if constexpr (SCALED) return sinv[inv2_off + 16 * m]; else return 1.f; }
    static __device__ __forceinline__ f32x4 finish(const f32x4& a, float iv, float bias) {
        if constexpr (SCALED) return a * iv + bias; else return a + bias;
    }
    static __device__ __forceinline__ f32x4 unscale(const f32x4& a, float iv) {
        if constexpr (SCALED) return a * iv; else return a;
    }
    // cot: channel of this lane in tile m (bias arrays are padded to the tiles), co: the same clamped to COUT
    __device__ __forceinline__ float bias(const ConvParams& p, int sig, int m, int cot) const {
        if constexpr (HOISTED) return k_bias[m]; else return p.bias[(long)sig * p.bias_sig + cot];
    }
    __device__ __forceinline__ float bias2(const ConvParams& p, int sig, int m, int cot) const {
        if constexpr (HOISTED) return k_bias2[m]; else return p.bias2[(long)sig * p.bias2_sig + cot];
    }
    __device__ __forceinline__ float r1w(const ConvParams& p, int sig, int m, int co) const {
        if constexpr (HOISTED) return k_r1w[m]; else return p.r1w[(long)sig * p.r1_sig + co];
    }
    __device__ __forceinline__ float r1b(const ConvParams& p, int sig, int m, int co) const {
        if constexpr (HOISTED) return k_r1b[m]; else return p.r1b[(long)sig * p.r1_sig + co];
    }
};

template <int MW, int NW>
__device__ __forceinline__ void ws_epilogue_tile(const ConvParams& p, const EpiRsrc& R, f32x4 (&acc)[NW][MW],
                                                 float (&s1)[MW], float (&s2)[MW],
                                                 int sig, int mg, int tcol0, bool active, int lane) {
    const int flags = p.flags;
    if (FASTSVC_DBG_ON(p, DBG_NO_EPILOGUE)) {
        float keep = 0.f;
        #pragma unroll
        for (int n = 0; n < NW; ++n)
            #pragma unroll
            for (int m = 0; m < MW; ++m) keep += acc[n][m].x + acc[n][m].y + acc[n][m].z + acc[n][m].w;
        if (keep == 1.2345678e33f) (p.y ? p.y : p.y2)[0] = keep;
        return;
    }
    if (!active) return;
    const float* biasp = p.bias + (long)sig * p.bias_sig;
    const int shift_soff = p.COUT * p.ldy * 4;            // shift rows follow the scale rows
    #pragma unroll
    for (int m = 0; m < MW; ++m) {
        const int co = (mg * MW + m) * 16 + (lane & 15);
        if (co >= p.COUT) continue;
        const float bias = biasp[co];
        float r1w = 0.f, r1b = 0.f;
        if (p.r1x) { r1w = p.r1w[(long)sig * p.r1_sig + co]; r1b = p.r1b[(long)sig * p.r1_sig + co]; }
        const int rowoff = co * p.ldy;
        #pragma unroll
        for (int n = 0; n < NW; ++n) {
            const int t = tcol0 + n * 16 + (lane >> 4) * 4;
            if (t >= p.T) continue;
            constexpr bool TAIL = ws_tail_ok<MW, NW, MODE_DIRECT, EPI_GENERIC, 1>();
            const int nv = TAIL ? row_valid(t, p.T) : 4;
            const int off = (rowoff + t) * 4;
            f32x4 v = acc[n][m];
            v += bias;
            if (flags & F_POST_LRELU) {
                v.x = lrelu(v.x); v.y = lrelu(v.y); v.z = lrelu(v.z); v.w = lrelu(v.w);
            }
            if (p.res) v += act_load4(R.res, off, 0);
            if (p.r1x) v += buf_load4(R.r1x, t * 4, 0) * r1w + r1b;
            if (p.y) store_row4<TAIL>(R.y, off, v, nv);
            if (flags & (F_STATS | F_AFF_OUT)) {
                const f32x4 u = keep_row<TAIL>(act_load4(R.ss, off, 0) * v + act_load4(R.ss, off, shift_soff), nv);
                if (flags & F_AFF_OUT) store_row4<TAIL>(R.y2, off, u, nv);
                s1[m] += (u.x + u.y) + (u.z + u.w);
                s2[m] += (u.x * u.x + u.y * u.y) + (u.z * u.z + u.w * u.w);
            } else amax_track(R, keep_row<TAIL>(v, nv));
        }
    }
}

// Compile-time specialised epilogues for the NARROW (HBM-bound) layers.  The generic epilogue
// above keeps every optional tensor behind a uniform branch, which makes hipcc wait vmcnt(0)
// after each load: ~3 serialised memory latencies per item, 8 items per tile.  Here the kind is a
// template parameter, the code is straight-line, out-of-range lanes use an offset beyond every
// descriptor (loads return 0, stores are dropped) and the loads of G items are issued together.
constexpr int OOB_OFF = 0x7ffffff0;

// Epilogue operands staged in LDS by the consumer wave itself (see ws_estage): fetched inside the epilogue
// they cost MW*NW serialised memory round trips after the MFMA loop (timeline of a C = 24 unit: 16.8k of
// 23.6k cycles), and the 128-register budget has no room to prefetch them into VGPRs.  One LDS-DMA (`buffer_load_dwordx4 ... lds`, no VGPRs) per operand and
// 16x16 item, issued before the MFMA loop of the tile's last K chunk.  A piece lands lane-linear
// (wave base + lane * 16), so in the epilogue every lane reads back exactly the float4 it requested:
// a private, conflict-free extension of the register file; no cross-wave synchronisation.
// Wave region: [operand: scale, shift, residual][m][n][64 lanes] float4.
// The DMA is inline assembly on purpose: behind the builtin hipcc drains vmcnt(0) before every LDS read
// that follows (and again after each item's stores); hidden from it, its own counted waits on the
// weight ring stay valid (loads return in order, the extra pieces only make them conservative) and
// the epilogue waits with ws_epilogue_stage_wait.  M0 (LDS base of the piece) has no other user here.
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t r, unsigned lds_byte, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :: "s"(lds_byte), "v"(voff), "s"(r), "s"(soff) : "memory");
}
__device__ __forceinline__ void lds_dma4(__amdgpu_buffer_rsrc_t r, unsigned lds_byte, int voff, int soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
                 :: "s"(lds_byte), "v"(voff), "s"(r), "s"(soff) : "memory");
}
// One 16 x 16 item of an activation tensor (this lane's four consecutive elements) into the wave's slot.
// float32: one 16-byte piece per lane (1 KB slot).  bfloat16 storage: the lane's 8 bytes go as two
// dword pieces (LDS-DMA has no 8-byte form): elements 0-1 in the first 256 B of the slot, 2-3 in the second.
#ifdef FASTSVC_ACT_2B
constexpr int EST_ITEM_FLOATS = 128;
constexpr int EST_DMA_PER_ITEM = 2;                         // LDS-DMA instructions of one item (what a counted wait skips)
__device__ __forceinline__ void est_fetch(__amdgpu_buffer_rsrc_t r, unsigned slot_byte, int off, int soff) {
    lds_dma4(r, slot_byte, off >> 1, soff >> 1);
    lds_dma4(r, slot_byte + 256, (off >> 1) + 4, soff >> 1);
}
__device__ __forceinline__ f32x4 est_read(const float* slot, int lane) {
    const unsigned w0 = __builtin_bit_cast(unsigned, slot[lane]), w1 = __builtin_bit_cast(unsigned, slot[64 + lane]);
    return a16_unpack4(w0, w1);
}
#else
constexpr int EST_ITEM_FLOATS = 256;
constexpr int EST_DMA_PER_ITEM = 1;
__device__ __forceinline__ void est_fetch(__amdgpu_buffer_rsrc_t r, unsigned slot_byte, int off, int soff) {
    lds_dma16(r, slot_byte, off, soff);
}
__device__ __forceinline__ f32x4 est_read(const float* slot, int lane) {
    return reinterpret_cast<const f32x4*>(slot)[lane];
}
#endif
// all pieces landed: they are older than the NEWER weight-ring loads of at least one unit
template <int NEWER>
__device__ __forceinline__ void ws_epilogue_stage_wait(bool counted) {
    if (counted) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NEWER) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int MW, int NW, int EPI>
__device__ __forceinline__ void ws_epilogue_stage(const ConvParams& p, const EpiRsrc& R, const float* Ew,
                                                  int mg, int tcol0, int lane) {
    const int shift_soff = p.COUT * p.ldy * 4;
    const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const float*)Ew;
    #pragma unroll
    for (int m = 0; m < MW; ++m) {
        const int cot = (mg * MW + m) * 16 + (lane & 15);
        const bool cok = cot < p.COUT;
        const int rowoff = (cok ? cot : 0) * p.ldy;
        #pragma unroll
        for (int n = 0; n < NW; ++n) {
            const int t = tcol0 + n * 16 + (lane >> 4) * 4;
            const int off = (cok && t < p.T) ? (rowoff + t) * 4 : OOB_OFF;
            constexpr int IB = EST_ITEM_FLOATS * 4;            // bytes of one item slot
            const unsigned slot = base + (m * NW + n) * IB;
            if (EPI == EPI_RES) est_fetch(R.res, slot, off, 0);
            if (EPI == EPI_AFF) {
                est_fetch(R.ss, slot, off, 0);
                est_fetch(R.ss, slot + MW * NW * IB, off, shift_soff);
                if (p.res) est_fetch(R.res, slot + 2 * MW * NW * IB, off, 0);
            }
        }
    }
}

// TAILMODE: -1 = row-end handling as ws_tail_ok says for the f32-MFMA variants, 0 = off (callers that only run
// on rows that are a multiple of 4 long), 1 = on, 2 = "soft": the row PITCH is a multiple of 4 but this utterance's
// own length (ragged batch) need not be - the float4 that straddles the row end is stored whole (what lies between
// the row end and the pitch is nobody's data: every reader masks by its own length) and only what is SUMMED or
// measured (InstanceNorm statistics, running max) is masked, behind a wave-uniform test of the length
// TRACK: keep the running max |value| of what is written (ConvParams::amax_out).  Only the tensors a later launch
// scales its staging by are measured - a conditioning stage's output and a block's output, both written by residual
// epilogues (and by the fused pair's final epilogue, which passes TRACK = 1) - so the FiLM-affine, plain, polyphase
// and decimating epilogues, which are bound by their store phase, carry none of it.  -1: by kind.
template <int MW, int NW, int EPI, bool EST = false, int TAILMODE = -1, int TRACK = -1, class KT>
__device__ __forceinline__ void ws_epilogue_kind(const ConvParams& p, const EpiRsrc& R, f32x4 (&acc)[NW][MW],
                                                 float (&s1)[MW], float (&s2)[MW],
                                                 int sig, int mg, int tcol0, bool active, int lane,
                                                 const KT& K, const float* Ew = nullptr) {
    if (FASTSVC_DBG_ON(p, DBG_NO_EPILOGUE)) { ws_epilogue_tile<MW, NW>(p, R, acc, s1, s2, sig, mg, tcol0, active, lane); return; }
    if (!active) return;                                   // whole wave (uniform)
    const float slope = (p.flags & F_POST_LRELU) ? LRELU_SLOPE : 1.0f;     // max(v, slope*v): identity for 1
    const int shift_soff = p.COUT * p.ldy * 4;
    // items whose loads fly together (register budget)
    // (FiLM-affine, operands not staged in LDS: NW = 3 fetches the three items of a channel tile together - fetched one
    // at a time each item waited out a memory round trip, nine of them per tile in conv_hx<3,3,1,4,0,4,1>; NW = 4: two at a
    // time - one at a time the ISA of conv_hx<3,4,2,2,0,4,1> was load, vmcnt(0), store, load, vmcnt(0) ... twelve times per tile)
    constexpr int G = (EPI == EPI_AFF) ? (NW == 2 ? 2 : (NW == 3 && !EST) ? 3 : (NW == 4 && !EST) ? 2 : 1) : (NW <= 4 ? NW : (NW % 4 == 0 ? 4 : (NW % 3 == 0 ? 3 : 2)));
    constexpr bool SOFT = TAILMODE == 2;
    constexpr bool TAIL = TAILMODE < 0 ? ws_tail_ok<MW, NW, MODE_DIRECT, EPI, 1>() : (TAILMODE == 1);
    const bool soft_tail = SOFT && (p.T & 3) != 0;
    #pragma unroll
    for (int m = 0; m < MW; ++m) {
        const int cot = (mg * MW + m) * 16 + (lane & 15);
        const bool cok = cot < p.COUT;
        const int co = cok ? cot : 0;
        const float bias = K.bias(p, sig, m, cot);
        const float iv = K.inv(m);
        float r1w = 0.f, r1b = 0.f;
        if (EPI == EPI_RANK1) { r1w = K.r1w(p, sig, m, co); r1b = K.r1b(p, sig, m, co); }
        const int rowoff = co * p.ldy;
        #pragma unroll
        for (int n0 = 0; n0 < NW; n0 += G) {
            int off[G], nv[G];
            f32x4 l0[G], l1[G], l2[G];
            #pragma unroll
            for (int g = 0; g < G; ++g) {                  // every load of the group first
                const int t = tcol0 + (n0 + g) * 16 + (lane >> 4) * 4;
                const bool ok = cok && t < p.T;
                nv[g] = TAIL ? (ok ? row_valid(t, p.T) : 0) : (soft_tail ? row_valid(t, p.T) : 4);
                off[g] = ok ? (rowoff + t) * 4 : OOB_OFF;
                if constexpr (EST) {
                    const float* slot = Ew + (m * NW + n0 + g) * EST_ITEM_FLOATS;
                    if (EPI == EPI_RES) l0[g] = est_read(slot, lane);
                    if (EPI == EPI_AFF) {
                        l1[g] = est_read(slot, lane);
                        l2[g] = est_read(slot + MW * NW * EST_ITEM_FLOATS, lane);
                        l0[g] = p.res ? est_read(slot + 2 * MW * NW * EST_ITEM_FLOATS, lane) : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                } else {
                    if (EPI == EPI_RES) l0[g] = act_load4(R.res, off[g], 0);
                    if (EPI == EPI_RANK1) l0[g] = buf_load4(R.r1x, ok ? t * 4 : OOB_OFF, 0);
                    if (EPI == EPI_AFF) {
                        l0[g] = act_load4(R.res, off[g], 0);              // zero-length descriptor when absent
                        l1[g] = act_load4(R.ss, off[g], 0);
                        l2[g] = act_load4(R.ss, off[g], shift_soff);
                    }
                }
            }
            #pragma unroll
            for (int g = 0; g < G; ++g) {
                f32x4 v = KT::finish(acc[n0 + g][m], iv, bias);
                v.x = fmaxf(v.x, v.x * slope); v.y = fmaxf(v.y, v.y * slope);
                v.z = fmaxf(v.z, v.z * slope); v.w = fmaxf(v.w, v.w * slope);
                if (EPI == EPI_RES || EPI == EPI_AFF) v += l0[g];
                if (EPI == EPI_RANK1) v += l0[g] * r1w + r1b;
                acc[n0 + g][m] = v;                                   // (the finished value, for callers that go on with it)
                store_row4<TAIL>(R.y, off[g], v, nv[g]);              // dropped when y is absent
                if (EPI == EPI_AFF) {
                    f32x4 u = keep_row<TAIL>(l1[g] * v + l2[g], nv[g]);
                    if (soft_tail) u = keep_first(u, nv[g]);
                    store_row4<TAIL>(R.y2, off[g], u, nv[g]);
                    s1[m] += (u.x + u.y) + (u.z + u.w);
                    s2[m] += (u.x * u.x + u.y * u.y) + (u.z * u.z + u.w * u.w);
                }
                // (what lies past the row end - the next row's head, or in a ragged batch whatever the pitch holds - is
                // not this tensor's: a stale 1e30 there once became the tensor's "maximum" and scaled the consumer's
                // staging to nothing; found by tools/stress_parity.py on a no-speaker ragged batch)
                if constexpr (TRACK < 0 ? (EPI == EPI_RES || EPI == EPI_RANK1) : (TRACK != 0))
                    amax_track(R, (TAIL || soft_tail) ? keep_first(v, nv[g]) : v);
            }
        }
    }
}

// Polyphase epilogue (MODE_POLY): a lane holds z, a, c for FOUR consecutive input columns of one
// output channel, i.e. 4*S consecutive output samples = S float4 stores.  EPI_PLAIN: y = o + bias
// (the stretched residual conv, fastsvc.py:72-75,94); EPI_AFF: t = lrelu(o + bias),
// u = scale * t + shift -> y2, InstanceNorm partial sums (fastsvc.py:57-62,97 + 115-140).
template <int MW, int NW, int EPI, int S, int TAILMODE = -1, class KT>
__device__ __forceinline__ void ws_epilogue_poly(const ConvParams& p, const EpiRsrc& R, f32x4 (&acc)[3][NW][MW],
                                                 float (&s1)[MW], float (&s2)[MW],
                                                 int mg, int tcol0, bool active, int lane, const KT& K) {
    if (!active) return;                                   // whole wave (uniform)
    const float slope = (p.flags & F_POST_LRELU) ? LRELU_SLOPE : 1.0f;
    const int T_out = p.ldy;                               // output row pitch
    const int shift_soff = p.COUT * T_out * 4;
    constexpr int G = (MW <= 2 && NW == 1) ? (S < 4 ? S : 4) : S;  // output float4s whose loads fly together (register budget)
    #pragma unroll
    for (int m = 0; m < MW; ++m) {
        const int cot = (mg * MW + m) * 16 + (lane & 15);
        const bool cok = cot < p.COUT;
        const int co = cok ? cot : 0;
        const float bias = K.bias(p, 0, m, cot);
        const float iv = K.inv(m);
        const int rowoff = co * T_out;
        #pragma unroll
        for (int n = 0; n < NW; ++n) {
            const int t = tcol0 + n * 16 + (lane >> 4) * 4;            // input-rate column
            const bool ok = cok && t < p.T;
            constexpr bool TAIL = TAILMODE < 0 ? ws_tail_ok<MW, NW, MODE_POLY, EPI, S>() : (TAILMODE == 1);
            const bool soft_tail = TAILMODE == 2 && (p.T & 3) != 0;            // (see ws_epilogue_kind)
            const int nvo = (TAIL || soft_tail) ? (ok ? row_valid(t, p.T) * S : 0) : 4 * S;   // valid output samples of this lane
            const int off0 = ok ? (rowoff + t * S) * 4 : OOB_OFF;
            // first / last phase of each input column (bias folded in); the middle phases are z + bias
            const f32x4 zz = KT::finish(acc[1][n][m], iv, bias);
            const f32x4 zf = zz + KT::unscale(acc[0][n][m], iv);
            const f32x4 zl = zz + KT::unscale(acc[2][n][m], iv);
            auto phase_value = [&](int k) -> float {               // k: compile-time after unrolling
                const int jj = k / S, ph = k % S;
                return ph == 0 ? zf[jj] : ph == S - 1 ? zl[jj] : zz[jj];
            };
            #pragma unroll
            for (int q0 = 0; q0 < S; q0 += G) {
                f32x4 l1[G], l2[G];
                if (EPI == EPI_AFF) {
                    #pragma unroll
                    for (int g = 0; g < G; ++g)
                        if (q0 + g < S) {
                            l1[g] = act_load4(R.ss, off0 + (q0 + g) * 16, 0);
                            l2[g] = act_load4(R.ss, off0 + (q0 + g) * 16, shift_soff);
                        }
                }
                #pragma unroll
                for (int g = 0; g < G; ++g)
                    if (q0 + g < S) {
                        const int q = q0 + g;
                        f32x4 v = f32x4{phase_value(4 * q), phase_value(4 * q + 1), phase_value(4 * q + 2), phase_value(4 * q + 3)};
                        v.x = fmaxf(v.x, v.x * slope); v.y = fmaxf(v.y, v.y * slope);
                        v.z = fmaxf(v.z, v.z * slope); v.w = fmaxf(v.w, v.w * slope);
                        const int nv = min(4, max(0, nvo - 4 * q));
                        store_row4<TAIL>(R.y, off0 + q * 16, v, nv);   // dropped when y is absent
                        if (EPI == EPI_AFF) {
                            f32x4 u = keep_row<TAIL>(l1[g] * v + l2[g], nv);
                            if (soft_tail) u = keep_first(u, nv);
                            store_row4<TAIL>(R.y2, off0 + q * 16, u, nv);
                            s1[m] += (u.x + u.y) + (u.z + u.w);
                            s2[m] += (u.x * u.x + u.y * u.y) + (u.z * u.z + u.w * u.w);
                        }
                    }
            }
        }
    }
}

// Winograd epilogue: a lane holds m0..m3 of FOUR consecutive pairs of one output channel = the 8
// consecutive outputs starting at tcol0 + 32 n + 8 (lane >> 4).  The even/odd interleave depends on
// the dilation: D=1 e0 o0 e1 o1 | e2 o2 e3 o3;  D=2 e0 e1 o0 o1 | e2 e3 o2 o3;  D=4 e0..e3 | o0..o3.
template <int MW, int NW, int EPI, int D, class KT>
__device__ __forceinline__ void ws_epilogue_wino(const ConvParams& p, const EpiRsrc& R, f32x4 (&acc)[4][NW][MW],
                                                 int sig, int mg, int tcol0, bool active, int lane, const KT& K) {
    if (!active) return;                                   // whole wave (uniform)
    const float slope = (p.flags & F_POST_LRELU) ? LRELU_SLOPE : 1.0f;
    #pragma unroll
    for (int m = 0; m < MW; ++m) {
        const int cot = (mg * MW + m) * 16 + (lane & 15);
        const bool cok = cot < p.COUT;
        const int co = cok ? cot : 0;
        const float bias = K.bias(p, sig, m, cot);
        float r1w = 0.f, r1b = 0.f;
        if (EPI == EPI_RANK1) { r1w = K.r1w(p, sig, m, co); r1b = K.r1b(p, sig, m, co); }
        const int rowoff = co * p.ldy;
        #pragma unroll
        for (int n = 0; n < NW; ++n) {
            const int t = tcol0 + n * 32 + (lane >> 4) * 8;
            int off[2], nv[2];
            f32x4 l0[2];
            #pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool ok = cok && t + 4 * h < p.T;
                nv[h] = cok ? row_valid(t + 4 * h, p.T) : 0;
                off[h] = ok ? (rowoff + t + 4 * h) * 4 : OOB_OFF;
                if (EPI == EPI_RES) l0[h] = act_load4(R.res, off[h], 0);
                if (EPI == EPI_RANK1) l0[h] = buf_load4(R.r1x, ok ? (t + 4 * h) * 4 : OOB_OFF, 0);
            }
            const f32x4 m1 = acc[1][n][m], m2 = acc[2][n][m];
            const f32x4 e = acc[0][n][m] + m1 + m2 + bias;
            const f32x4 o = m1 - m2 - acc[3][n][m] + bias;
            f32x4 v[2];
            if (D == 1) { v[0] = f32x4{e.x, o.x, e.y, o.y}; v[1] = f32x4{e.z, o.z, e.w, o.w}; }
            else if (D == 2) { v[0] = f32x4{e.x, e.y, o.x, o.y}; v[1] = f32x4{e.z, e.w, o.z, o.w}; }
            else { v[0] = e; v[1] = o; }
            #pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 w = v[h];
                w.x = fmaxf(w.x, w.x * slope); w.y = fmaxf(w.y, w.y * slope);
                w.z = fmaxf(w.z, w.z * slope); w.w = fmaxf(w.w, w.w * slope);
                if (EPI == EPI_RES) w += l0[h];
                if (EPI == EPI_RANK1) w += l0[h] * r1w + r1b;
                act_store4_n(R.y, off[h], w, nv[h]);
                // the running maximum counts the row's OWN elements only: a float4 that straddles the row end also holds
                // whatever the workspace holds past it (the residual load), and a stale huge value there would scale the
                // next layer's split-binary16 staging to nothing (same rule as the direct / generic epilogues)
                if constexpr (EPI == EPI_RES || EPI == EPI_RANK1) amax_track(R, keep_first(w, nv[h]));
            }
        }
    }
}

// MODE_DEC2 epilogue: two plain outputs, y = acc[0] + bias, y2 = acc[1] + bias2.
template <int MW, int NW, class KT>
__device__ __forceinline__ void ws_epilogue_dec2(const ConvParams& p, const EpiRsrc& R, f32x4 (&acc)[2][NW][MW],
                                                 int sig, int mg, int tcol0, bool active, int lane, const KT& K) {
    if (!active) return;
    #pragma unroll
    for (int m = 0; m < MW; ++m) {
        const int cot = (mg * MW + m) * 16 + (lane & 15);
        const bool cok = cot < p.COUT;
        const int co = cok ? cot : 0;
        const float bias = K.bias(p, sig, m, cot), bias2 = K.bias2(p, sig, m, cot);
        const float iv = K.inv(m), iv2 = K.inv2(m);
        const int rowoff = co * p.ldy;
        #pragma unroll
        for (int n = 0; n < NW; ++n) {
            const int t = tcol0 + n * 16 + (lane >> 4) * 4;
            const bool ok = cok && t < p.T;
            const int nv = ok ? row_valid(t, p.T) : 0;
            const int off = ok ? (rowoff + t) * 4 : OOB_OFF;
            const f32x4 v = KT::finish(acc[0][n][m], iv, bias);
            act_store4_n(R.y, off, v, nv);
            act_store4_n(R.y2, off, KT::finish(acc[1][n][m], iv2, bias2), nv);
        }
    }
}

