// Shared device/host helpers for the CrisperWhisper MI355X (gfx950) hot path.
// Written for CDNA4 only: wave = 64 lanes, MFMA 16x16x32 bf16, 160 KiB LDS/CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <math.h>

// The engine's 16-bit storage type.  The dtype-dependent translation units (gemm / attention / elementwise / mel) are compiled
// twice: as is -> bfloat16 (namespace cw_bf16), and with -DCW_F16 -> IEEE binary16, the reference's GPU dtype
// (REF/transcribe.py:10; namespace cw_f16).  The names `bf16_t`, `f32_to_bf16`, `Act<bf16_t>` ... therefore mean "the 16-bit type
// of this build"; only the conversions and the MFMA opcode differ (f32 accumulation, f32 residual stream, f32 softmax / LN
// statistics in both).  binary16 has 3 more significand bits and a 65504 range: every 16-bit tensor of the path (weights, LN
// outputs, attention probabilities <= e^8 under the deferred rescale, K/V, MLP activations) stays far inside it, and the f32
// residual stream makes HF's fp16 overflow clamp (modeling_whisper.py:409-411) unnecessary.
typedef unsigned short bf16_t;

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;  // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) float f32x4_t;   // one MFMA 16x16 C/D fragment

#define CW_WAVE 64

// Streams that exactly one block of a launch reads, once per token step: non-temporal loads (`global_load ... nt`).  Used by the
// cross- and self-attention K/V streams, the logits projection and -- on fragment-major weights, where one wave instruction covers
// eight whole cache lines -- the weight streams of the <= 16-row decode GEMVs (gemv2_bf16_kernel / gemv_stack_kernel / qkv_self_kernel
// <.., WNT>; a run-time choice per launch, CW_NO_WNT).  Not used where a tile is re-read from L2 by design
// (row groups, 17..64 rows), on row-major weights, on operands every block re-reads (activation rows, bias, partial planes) or on
// granule hand-offs.  -DCW_NO_NT restores the default policy everywhere (A/B builds).
#ifdef CW_NO_NT
#define CW_STREAM_LD(p) (*(p))
#else
#define CW_STREAM_LD(p) __builtin_nontemporal_load(p)
#endif

// host conversions of both formats (the engine TU uploads weights for either build)
static inline float cw_host_bf16_to_f32(unsigned short v) { union { uint32_t u; float f; } x; x.u = ((uint32_t)v) << 16; return x.f; }
static inline unsigned short cw_host_f32_to_bf16(float f) {   // round-nearest-even (NaN stays quiet NaN)
    union { uint32_t u; float f; } x; x.f = f;
    const uint32_t rounded = (x.u + 0x7fffu + ((x.u >> 16) & 1u)) >> 16;
    const uint32_t nan = (x.u >> 16) | 0x40u;
    return (unsigned short)(((x.u & 0x7fffffffu) > 0x7f800000u) ? nan : rounded);
}
static inline unsigned short cw_host_f32_to_f16(float f) {    // IEEE binary16, round-nearest-even, overflow -> inf
    union { uint32_t u; float f; } x; x.f = f;
    const uint32_t sign = (x.u >> 16) & 0x8000u;
    uint32_t a = x.u & 0x7fffffffu;
    if (a > 0x7f800000u) return (unsigned short)(sign | 0x7e00u);             // NaN
    if (a >= 0x47800000u) return (unsigned short)(sign | 0x7c00u);            // >= 65536 (or inf) -> inf
    if (a < 0x33000000u) return (unsigned short)sign;                          // < 2^-25 -> 0
    if (a < 0x38800000u) {                                                     // subnormal half
        const int shift = 126 - (int)(a >> 23);                               // 14..24
        uint32_t m = (a & 0x7fffffu) | 0x800000u;
        const uint32_t rnd = 1u << (shift - 1), rest = m & ((1u << shift) - 1u);
        m >>= shift;
        if (rest > rnd || (rest == rnd && (m & 1u))) ++m;
        return (unsigned short)(sign | m);
    }
    uint32_t h = ((a - 0x38000000u) >> 13);
    const uint32_t rest = a & 0x1fffu;
    if (rest > 0x1000u || (rest == 0x1000u && (h & 1u))) ++h;                 // may carry into the exponent (-> inf at the top)
    return (unsigned short)(sign | h);
}
static inline float cw_host_f16_to_f32(unsigned short v) {
    const uint32_t sign = ((uint32_t)v & 0x8000u) << 16, e = (v >> 10) & 0x1f, m = v & 0x3ff;
    union { uint32_t u; float f; } x;
    if (e == 0) {
        if (m == 0) { x.u = sign; return x.f; }
        float f = (float)m * (1.0f / 16777216.0f);                            // m * 2^-24
        return sign ? -f : f;
    }
    if (e == 31) { x.u = sign | 0x7f800000u | (m << 13); return x.f; }
    x.u = sign | ((e + 112) << 23) | (m << 13);
    return x.f;
}

#ifdef CW_F16
#define CW_NS cw_f16
typedef __attribute__((ext_vector_type(8))) _Float16 cw_mfma16x8;
__host__ __device__ static inline float bf16_to_f32(bf16_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, v);
#else
    return cw_host_f16_to_f32(v);
#endif
}
__host__ __device__ static inline bf16_t f32_to_bf16(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(bf16_t, (_Float16)f);                           // v_cvt_f16_f32, round-nearest-even
#else
    return cw_host_f32_to_f16(f);
#endif
}
__device__ static inline void h16_unpack8(const uint4& a, float* o) {         // 8 consecutive 16-bit elements -> f32
    const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[2 * i] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] & 0xffffu));
        o[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w[i] >> 16));
    }
}
__device__ static inline f32x4_t cw_mfma_16x16x32(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(cw_mfma16x8, a), __builtin_bit_cast(cw_mfma16x8, b), c, 0, 0, 0);
}
#else
#define CW_NS cw_bf16
typedef __attribute__((ext_vector_type(8))) __bf16 cw_mfma16x8;
__host__ __device__ static inline float bf16_to_f32(bf16_t v) {
    union { uint32_t u; float f; } x; x.u = ((uint32_t)v) << 16; return x.f;
}
__host__ __device__ static inline bf16_t f32_to_bf16(float f) {   // round-nearest-even (NaN stays quiet NaN)
#if defined(__HIP_DEVICE_COMPILE__)
    // gfx950 has a hardware converter: the cast lowers to v_cvt_pk_bf16_f32 (pairs are packed by the compiler)
    return __builtin_bit_cast(bf16_t, (__bf16)f);
#else
    return cw_host_f32_to_bf16(f);
#endif
}
__device__ static inline void h16_unpack8(const uint4& a, float* o) {         // 8 consecutive 16-bit elements -> f32
    o[0] = __uint_as_float(a.x << 16); o[1] = __uint_as_float(a.x & 0xffff0000u);
    o[2] = __uint_as_float(a.y << 16); o[3] = __uint_as_float(a.y & 0xffff0000u);
    o[4] = __uint_as_float(a.z << 16); o[5] = __uint_as_float(a.z & 0xffff0000u);
    o[6] = __uint_as_float(a.w << 16); o[7] = __uint_as_float(a.w & 0xffff0000u);
}
__device__ static inline f32x4_t cw_mfma_16x16x32(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cw_mfma16x8, a), __builtin_bit_cast(cw_mfma16x8, b), c, 0, 0, 0);
}
#endif

// Activation storage trait: the engine runs either fully in f32 (parity mode) or with bf16
// weights/activations (performance mode); memory-bound kernels are templated on the storage type.
template <typename T> struct Act;
template <> struct Act<float> {
    __device__ static inline float ld(const float* p) { return *p; }
    __device__ static inline void st(float* p, float v) { *p = v; }
};
template <> struct Act<bf16_t> {
    __device__ static inline float ld(const bf16_t* p) { return bf16_to_f32(*p); }
    __device__ static inline void st(bf16_t* p, float v) { *p = f32_to_bf16(v); }
};

__device__ inline float gelu_erf(float x) {  // nn.functional.gelu default (exact erf form)
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

// Decode residual stream of the bf16 engine on a 2^-12 grid.  The K-split GEMVs accumulate their partial sums into the
// f32 residual with atomics, whose order varies from run to run; f32 addition is exact -- and therefore order-independent
// -- when every operand is a multiple of one quantum q and the sums stay below 2^24 q.  So the embedding and every
// residual update are rounded to multiples of q = 2^-12 (|x| < 4096 stays exact; 1.2e-4 absolute, far below the bf16
// rounding the next GEMV applies to the normalised row): the engine becomes bit-reproducible run to run at the cost of
// two VALU ops per output element and no extra traffic or synchronisation.
__device__ inline float resid_grid(float v) { return rintf(v * 4096.0f) * (1.0f / 4096.0f); }

// Sum of four squares of the LayerNorm variance, a^2 + b^2 + c^2 + d^2, with the roundings spelled out:
//     fma(a, a, rn(b b)) + fma(c, c, rn(d d)).
// Left to hipcc (-ffp-contract=fast) the expression (a*a + b*b) + (c*c + d*d) is contracted differently from one inlining
// context to the next -- in one and the same kernel the first 256-column chunk of a row got v_pk_mul + v_add, the others two
// v_fmac -- so two copies of one source line are NOT bit-identical (found by the differential test of declayer.hip: one
// last-place difference in a variance at decoder position 313).  Every decode-time LayerNorm goes through this helper.
__device__ inline float cw_sumsq4(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    const float bb = b * b, dd = d * d;
    const float ab = __builtin_fmaf(a, a, bb), cd = __builtin_fmaf(c, c, dd);
    return ab + cd;
}

// Wave-wide reductions on the DPP path (VALU cross-lane moves, a few cycles each).  __shfl_xor compiles to
// ds_bpermute_b32 -- an LDS-crossbar round trip of ~100+ cycles per step, 6 dependent steps per reduction: measured
// 1.2-1.5 us for the four reductions of a fused LayerNorm, which sat on the critical path of every decode GEMV.
// Inclusive scan inside each row of 16 lanes (row_shr 1,2,4,8), then row_bcast:15 / row_bcast:31 carry the row totals
// upwards: lane 63 ends up with the wave total, read back as a scalar.
template <int CTRL, int ROW_MASK>
__device__ inline float dpp_mov(float identity, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ inline float wave_sum(float v) {
    v += dpp_mov<0x111, 0xf>(0.f, v);   // row_shr:1
    v += dpp_mov<0x112, 0xf>(0.f, v);   // row_shr:2
    v += dpp_mov<0x114, 0xf>(0.f, v);   // row_shr:4
    v += dpp_mov<0x118, 0xf>(0.f, v);   // row_shr:8    lane 15 of each row = row total
    v += dpp_mov<0x142, 0xa>(0.f, v);   // row_bcast:15 rows 1, 3 += total of the row below
    v += dpp_mov<0x143, 0xc>(0.f, v);   // row_bcast:31 rows 2, 3 += total of rows 0-1
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ inline float wave_max(float v) {
    v = fmaxf(v, dpp_mov<0x111, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x112, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x114, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x118, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x142, 0xa>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x143, 0xc>(-INFINITY, v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Cross-row exchanges (lane ^ 16, lane ^ 32) on gfx950's v_permlane16/32_swap: with both operands = v the two results
// are the even-row and odd-row (lower-half and upper-half) copies, so op(r0, r1) is the butterfly step in one VALU op.
__device__ inline float xor16_max(float v) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ inline float xor32_max(float v) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ inline float xor16_sum(float v) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ inline float xor32_sum(float v) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// Block-wide reductions through a small LDS scratch (>= 32 floats).  All threads get the result.
__device__ inline float block_sum(float v, float* scratch) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += scratch[i];
    return r;
}
__device__ inline float block_max(float v, float* scratch) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    float r = -INFINITY;
    for (int i = 0; i < nw; ++i) r = fmaxf(r, scratch[i]);
    return r;
}

// ---------------------------------------------------------------------------------------------
// GEMM epilogues.  Every GEMM flavour (MFMA bf16 tile GEMM, f32 parity GEMM, decode GEMV) funnels
// its accumulators through epi_store4(): 4 consecutive output columns n..n+3 of one row m.
// ---------------------------------------------------------------------------------------------
enum EpiMode {
    EPI_STORE = 0,       // out[m][n] = T(acc + bias)
    EPI_GELU = 1,        // out[m][n] = T(gelu(acc + bias))
    EPI_RESID_F32 = 2,   // outf[m][n] = resid[m][n] + acc + bias            (f32 residual stream)
    EPI_GELU_POS_F32 = 3,// outf[m][n] = gelu(acc + bias) + pos[m % T][n]     (conv2 + sinusoid pos)
    EPI_HEADS = 4,       // split columns into (which, head, dd); rows into (b, s):
                         //   outs[which][((b*H + h)*S_pad + s)*64 + dd] = T(acc + bias)
    EPI_STORE_F32 = 5,   // outf[m][n] = acc + bias                            (logits, q vectors)
    EPI_QKV_CACHE = 6,   // decode: which==0 -> outf[m][n] (q, f32); 1/2 -> self-KV cache row `pos`
    EPI_GELU_F32 = 7,    // outf[m][n] = gelu(acc + bias)                      (decode MLP mid)
    EPI_GELU_FRAG = 8,   // bf16 gelu(acc + bias) in MFMA fragment-major order (gemm.hip, 17..64-row decode GEMV), K' = ldo
};

struct EpiParams {
    void* out;            // T* (EPI_STORE/GELU) or base for `which == 0` (EPI_HEADS)
    void* out1;           // which == 1
    void* out2;           // which == 2
    float* outf;          // f32 outputs
    const float* bias;    // [N] or null
    const float* resid;   // [M][ldo] f32
    const float* pos;     // [T][N] f32
    int ldo;              // leading dimension of out/outf/resid
    int T;                // rows per batch item (EPI_GELU_POS_F32, EPI_HEADS)
    int S_pad;            // padded per-head sequence capacity (EPI_HEADS / cache capacity)
    int H;                // heads
    int d_model;          // columns per `which`
    const int* row_pos;   // EPI_QKV_CACHE: [batch] device array, cache row to write for each batch row
    int x16;              // decode GEMV: the activation rows are 16-bit (a producer's EPI_GELU output) instead of f32
    int row_pos_pre;      // EPI_QKV_CACHE with row_pos == nullptr: the cache row, read by the kernel at entry (the decode GEMVs: a
                          // dependent load + vmcnt(0) in the epilogue otherwise -- one L2 round trip per stored row tile)
};

// MFMA 16x16x32 A-operand fragment-major position of activation (row m, column k) of a [rows][K] matrix:
// xf[((mt * K/32 + ks) * 64 + g*16 + l15) * 8 + e], row = mt*16 + l15, k = ks*32 + g*8 + e.
__host__ __device__ inline size_t frag_index(int m, int k, int K) {
    return (((size_t)(m >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (m & 15)) * 8 + (k & 7);
}

template <typename T, int MODE>
__device__ inline void epi_store1(const EpiParams& p, int m, int n, float acc) {
    float v = acc + (p.bias ? p.bias[n] : 0.f);
    if (MODE == EPI_STORE) {
        Act<T>::st((T*)p.out + (size_t)m * p.ldo + n, v);
    } else if (MODE == EPI_GELU) {
        Act<T>::st((T*)p.out + (size_t)m * p.ldo + n, gelu_erf(v));
    } else if (MODE == EPI_RESID_F32) {
        size_t o = (size_t)m * p.ldo + n;
        p.outf[o] = p.resid[o] + v;
    } else if (MODE == EPI_GELU_POS_F32) {
        p.outf[(size_t)m * p.ldo + n] = gelu_erf(v) + p.pos[(size_t)(m % p.T) * p.ldo + n];
    } else if (MODE == EPI_HEADS) {
        int which = n / p.d_model, r = n - which * p.d_model;
        int h = r >> 6, dd = r & 63;
        int b = m / p.T, s = m - b * p.T;
        T* base = (T*)(which == 0 ? p.out : (which == 1 ? p.out1 : p.out2));
        Act<T>::st(base + (((size_t)b * p.H + h) * p.S_pad + s) * 64 + dd, v);
    } else if (MODE == EPI_STORE_F32) {
        p.outf[(size_t)m * p.ldo + n] = v;
    } else if (MODE == EPI_GELU_F32) {
        p.outf[(size_t)m * p.ldo + n] = gelu_erf(v);
    } else if (MODE == EPI_GELU_FRAG) {
        ((unsigned short*)p.out)[frag_index(m, n, p.ldo)] = f32_to_bf16(gelu_erf(v));
    } else if (MODE == EPI_QKV_CACHE) {
        int which = n / p.d_model, r = n - which * p.d_model;
        if (which == 0) {
            p.outf[(size_t)m * p.d_model + r] = v;
        } else {
            int h = r >> 6, dd = r & 63;
            T* base = (T*)(which == 1 ? p.out1 : p.out2);
            const int rpos = p.row_pos ? p.row_pos[m] : p.row_pos_pre;
            Act<T>::st(base + (((size_t)m * p.H + h) * p.S_pad + rpos) * 64 + dd, v);
        }
    }
}

// erf for the bf16 path: Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7, far below bf16 resolution); the f32
// parity path keeps erff().
__device__ inline float gelu_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __frcp_rn(1.0f + 0.3275911f * z);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float e = 1.0f - poly * __expf(-z * z);
    return 0.5f * x * (1.0f + copysignf(e, x));
}

// Vectorised epilogue of the tile GEMMs: 4 consecutive output columns n..n+3 (n % 4 == 0, all < N) of row m.
template <typename T> struct Pack4;
template <> struct Pack4<bf16_t> {
    __device__ static inline void st(bf16_t* p, float a, float b, float c, float d) {
        ushort4 o; o.x = f32_to_bf16(a); o.y = f32_to_bf16(b); o.z = f32_to_bf16(c); o.w = f32_to_bf16(d);
        *(ushort4*)p = o;
    }
    __device__ static inline float gelu(float x) { return gelu_fast(x); }
};
template <> struct Pack4<float> {
    __device__ static inline void st(float* p, float a, float b, float c, float d) { *(float4*)p = make_float4(a, b, c, d); }
    __device__ static inline float gelu(float x) { return gelu_erf(x); }
};

template <typename T, int MODE>
__device__ inline void epi_store4(const EpiParams& p, int m, int n, float a0, float a1, float a2, float a3) {
    if (p.bias) {
        const float4 b = *(const float4*)(p.bias + n);
        a0 += b.x; a1 += b.y; a2 += b.z; a3 += b.w;
    }
    if (MODE == EPI_STORE) {
        Pack4<T>::st((T*)p.out + (size_t)m * p.ldo + n, a0, a1, a2, a3);
    } else if (MODE == EPI_GELU) {
        Pack4<T>::st((T*)p.out + (size_t)m * p.ldo + n, Pack4<T>::gelu(a0), Pack4<T>::gelu(a1), Pack4<T>::gelu(a2), Pack4<T>::gelu(a3));
    } else if (MODE == EPI_RESID_F32) {
        const size_t o = (size_t)m * p.ldo + n;
        const float4 r = *(const float4*)(p.resid + o);
        *(float4*)(p.outf + o) = make_float4(r.x + a0, r.y + a1, r.z + a2, r.w + a3);
    } else if (MODE == EPI_GELU_POS_F32) {
        const float4 ps = *(const float4*)(p.pos + (size_t)(m % p.T) * p.ldo + n);
        *(float4*)(p.outf + (size_t)m * p.ldo + n) =
            make_float4(Pack4<T>::gelu(a0) + ps.x, Pack4<T>::gelu(a1) + ps.y, Pack4<T>::gelu(a2) + ps.z, Pack4<T>::gelu(a3) + ps.w);
    } else if (MODE == EPI_HEADS) {
        const int which = n / p.d_model, r = n - which * p.d_model;
        const int h = r >> 6, dd = r & 63;
        const int b = m / p.T, s = m - b * p.T;
        T* base = (T*)(which == 0 ? p.out : (which == 1 ? p.out1 : p.out2));
        Pack4<T>::st(base + (((size_t)b * p.H + h) * p.S_pad + s) * 64 + dd, a0, a1, a2, a3);
    } else if (MODE == EPI_STORE_F32) {
        *(float4*)(p.outf + (size_t)m * p.ldo + n) = make_float4(a0, a1, a2, a3);
    }
}

// Tile epilogue with the row / column decompositions hoisted out of the 4x4 fragment loop: per lane 4 row
// offsets (integer divisions for the head-split and position layouts happen here, 4 instead of 16 times) and
// 4 column descriptors (bias vector, destination pointer), then 16 vector stores.  rows[i] / cols[j] are the
// lane's 4 row indices and 4 first-column indices (cols multiple of 4), all inside [0,M) x [0,N).
template <typename T, int MODE>
__device__ inline void epi_tile_interior(const EpiParams& p, const int (&rows)[4], const int (&cols)[4],
                                         const f32x4_t (&acc)[4][4]) {
    size_t roff[4]; int rpos[4];
    float4 bias[4]; size_t coff[4]; T* cbase[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = rows[i];
        rpos[i] = 0;
        if (MODE == EPI_HEADS) {
            const int b = m / p.T, s_ = m - b * p.T;
            roff[i] = ((size_t)b * p.H * p.S_pad + s_) * 64;
        } else {
            roff[i] = (size_t)m * p.ldo;
            if (MODE == EPI_GELU_POS_F32) rpos[i] = m % p.T;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = cols[j];
        bias[j] = p.bias ? *(const float4*)(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
        cbase[j] = (T*)p.out;
        if (MODE == EPI_HEADS) {
            const int which = n / p.d_model, r = n - which * p.d_model;
            cbase[j] = (T*)(which == 0 ? p.out : (which == 1 ? p.out1 : p.out2));
            coff[j] = (size_t)(r >> 6) * p.S_pad * 64 + (r & 63);
        } else {
            coff[j] = (size_t)n;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a0 = acc[i][j][0] + bias[j].x, a1 = acc[i][j][1] + bias[j].y;
            const float a2 = acc[i][j][2] + bias[j].z, a3 = acc[i][j][3] + bias[j].w;
            const size_t o = roff[i] + coff[j];
            if (MODE == EPI_STORE || MODE == EPI_HEADS) {
                Pack4<T>::st(cbase[j] + o, a0, a1, a2, a3);
            } else if (MODE == EPI_GELU) {
                Pack4<T>::st(cbase[j] + o, Pack4<T>::gelu(a0), Pack4<T>::gelu(a1), Pack4<T>::gelu(a2), Pack4<T>::gelu(a3));
            } else if (MODE == EPI_RESID_F32) {
                const float4 r = *(const float4*)(p.resid + o);
                *(float4*)(p.outf + o) = make_float4(r.x + a0, r.y + a1, r.z + a2, r.w + a3);
            } else if (MODE == EPI_GELU_POS_F32) {
                const float4 ps = *(const float4*)(p.pos + (size_t)rpos[i] * p.ldo + cols[j]);
                *(float4*)(p.outf + o) = make_float4(Pack4<T>::gelu(a0) + ps.x, Pack4<T>::gelu(a1) + ps.y,
                                                     Pack4<T>::gelu(a2) + ps.z, Pack4<T>::gelu(a3) + ps.w);
            } else if (MODE == EPI_STORE_F32) {
                *(float4*)(p.outf + o) = make_float4(a0, a1, a2, a3);
            }
        }
}

// Host-side error plumbing -----------------------------------------------------------------------
#define CW_OK 0
#define CW_ERR_INVALID (-22)
#define CW_ERR_NOMEM (-12)
#define CW_ERR_HIP (-5)
#define CW_ERR_STATE (-1)
#define CW_TOP_LOGPROBS_MAX 8   /* as in include/crisperwhisper.h: alternatives per position (cw_set_top_logprobs) */
#define CW_LANG_IDS_MAX 128     /* as in include/crisperwhisper.h: language candidates (cw_detect_language) */
