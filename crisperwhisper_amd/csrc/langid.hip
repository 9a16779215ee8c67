// Language identification from the logits the decode step left on the device (engine.hip: cw_detect_language):
//   language_probs_kernel   one block per row of f32 logits [rows][ldv], V valid columns.
//     language part   the n_lang <= CW_LANG_IDS_MAX candidate logits l_k = x[lang_ids[k]] (a NaN counts as -inf: never a
//                     candidate); best = the largest, lowest token id on an exact tie; prob[k] = expf(l_k - m) / S with m the
//                     candidates' maximum and S the f32 sum of expf(l_j - m) over the candidates ONLY (Whisper's detect_language:
//                     every other column masked, then softmax), written in table order.  A candidate at -inf gets exactly 0;
//                     no candidate above -inf: best = the lowest candidate id, every prob NaN (expf(-inf - -inf)).
//     no-speech part  (ns_tok >= 0) expf(x[ns_tok] - M) / Z over the V columns: float4 loads, per thread a running maximum and
//                     sum of exponentials, rescaled once to the row maximum.  The pad columns V .. ldv-1 never count.
//   Reduction order (fixed: a row's values do not depend on its index, the batch or the run):
//     thread   groups tid, tid + 256, ... of four columns: s = s * expf(m_old - m_new) + (((e0 + e1) + e2) + e3)
//     wave     xor butterfly over offsets 32, 16, 8, 4, 2, 1 (every lane ends with the same bits: a + b == b + a)
//     block    (w0 + w1) + (w2 + w3) of the four wave results from LDS
//   Record per row, n_lang + 2 words: best (int32), no-speech probability (NaN when not asked for), prob[n_lang].
//   No atomics, no scratch, 48 bytes of LDS.
#include "common.h"
#include "kernels.h"

__device__ static inline bool lang_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ static inline float lang_wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__global__ __launch_bounds__(256) void language_probs_kernel(const float* __restrict__ logits, int ldv, int V,
                                                             const int* __restrict__ lang_ids, int n_lang, int ns_tok,
                                                             float* __restrict__ out) {
    __shared__ float s_v[4], s_s[4];
    __shared__ int s_i[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lg = logits + (size_t)row * ldv;
    float* rec = out + (size_t)row * (n_lang + 2);

    // ---- language part: candidate k on thread k (n_lang <= 128: waves 2 and 3 carry neutral elements)
    float l = -INFINITY;
    int id = 0x7fffffff;
    if (tid < n_lang) {
        id = lang_ids[tid];
        l = lg[id];
        if (l != l) l = -INFINITY;
    }
    float bv = l;
    int bi = id;
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (lang_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
    __syncthreads();
    bv = s_v[0]; bi = s_i[0];
    for (int w = 1; w < 4; ++w)
        if (lang_better(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
    const float e = tid < n_lang ? expf(l - bv) : 0.f;       // -inf - -inf = NaN: a row without a candidate reports NaN
    const float ws = lang_wave_sum(e);
    if (lane == 0) s_s[wave] = ws;
    __syncthreads();
    const float S = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
    if (tid < n_lang) rec[2 + tid] = e / S;
    if (tid == 0) rec[0] = __int_as_float(bi);
    if (ns_tok < 0) {
        if (tid == 0) rec[1] = __int_as_float(0x7fc00000);
        return;
    }
    __syncthreads();                                          // s_v / s_s are reused below

    // ---- no-speech part: online maximum and sum of exponentials over the V columns
    float m = -INFINITY, s = 0.f;
    const int n4 = ldv >> 2;
    for (int g = tid; g < n4; g += 256) {
        const float4 q = *(const float4*)(lg + 4 * g);
        const int c0 = 4 * g;
        const float v0 = c0 < V ? q.x : -INFINITY, v1 = c0 + 1 < V ? q.y : -INFINITY;
        const float v2 = c0 + 2 < V ? q.z : -INFINITY, v3 = c0 + 3 < V ? q.w : -INFINITY;
        const float mn = fmaxf(fmaxf(fmaxf(m, v0), fmaxf(v1, v2)), v3);
        if (mn > -INFINITY) {
            const float add = ((expf(v0 - mn) + expf(v1 - mn)) + expf(v2 - mn)) + expf(v3 - mn);
            s = (m > -INFINITY ? s * expf(m - mn) : 0.f) + add;
            m = mn;
        }
    }
    float wm = m;
    for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o, 64));
    if (lane == 0) s_v[wave] = wm;
    __syncthreads();
    const float M = fmaxf(fmaxf(s_v[0], s_v[1]), fmaxf(s_v[2], s_v[3]));
    const float zs = lang_wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    if (lane == 0) s_s[wave] = zs;
    __syncthreads();
    if (tid == 0) {
        const float Z = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
        rec[1] = expf(lg[ns_tok] - M) / Z;
    }
}

int cw_launch_language_probs(const float* logits, int ldv, int V, const int* lang_ids, int n_lang, int ns_tok, int rows,
                             float* out, hipStream_t st) {
    if (rows < 1 || V < 1 || ldv < V || (ldv & 3) || n_lang < 1 || n_lang > CW_LANG_IDS_MAX || ns_tok >= V) return CW_ERR_INVALID;
    hipLaunchKernelGGL(language_probs_kernel, dim3(rows), dim3(256), 0, st, logits, ldv, V, lang_ids, n_lang, ns_tok, out);
    return CW_OK;
}
