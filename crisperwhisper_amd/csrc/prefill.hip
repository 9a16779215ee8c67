// Decoder prompt prefill (16-bit engines): one decoder forward over rows x n_pos prompt positions at once, on the matrix cores.
// It leaves the self-attention K/V cache rows 0 .. n_pos-1 of every layer exactly where the per-position decode step writes them
// ([row][head][cap][64]); engine.hip: run_prefill drives it layer by layer.
//
//   prefill_embed_kernel   x[m] = embed[token] + pos_embed[pos]                       (f32 residual, m = row * n_pos + pos)
//   prefill_ln_kernel      a[m] = (x[m] - mean) * rstd as 16-bit                      (the LN affine is folded into W / bias)
//   prefill_gemm_kernel    C = A W^T + bias, MFMA 16x16x32 over fragment-major packed W (gemm.hip: wfrag_pack_kernel), epilogues:
//                          16-bit store | q store + self-cache scatter of k / v | f32 residual add | erf GELU to 16-bit
//   prefill_attn_kernel    flash attention of 16 query positions of one (row, head): online softmax in f32, MFMA for Q K^T and
//                          P V; causal over the row's own self cache, or every key of the row's cross K/V cache; in cross mode
//                          it can record the alignment heads' attention rows (forced alignment, engine.hip: cw_align_tokens)
#include <hip/hip_runtime.h>
#include <string.h>
#include "kernels.h"

namespace CW_NS {

__global__ __launch_bounds__(256) void prefill_embed_kernel(const int* __restrict__ ids, int ids_stride, int n_pos,
                                                            const bf16_t* __restrict__ embed, const float* __restrict__ pos_embed,
                                                            float* __restrict__ x, int M, int D) {
    const int m = blockIdx.x;
    if (m >= M) return;
    const int r = m / n_pos, p = m - r * n_pos;
    const int tok = ids[(size_t)r * ids_stride + p];
    for (int k = threadIdx.x; k < D; k += blockDim.x)
        x[(size_t)m * D + k] = resid_grid(Act<bf16_t>::ld(embed + (size_t)tok * D + k) + pos_embed[(size_t)p * D + k]);
}

// one wave per row, 4 rows per block
__global__ __launch_bounds__(256) void prefill_ln_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int M, int D) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* xr = x + (size_t)m * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s += xr[k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)D;
    float q = 0.f;
    for (int k = lane; k < D; k += 64) { const float d = xr[k] - mean; q += d * d; }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q / (float)D + 1e-5f);
    for (int k = lane; k < D; k += 64) Act<bf16_t>::st(out + (size_t)m * D + k, (xr[k] - mean) * rstd);
}

// 4 waves per block as 2 x 2; each wave owns 32 rows x 32 columns (2 x 2 MFMA tiles); K % 32 == 0, N % 16 == 0.
// A: [M][K] 16-bit row-major; W: [N][K] fragment-major (tile t of 16 output rows, k step s: 64 lanes x 8 elements at
// ((t * K/32 + s) * 64 + lane) * 8 = W[t*16 + (lane & 15)][s*32 + (lane >> 4) * 8 ..]), i.e. the MFMA B operand as stored.
__global__ __launch_bounds__(256) void prefill_gemm_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                           PrefillEpi ep, int M, int N, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 64 + (wave >> 1) * 32;
    const int n0 = blockIdx.x * 64 + (wave & 1) * 32;
    const int KS = K >> 5;
    const int l15 = lane & 15, g = lane >> 4;
    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bool nv[2] = {n0 < N, n0 + 16 < N};
    const bool mv[2] = {m0 + l15 < M, m0 + 16 + l15 < M};
    const bf16x8_t zero = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < KS; ++s) {
        bf16x8_t a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
            a[i] = mv[i] ? *(const bf16x8_t*)(A + (size_t)(m0 + i * 16 + l15) * K + s * 32 + g * 8) : zero;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            b[j] = nv[j] ? *(const bf16x8_t*)(W + ((((size_t)((n0 >> 4) + j) * KS) + s) * 64 + lane) * 8) : zero;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = cw_mfma_16x16x32(a[i], b[j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + j * 16 + l15;
            if (!nv[j]) continue;
            const float bias = ep.bias ? ep.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + i * 16 + g * 4 + r;
                if (m >= M) continue;
                const float v = acc[i][j][r] + bias;
                if (ep.mode == PF_STORE) {
                    Act<bf16_t>::st((bf16_t*)ep.out + (size_t)m * N + n, v);
                } else if (ep.mode == PF_GELU) {
                    Act<bf16_t>::st((bf16_t*)ep.out + (size_t)m * N + n, gelu_erf(v));
                } else if (ep.mode == PF_RESID) {
                    ep.x[(size_t)m * N + n] += v;
                } else {                                          // PF_QKV: q -> out [M][D]; k / v -> self cache [row][h][cap][64]
                    const int which = n / ep.D, c = n - which * ep.D;
                    if (which == 0) {
                        Act<bf16_t>::st((bf16_t*)ep.out + (size_t)m * ep.D + c, v);
                    } else {
                        const int row = m / ep.n_pos, p = m - row * ep.n_pos;
                        bf16_t* base = (bf16_t*)(which == 1 ? ep.sk : ep.sv);
                        Act<bf16_t>::st(base + (((size_t)row * ep.H + (c >> 6)) * ep.cap + p) * 64 + (c & 63), v);
                    }
                }
            }
        }
}

// grid (ceil(n_q / 16), H, rows), one wave.  Q: [rows * n_q][H * 64] 16-bit (the 1/8 scale is in the weights); K / V: cache
// [kv rows][H][cap][64], kv row = row / kv_div; causal: query position i sees keys 0 .. i, else keys 0 .. n_keys - 1.
__global__ __launch_bounds__(64) void prefill_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ Kc,
                                                          const bf16_t* __restrict__ Vc, bf16_t* __restrict__ out, int n_q, int H,
                                                          int cap, int n_keys, int causal, int kv_div, PrefillAlign al) {
    __shared__ bf16_t Ps[16][32 + 8];
    __shared__ bf16_t Vs[32][64 + 8];
    const int lane = threadIdx.x, l15 = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.x * 16, h = blockIdx.y, row = blockIdx.z;
    const int D = H * 64;
    const size_t kvo = (((size_t)(row / kv_div)) * H + h) * (size_t)cap * 64;
    const bf16x8_t zero = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8_t qa[2];
    {
        const int i = i0 + l15;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            qa[c] = i < n_q ? *(const bf16x8_t*)(Q + ((size_t)row * n_q + i) * D + h * 64 + c * 32 + g * 8) : zero;
    }
    const int kend = causal ? min(n_keys, i0 + 16) : n_keys;   // keys any of the 16 queries may see
    float mrow[4], lrow[4];
    f32x4_t o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { mrow[r] = -INFINITY; lrow[r] = 0.f; o[r] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    for (int j0 = 0; j0 < kend; j0 += 32) {
        f32x4_t s[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int j = j0 + hh * 16 + l15;
            s[hh] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bf16x8_t kb = j < kend ? *(const bf16x8_t*)(Kc + kvo + (size_t)j * 64 + c * 32 + g * 8) : zero;
                s[hh] = cw_mfma_16x16x32(qa[c], kb, s[hh]);
            }
        }
        // V tile [32 keys][64] into LDS (zero beyond the last key: P is 0 there, but 0 * garbage could be NaN)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int e = (t * 64 + lane) * 8;                   // element of the 32 x 64 tile
            const int jr = e >> 6, d = e & 63;
            const bf16x8_t v = j0 + jr < kend ? *(const bf16x8_t*)(Vc + kvo + (size_t)(j0 + jr) * 64 + d) : zero;
            *(bf16x8_t*)&Vs[jr][d] = v;
        }
        // online softmax: S element (query i0 + g*4 + r, key j0 + hh*16 + l15)
        float p[2][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = i0 + g * 4 + r;
            float mx = -INFINITY;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int j = j0 + hh * 16 + l15;
                const bool ok = j < kend && (!causal || j <= qi);
                p[hh][r] = ok ? s[hh][r] : -INFINITY;
                mx = fmaxf(mx, p[hh][r]);
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            const float mnew = fmaxf(mrow[r], mx);
            const float alpha = mnew == -INFINITY ? 1.f : __expf(mrow[r] - mnew);
            float sum = 0.f;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                p[hh][r] = p[hh][r] == -INFINITY ? 0.f : __expf(p[hh][r] - mnew);
                sum += p[hh][r];
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off, 64);
            lrow[r] = lrow[r] * alpha + sum;
            mrow[r] = mnew;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt][r] *= alpha;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) Act<bf16_t>::st(&Ps[g * 4 + r][hh * 16 + l15], p[hh][r]);
        }
        __syncthreads();
        bf16x8_t pa;                                             // A operand: P[query l15][key g*8 + e]
#pragma unroll
        for (int e = 0; e < 8; ++e) pa[e] = (short)Ps[l15][g * 8 + e];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            bf16x8_t vb;                                         // B operand: V[key g*8 + e][d = dt*16 + l15]
#pragma unroll
            for (int e = 0; e < 8; ++e) vb[e] = (short)Vs[g * 8 + e][dt * 16 + l15];
            o[dt] = cw_mfma_16x16x32(pa, vb, o[dt]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + g * 4 + r;
        if (qi >= n_q) continue;
        const float inv = lrow[r] > 0.f ? 1.f / lrow[r] : 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            Act<bf16_t>::st(out + ((size_t)row * n_q + qi) * D + h * 64 + dt * 16 + l15, o[dt][r] * inv);
    }
    // Alignment heads (cross mode only): a second pass over the keys, once the final (m, l) of every query is known, writes
    // exp(s - m) for query position qi into alignment row qi of slot al.slot[h] -- the row the decode step at position qi
    // writes -- and (m, l) into split 0 of its ATT_NS statistics (the other splits (m, 0)), i.e. what a one-split decode
    // launch leaves for align_normalize_kernel.  S is recomputed with the same MFMA sequence, so it equals the first pass's.
    // Every other head leaves here: the branch is uniform per block.
    const int slot = (al.out && !causal) ? al.slot[h] : -1;
    if (slot < 0) return;
    size_t rowi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rowi[r] = ((size_t)row * al.n_align + slot) * al.rows + (i0 + g * 4 + r);
    for (int j0 = 0; j0 < kend; j0 += 32) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int j = j0 + hh * 16 + l15;
            f32x4_t s = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bf16x8_t kb = j < kend ? *(const bf16x8_t*)(Kc + kvo + (size_t)j * 64 + c * 32 + g * 8) : zero;
                s = cw_mfma_16x16x32(qa[c], kb, s);
            }
            if (j >= kend) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (i0 + g * 4 + r < n_q) al.out[rowi[r] * n_keys + j] = __expf(s[r] - mrow[r]);
        }
    }
    if (l15 < ATT_NS) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (i0 + g * 4 + r < n_q) {
                al.ml[(rowi[r] * ATT_NS + l15) * 2] = mrow[r];
                al.ml[(rowi[r] * ATT_NS + l15) * 2 + 1] = l15 == 0 ? lrow[r] : 0.f;
            }
    }
}

int cw_launch_prefill_embed(const int* ids, int ids_stride, int n_pos, const void* embed, const float* pos_embed, float* x,
                            int M, int D, hipStream_t st) {
    if (M < 1 || n_pos < 1) return CW_ERR_INVALID;
    hipLaunchKernelGGL(prefill_embed_kernel, dim3(M), dim3(256), 0, st, ids, ids_stride, n_pos, (const bf16_t*)embed, pos_embed,
                       x, M, D);
    return CW_OK;
}

int cw_launch_prefill_ln(const float* x, void* out, int M, int D, hipStream_t st) {
    if (M < 1) return CW_ERR_INVALID;
    hipLaunchKernelGGL(prefill_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, st, x, (bf16_t*)out, M, D);
    return CW_OK;
}

int cw_launch_prefill_gemm(const void* A, const void* W, const PrefillEpi& ep, int M, int N, int K, hipStream_t st) {
    if (M < 1 || N < 16 || N % 16 || K < 32 || K % 32) return CW_ERR_INVALID;
    if (ep.mode == PF_QKV && (N != 3 * ep.D || ep.D % 64 || ep.n_pos < 1 || M % ep.n_pos)) return CW_ERR_INVALID;
    hipLaunchKernelGGL(prefill_gemm_kernel, dim3((N + 63) / 64, (M + 63) / 64), dim3(256), 0, st, (const bf16_t*)A,
                       (const bf16_t*)W, ep, M, N, K);
    return CW_OK;
}

int cw_launch_prefill_attn(const void* Q, const void* K, const void* V, void* out, int rows, int n_q, int H, int cap, int n_keys,
                           int causal, int kv_div, hipStream_t st) {
    PrefillAlign none;
    memset(&none, 0, sizeof(none));
    return cw_launch_prefill_attn_align(Q, K, V, out, rows, n_q, H, cap, n_keys, causal, kv_div, none, st);
}

// al.out null: no alignment rows (the prompt prefill).  Otherwise cross mode only, n_q <= al.rows (alignment rows per slot).
int cw_launch_prefill_attn_align(const void* Q, const void* K, const void* V, void* out, int rows, int n_q, int H, int cap,
                                 int n_keys, int causal, int kv_div, const PrefillAlign& al, hipStream_t st) {
    if (rows < 1 || n_q < 1 || H < 1 || n_keys < 1 || n_keys > cap || kv_div < 1 || (causal && n_keys < n_q)) return CW_ERR_INVALID;
    if (al.out && (causal || !al.ml || !al.slot || al.n_align < 1 || n_q > al.rows)) return CW_ERR_INVALID;
    hipLaunchKernelGGL(prefill_attn_kernel, dim3((n_q + 15) / 16, H, rows), dim3(64), 0, st, (const bf16_t*)Q, (const bf16_t*)K,
                       (const bf16_t*)V, (bf16_t*)out, n_q, H, cap, n_keys, causal, kv_div, al);
    return CW_OK;
}

}  // namespace CW_NS
