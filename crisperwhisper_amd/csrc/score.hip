// Scoring head (16-bit engines): the end of a teacher-forced decoder forward for every scored position at once -- final LayerNorm,
// projection onto the vocabulary, log-softmax and the pick of the target token -- without ever writing the [M][V] logits
// (engine.hip: cw_score_tokens, score_head_launch / score_head_fetch).
//
//   score_ln_kernel        a[m] = ((x[src[m]] - mean) * rstd) * g + b as 16-bit    (the final LayerNorm keeps its affine: the
//                          tied embedding is shared with the token lookup, so nothing is folded into it)
//   score_head_kernel      logits tile = a W^T on MFMA 16x16x32 over the fragment-major tied embedding (gemm.hip:
//                          wfrag_pack_kernel); block (m-tile of 128 rows, split of the vocabulary).  Per row, in f32 registers:
//                          running maximum, running sum of exp(logit - max), the target's logit if its column is the block's,
//                          the best (logit, id) -- lowest id on an exact tie, as sample_kernel.  Columns >= V take no part.
//   score_combine_kernel   merges the [M][n_split] partials: logprob = logit[target] - logsumexp, top_id, top_logprob
//   score_rows_kernel      the same three numbers from a row of f32 logits the decode step left (the per-position fallback)
// STOP forms (cw_align_cut_tokens): besides the above, stop_logprob = logsumexp(logit[n], n in S) - logsumexp(all logits) with
// S = {eos} + {n >= timestamp_begin}: the log-probability that the text stops before this position.  S keeps its own running
// (maximum, sum of exp) pair, never rescaled against the row's maximum: a stop set 100 nats under the row maximum would
// underflow to log(0) there.  The pair travels in its own record array (ScoreStopPart); the plain forms write what they wrote.
// TOPK forms (cw_set_score_top_logprobs): besides the above, the k <= CW_TOP_LOGPROBS_MAX best (logit, id) pairs of every row --
// value descending, id ascending on an exact tie, over the columns < V with a logit > -inf -- as alt_id and alt_logprob = logit -
// logsumexp.  The head keeps a sorted list per row and split in LDS and writes it to its own record array (ScoreTopPart), the
// combine kernel merges the splits' lists, the row kernel runs k selection rounds; the logits are still never stored.
// ENT forms (cw_set_score_entropy): besides the above, entropy = log S - Zc / S with S = sum exp(logit - mx), Zc = sum exp(logit - mx)
// (logit - mx) over the columns < V with a logit > -inf.  Wherever a (mx, S, Zc) partial moves to a new centre M it becomes
// (M, S e^(mx - M), (Zc + S (mx - M)) e^(mx - M)): in a lane when its maximum moves, between the 16 lanes of a row, between the
// splits.  Zc travels in its own record array (one float per row and split); the other forms write what they wrote.  A NaN logit,
// which the (maximum, sum) pair steps over, makes the row's entropy NaN.
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace CW_NS {

// one wave per row, 4 rows per block; src null: row m of x
__global__ __launch_bounds__(256) void score_ln_kernel(const float* __restrict__ x, const int* __restrict__ src,
                                                       const float* __restrict__ gam, const float* __restrict__ bet,
                                                       bf16_t* __restrict__ out, int M, int D) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* xr = x + (size_t)(src ? src[m] : m) * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s += xr[k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)D;
    float q = 0.f;
    for (int k = lane; k < D; k += 64) { const float d = xr[k] - mean; q += d * d; }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q / (float)D + 1e-5f);
    for (int k = lane; k < D; k += 64) Act<bf16_t>::st(out + (size_t)m * D + k, (xr[k] - mean) * rstd * gam[k] + bet[k]);
}

__device__ static inline bool score_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ static inline float score_recentre(float z, float s, float d) { return (z + s * d) * expf(d); }   // d = old centre - new <= 0
__device__ static inline float score_entropy(float S, float Zc) {            // rounding may leave a one-point row a hair below 0
    const float H = logf(S) - Zc / S;
    return H < 0.f ? 0.f : H;                                                 // (a NaN stays)
}

// grid (m-tiles of 128 rows, n_split); 4 waves, wave w owns rows m0 + 32 w .. + 31 and walks the split's 16-column tiles four at
// a time (2 x 4 MFMA tiles, 8 accumulators).  The four waves read the same W fragments (one fetch, three cache hits), so one
// block streams its vocabulary slice once for 128 rows.  A: [M][K] 16-bit row-major; W: fragment-major, (V + 15) / 16 tiles.
// C fragment element r of lane (l15, g) is row 16 i + 4 g + r, column 16 j + l15: a lane keeps the statistics of its 8 rows over
// its own columns, and the 16 lanes of a row are merged once at the end.
// STORE (the unfused form, kept for the A/B of cw_time_score_head only): the same tile loop writes the f32 logits [M][ldv]
// instead of keeping statistics; score_rows_kernel then makes one pass per row.
// TOPK (cw_set_score_top_logprobs): besides the above, the split's topk best (logit, id) pairs of every row, in (value descending,
// id ascending) order.  They live in LDS, one sorted list of CW_TOP_LOGPROBS_MAX pairs per row (32 accumulators a lane leave no
// registers for 8 rows x 8 pairs); a wave's 32 rows are its own, so the lists need wave-level ordering only.  A lane keeps its
// rows' topk-th pair in registers and offers a column only if it beats that pair in the full order -- after the first tile
// groups almost none does.  Offers are served one lane at a time per 16-lane group (the four groups own different rows); the
// serving lane tests against the list itself, so the result is the exact top of the split whatever the order of service.
// ENT (cw_set_score_entropy): a lane also keeps zc = sum exp(v - mx) (v - mx) for its 8 rows, and one bit per row for a NaN it saw.
template <bool STORE, bool STOP, bool TOPK = false, bool ENT = false>
__global__ __launch_bounds__(256) void score_head_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                         const int* __restrict__ target, ScorePart* __restrict__ part,
                                                         int M, int V, int K, int tiles_per_split, int n_split,
                                                         float* __restrict__ logits, int ldv,
                                                         ScoreStopPart* __restrict__ spart, int eos, int ts_begin,
                                                         ScoreTopPart* __restrict__ tpart, int topk,
                                                         float* __restrict__ epart) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int m0 = blockIdx.x * 128 + wave * 32;
    const int split = blockIdx.y;
    const int NT = (V + 15) >> 4, KS = K >> 5;
    const int t_begin = split * tiles_per_split;
    const int t_end = min(NT, t_begin + tiles_per_split);
    const bool mv[2] = {m0 + l15 < M, m0 + 16 + l15 < M};
    const bf16x8_t zero = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
    float mx[8], sum[8], tl[8], bv[8];
    int bi[8], tg[8];
    float smx[8], ssum[8];                                            // STOP only: the lane's columns that lie in S
    float zc[8];                                                      // ENT only
    unsigned nanrow = 0;                                              // ENT only: bit q = row q met a NaN logit
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int m = m0 + (q >> 2) * 16 + g * 4 + (q & 3);
        mx[q] = -INFINITY; sum[q] = 0.f; tl[q] = -INFINITY; bv[q] = -INFINITY; bi[q] = 0x7fffffff;
        tg[q] = m < M ? target[m] : -1;
        if (STOP) { smx[q] = -INFINITY; ssum[q] = 0.f; }
        if (ENT) zc[q] = 0.f;
    }
    // TOPK: s_tv / s_ti [128 rows][CW_TOP_LOGPROBS_MAX], sorted best first, (-inf, INT_MAX) where empty; kv / ki: the topk-th pair
    __shared__ float s_tv[TOPK ? 128 * CW_TOP_LOGPROBS_MAX : 1];
    __shared__ int s_ti[TOPK ? 128 * CW_TOP_LOGPROBS_MAX : 1];
    float kv[8];
    int ki[8];
    if (TOPK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s_tv[wave * 32 * CW_TOP_LOGPROBS_MAX + e * 64 + lane] = -INFINITY;
            s_ti[wave * 32 * CW_TOP_LOGPROBS_MAX + e * 64 + lane] = 0x7fffffff;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) { kv[q] = -INFINITY; ki[q] = 0x7fffffff; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    const bf16_t* a0 = A + (size_t)(m0 + l15) * K + g * 8;
    const bf16_t* a1 = a0 + (size_t)16 * K;
    for (int t0 = t_begin; t0 < t_end; t0 += 4) {
        // STOP: does any of the four tiles' columns lie in S (the same answer in every lane: most tile groups skip the pair)
        const bool stop_here = STOP && ((eos >= t0 * 16 && eos < (t0 + 4) * 16) || (t0 + 4) * 16 > ts_begin);
        f32x4_t acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        bool tv[4];
        const bf16_t* wp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tv[j] = t0 + j < t_end;
            wp[j] = W + ((size_t)(tv[j] ? t0 + j : t0) * KS * 64 + lane) * 8;
        }
        for (int s = 0; s < KS; ++s) {
            bf16x8_t a[2], b[4];
            a[0] = mv[0] ? *(const bf16x8_t*)(a0 + s * 32) : zero;
            a[1] = mv[1] ? *(const bf16x8_t*)(a1 + s * 32) : zero;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const bf16x8_t*)(wp[j] + (size_t)s * 512);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = cw_mfma_16x16x32(a[i], b[j], acc[i][j]);
        }
        if (STORE) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int m = m0 + (q >> 2) * 16 + g * 4 + (q & 3);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = (t0 + j) * 16 + l15;
                    if (tv[j] && n < V && m < M) logits[(size_t)m * ldv + n] = acc[q >> 2][j][q & 3];
                }
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = q >> 2, r = q & 3;
            float v[4];
            float mnew = mx[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = (t0 + j) * 16 + l15;
                const bool ok = tv[j] && n < V;
                v[j] = ok ? acc[i][j][r] : -INFINITY;
                mnew = fmaxf(mnew, v[j]);
                if (ok && n == tg[q]) tl[q] = v[j];
                if (ok && v[j] > bv[q]) { bv[q] = v[j]; bi[q] = n; }          // columns ascend within a lane: strict > keeps the lowest id
            }
            if constexpr (ENT) {
#pragma unroll
                for (int j = 0; j < 4; ++j) nanrow |= (v[j] != v[j]) ? 1u << q : 0u;
                if (mnew > -INFINITY) {
                    float add = 0.f, addz = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float d = v[j] - mnew, e = v[j] > -INFINITY ? expf(d) : 0.f;
                        add += e;
                        addz += v[j] > -INFINITY ? e * d : 0.f;
                    }
                    const float d0 = mx[q] - mnew, e0 = expf(d0);
                    zc[q] = (mx[q] > -INFINITY ? (zc[q] + sum[q] * d0) * e0 : 0.f) + addz;
                    sum[q] = (mx[q] > -INFINITY ? sum[q] * e0 : 0.f) + add;
                    mx[q] = mnew;
                }
            } else if (mnew > -INFINITY) {
                float add = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) add += v[j] > -INFINITY ? expf(v[j] - mnew) : 0.f;
                sum[q] = (mx[q] > -INFINITY ? sum[q] * expf(mx[q] - mnew) : 0.f) + add;
                mx[q] = mnew;
            }
            if (TOPK) {
                const int lrow = (wave * 32 + i * 16 + g * 4 + r) * CW_TOP_LOGPROBS_MAX;
                const int last = lrow + topk - 1;
                const bool row_ok = m0 + i * 16 + g * 4 + r < M;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = (t0 + j) * 16 + l15;
                    // v is -inf already for a padding column, and a NaN passes no comparison.  The full order, not the value
                    // alone: the 16 lanes of a row do not meet the ids of a tile group in ascending order.
                    const bool offer = row_ok && v[j] > -INFINITY && score_better(v[j], n, kv[q], ki[q]);
                    unsigned long long pend = __ballot(offer);
                    if (pend == 0) continue;
                    while (pend) {                                            // (the same in every lane)
                        const unsigned grp = (unsigned)(pend >> (g * 16)) & 0xffffu;
                        if (grp != 0 && l15 == __ffs(grp) - 1 && score_better(v[j], n, s_tv[last], s_ti[last])) {
                            int p = topk - 1;                                 // the list's last pair leaves; shift until v fits
                            while (p > 0) {
                                const float pv = s_tv[lrow + p - 1];
                                const int pi = s_ti[lrow + p - 1];
                                if (!score_better(v[j], n, pv, pi)) break;
                                s_tv[lrow + p] = pv; s_ti[lrow + p] = pi;
                                --p;
                            }
                            s_tv[lrow + p] = v[j]; s_ti[lrow + p] = n;
                        }
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        unsigned long long rest = 0;                          // every group's lowest offer is served
#pragma unroll
                        for (int gg = 0; gg < 4; ++gg) {
                            unsigned f = (unsigned)(pend >> (gg * 16)) & 0xffffu;
                            f &= f - 1;
                            rest |= (unsigned long long)f << (gg * 16);
                        }
                        pend = rest;
                    }
                    kv[q] = s_tv[last]; ki[q] = s_ti[last];
                }
            }
            if (STOP && stop_here) {
                float sv[4];
                float snew = smx[q];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = (t0 + j) * 16 + l15;
                    sv[j] = (n == eos || n >= ts_begin) ? v[j] : -INFINITY;   // v is -inf already for columns >= V
                    snew = fmaxf(snew, sv[j]);
                }
                if (snew > -INFINITY) {
                    float add = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) add += sv[j] > -INFINITY ? expf(sv[j] - snew) : 0.f;
                    ssum[q] = (smx[q] > -INFINITY ? ssum[q] * expf(smx[q] - snew) : 0.f) + add;
                    smx[q] = snew;
                }
            }
        }
    }
    if (STORE) return;
    // the 16 lanes (l15) of a row
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const float omx = __shfl_xor(mx[q], off, 64), osum = __shfl_xor(sum[q], off, 64), otl = __shfl_xor(tl[q], off, 64);
            const float obv = __shfl_xor(bv[q], off, 64);
            const int obi = __shfl_xor(bi[q], off, 64);
            const float mnew = fmaxf(mx[q], omx);
            if constexpr (ENT) {                                              // before sum and mx move
                const float ozc = __shfl_xor(zc[q], off, 64);
                if (mnew > -INFINITY)
                    zc[q] = (mx[q] > -INFINITY ? score_recentre(zc[q], sum[q], mx[q] - mnew) : 0.f) +
                            (omx > -INFINITY ? score_recentre(ozc, osum, omx - mnew) : 0.f);
            }
            if (mnew > -INFINITY)
                sum[q] = (mx[q] > -INFINITY ? sum[q] * expf(mx[q] - mnew) : 0.f) + (omx > -INFINITY ? osum * expf(omx - mnew) : 0.f);
            mx[q] = mnew;
            tl[q] = fmaxf(tl[q], otl);                                        // at most one lane holds the target's column
            if (score_better(obv, obi, bv[q], bi[q])) { bv[q] = obv; bi[q] = obi; }
            if (STOP) {
                const float osmx = __shfl_xor(smx[q], off, 64), ossum = __shfl_xor(ssum[q], off, 64);
                const float snew = fmaxf(smx[q], osmx);
                if (snew > -INFINITY)
                    ssum[q] = (smx[q] > -INFINITY ? ssum[q] * expf(smx[q] - snew) : 0.f) +
                              (osmx > -INFINITY ? ossum * expf(osmx - snew) : 0.f);
                smx[q] = snew;
            }
        }
        const int m = m0 + (q >> 2) * 16 + g * 4 + (q & 3);
        if constexpr (ENT) {
            bool bad = (nanrow >> q) & 1u;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) bad |= __shfl_xor((int)bad, off, 64) != 0;
            if (l15 == 0 && m < M) epart[(size_t)m * n_split + split] = bad ? __builtin_nanf("") : zc[q];
        }
        if (l15 == 0 && m < M) {
            ScorePart p;
            p.mx = mx[q]; p.sum = sum[q]; p.tl = tl[q]; p.bv = bv[q]; p.bi = bi[q];
            part[(size_t)m * n_split + split] = p;
            if (STOP) {
                ScoreStopPart sp;
                sp.mx = smx[q]; sp.sum = ssum[q];
                spart[(size_t)m * n_split + split] = sp;
            }
        }
        if (TOPK && l15 < CW_TOP_LOGPROBS_MAX && m < M) {                     // the row's list, padded with the identity
            const int e = (wave * 32 + (q >> 2) * 16 + g * 4 + (q & 3)) * CW_TOP_LOGPROBS_MAX + l15;
            ScoreTopPart tp;
            tp.v = s_tv[e]; tp.i = s_ti[e];
            tpart[((size_t)m * n_split + split) * CW_TOP_LOGPROBS_MAX + l15] = tp;
        }
    }
}

// one thread per row; STOP: stop_logprob[m] = logsumexp over S - logsumexp, -inf where no column of S exists
// TOPK: one wave per row instead (every lane runs the same merge of the statistics, lane 0 writes them), then topk selection
// rounds over the row's n_split x CW_TOP_LOGPROBS_MAX pairs: in each, the best pair behind the one the round before took --
// pairs are distinct (one per column), so "behind" needs no marks.  alt_id / alt_logprob [M][CW_TOP_LOGPROBS_MAX]: z - lse with
// the lse logprob is written with; -1 / NaN at the ranks no candidate fills and at ranks >= topk.
// ENT: entropy[m] from the splits' (mx, sum, Zc) moved to the row maximum in split order
template <bool STOP, bool TOPK = false, bool ENT = false>
__global__ __launch_bounds__(256) void score_combine_kernel(const ScorePart* __restrict__ part, int M, int n_split,
                                                            float* __restrict__ logprob, int* __restrict__ top_id,
                                                            float* __restrict__ top_logprob,
                                                            const ScoreStopPart* __restrict__ spart,
                                                            float* __restrict__ stop_logprob,
                                                            const ScoreTopPart* __restrict__ tpart, int topk,
                                                            int* __restrict__ alt_id, float* __restrict__ alt_logprob,
                                                            const float* __restrict__ epart, float* __restrict__ entropy) {
    const int m = TOPK ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const bool writer = !TOPK || (threadIdx.x & 63) == 0;
    const ScorePart* p = part + (size_t)m * n_split;
    float mx = -INFINITY, tl = -INFINITY, bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int s = 0; s < n_split; ++s) {
        mx = fmaxf(mx, p[s].mx);
        tl = fmaxf(tl, p[s].tl);
        if (score_better(p[s].bv, p[s].bi, bv, bi)) { bv = p[s].bv; bi = p[s].bi; }
    }
    float sum = 0.f;
    for (int s = 0; s < n_split; ++s)
        if (p[s].mx > -INFINITY) sum += p[s].sum * expf(p[s].mx - mx);
    const float lse = mx + logf(sum);
    if (writer) {
        logprob[m] = tl - lse;
        top_id[m] = bi;
        top_logprob[m] = bv - lse;
    }
    if constexpr (ENT) {
        const float* ep = epart + (size_t)m * n_split;
        float z = 0.f;
        for (int s = 0; s < n_split; ++s) z += p[s].mx > -INFINITY ? score_recentre(ep[s], p[s].sum, p[s].mx - mx) : ep[s];
        if (writer) entropy[m] = score_entropy(sum, z);
    }
    if (STOP) {
        const ScoreStopPart* sp = spart + (size_t)m * n_split;
        float smx = -INFINITY;
        for (int s = 0; s < n_split; ++s) smx = fmaxf(smx, sp[s].mx);
        float ssum = 0.f;
        for (int s = 0; s < n_split; ++s)
            if (sp[s].mx > -INFINITY) ssum += sp[s].sum * expf(sp[s].mx - smx);
        if (writer) stop_logprob[m] = smx > -INFINITY ? (smx + logf(ssum)) - lse : -INFINITY;
    }
    if (TOPK) {
        const int lane = threadIdx.x & 63, n_pairs = n_split * CW_TOP_LOGPROBS_MAX;
        const ScoreTopPart* tp = tpart + (size_t)m * n_pairs;
        float pv = INFINITY;                                                  // the pair the round before took
        int pi = -1;
        for (int j = 0; j < CW_TOP_LOGPROBS_MAX; ++j) {
            float cv = -INFINITY;
            int ci = 0x7fffffff;
            if (j < topk) {
                for (int e = lane; e < n_pairs; e += 64) {
                    const ScoreTopPart c = tp[e];
                    if (c.v > -INFINITY && score_better(pv, pi, c.v, c.i) && score_better(c.v, c.i, cv, ci)) { cv = c.v; ci = c.i; }
                }
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov = __shfl_xor(cv, o, 64);
                    const int oi = __shfl_xor(ci, o, 64);
                    if (score_better(ov, oi, cv, ci)) { cv = ov; ci = oi; }
                }
            }
            const bool any = cv > -INFINITY;
            if (lane == 0) {
                alt_id[(size_t)m * CW_TOP_LOGPROBS_MAX + j] = any ? ci : -1;
                alt_logprob[(size_t)m * CW_TOP_LOGPROBS_MAX + j] = any ? cv - lse : __builtin_nanf("");
            }
            if (any) { pv = cv; pi = ci; } else { pv = -INFINITY; pi = -1; }     // no candidate left: none in later rounds either
        }
    }
}

// one block per row of f32 logits [rows][ldv]; target[row * t_stride + t] (negative: no target, the row's logprob is -inf);
// results at out[row * t_stride + t].  STOP: stop_logprob likewise, from a second (maximum, sum) pass over the columns of S
// TOPK: topk block-wide selection rounds over the same row behind that, each taking the best (logit, id) behind the pair of the
// round before; alt_id / alt_logprob [rows][t_stride][CW_TOP_LOGPROBS_MAX] = logit - lse with the lse above, -1 / NaN at the
// ranks no candidate fills (a candidate is a column < V with a logit > -inf; a NaN is none) and at ranks >= topk
// ENT: entropy likewise, from sum exp(x - max) (x - max) beside the sum above (a -inf column adds nothing, a NaN makes it NaN)
template <bool STOP, bool TOPK = false, bool ENT = false>
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ logits, int ldv, int V,
                                                         const int* __restrict__ target, int t_stride, int t,
                                                         float* __restrict__ logprob, int* __restrict__ top_id,
                                                         float* __restrict__ top_logprob, int eos, int ts_begin,
                                                         float* __restrict__ stop_logprob, int topk,
                                                         int* __restrict__ alt_id, float* __restrict__ alt_logprob,
                                                         float* __restrict__ entropy) {
    __shared__ float s_v[4], s_s[4], s_sv[4], s_ss[4], s_z[4];
    __shared__ int s_i[4];
    __shared__ float s_lse, s_cv[2][4];                                       // TOPK only: rounds alternate between two slots
    __shared__ int s_ci[2][4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lg = logits + (size_t)row * ldv;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int n = tid; n < V; n += 256)
        if (lg[n] > bv) { bv = lg[n]; bi = n; }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (score_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
    __syncthreads();
    bv = s_v[0]; bi = s_i[0];
    for (int w = 1; w < 4; ++w)
        if (score_better(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
    float sum = 0.f;
    if constexpr (ENT) {
        float z = 0.f;
        for (int n = tid; n < V; n += 256) {
            const float d = lg[n] - bv, e = expf(d);
            sum += e;
            z += d > -INFINITY ? e * d : 0.f;                                 // (a NaN d is in sum already)
        }
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if (lane == 0) s_z[wave] = z;
    } else {
        for (int n = tid; n < V; n += 256) sum += expf(lg[n] - bv);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) s_s[wave] = sum;
    float smx = -INFINITY;
    if (STOP) {
        for (int n = tid; n < V; n += 256)
            if (n == eos || n >= ts_begin) smx = fmaxf(smx, lg[n]);
        for (int o = 32; o > 0; o >>= 1) smx = fmaxf(smx, __shfl_xor(smx, o, 64));
        if (lane == 0) s_sv[wave] = smx;
    }
    __syncthreads();
    if (STOP) {
        smx = fmaxf(fmaxf(s_sv[0], s_sv[1]), fmaxf(s_sv[2], s_sv[3]));
        float ssum = 0.f;
        if (smx > -INFINITY)
            for (int n = tid; n < V; n += 256)
                if (n == eos || n >= ts_begin) ssum += expf(lg[n] - smx);
        for (int o = 32; o > 0; o >>= 1) ssum += __shfl_xor(ssum, o, 64);
        if (lane == 0) s_ss[wave] = ssum;
        __syncthreads();
    }
    if (tid == 0) {
        const float lse = bv + logf((s_s[0] + s_s[1]) + (s_s[2] + s_s[3]));
        const size_t o = (size_t)row * t_stride + t;
        const int tg = target[o];
        logprob[o] = (tg >= 0 && tg < V) ? lg[tg] - lse : -INFINITY;
        top_id[o] = bi;
        top_logprob[o] = bv - lse;
        if (STOP)
            stop_logprob[o] = smx > -INFINITY ? (smx + logf((s_ss[0] + s_ss[1]) + (s_ss[2] + s_ss[3]))) - lse : -INFINITY;
        if (TOPK) s_lse = lse;
        if constexpr (ENT) entropy[o] = score_entropy((s_s[0] + s_s[1]) + (s_s[2] + s_s[3]), (s_z[0] + s_z[1]) + (s_z[2] + s_z[3]));
    }
    if (TOPK) {
        float pv = INFINITY;                                                  // the pair the round before took
        int pi = -1;
        const size_t o = ((size_t)row * t_stride + t) * CW_TOP_LOGPROBS_MAX;
        for (int j = 0; j < topk; ++j) {
            float cv = -INFINITY;
            int ci = 0x7fffffff;
            for (int n = tid; n < V; n += 256) {
                const float x = lg[n];
                if (x > -INFINITY && score_better(pv, pi, x, n) && score_better(x, n, cv, ci)) { cv = x; ci = n; }
            }
            for (int of = 32; of > 0; of >>= 1) {
                const float ov = __shfl_xor(cv, of, 64);
                const int oi = __shfl_xor(ci, of, 64);
                if (score_better(ov, oi, cv, ci)) { cv = ov; ci = oi; }
            }
            if (lane == 0) { s_cv[j & 1][wave] = cv; s_ci[j & 1][wave] = ci; }
            __syncthreads();                                                  // (the first one also publishes s_lse)
            cv = s_cv[j & 1][0]; ci = s_ci[j & 1][0];
            for (int w = 1; w < 4; ++w)
                if (score_better(s_cv[j & 1][w], s_ci[j & 1][w], cv, ci)) { cv = s_cv[j & 1][w]; ci = s_ci[j & 1][w]; }
            const bool any = cv > -INFINITY;
            if (tid == 0) {
                alt_id[o + j] = any ? ci : -1;
                alt_logprob[o + j] = any ? cv - s_lse : __builtin_nanf("");
            }
            if (any) { pv = cv; pi = ci; } else { pv = -INFINITY; pi = -1; }
        }
        if (tid >= topk && tid < CW_TOP_LOGPROBS_MAX) { alt_id[o + tid] = -1; alt_logprob[o + tid] = __builtin_nanf(""); }
    }
}

int cw_launch_score_ln(const float* x, const int* src, const float* g, const float* b, void* out, int M, int D, hipStream_t st) {
    if (M < 1 || D < 1) return CW_ERR_INVALID;
    hipLaunchKernelGGL(score_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, st, x, src, g, b, (bf16_t*)out, M, D);
    return CW_OK;
}

// Vocabulary splits for M rows: about two blocks per compute unit over all m-tiles, four 16-column tiles at least per split
int cw_score_head_splits(int M, int V, int* tiles_per_split) {
    const int NT = (V + 15) / 16, mt = (M + 127) / 128;
    int ns = 512 / mt;
    ns = ns < 1 ? 1 : (ns > 256 ? 256 : ns);
    int tps = ((NT + ns - 1) / ns + 3) & ~3;
    if (tiles_per_split) *tiles_per_split = tps;
    return (NT + tps - 1) / tps;
}

// One form of the fused head: the split kernel and its combine.  The arguments of a form that is off are null / 0.
template <bool STOP, bool TOPK, bool ENT = false>
static void score_head_form(const void* A, const void* W, const int* target, int M, int V, int K, const ScoreHeadOut& o, hipStream_t st) {
    int tps = 0;
    const int ns = cw_score_head_splits(M, V, &tps);
    ScoreStopPart* const spart = STOP ? o.spart : nullptr;
    ScoreTopPart* const tpart = TOPK ? o.tpart : nullptr;
    float* const epart = ENT ? o.epart : nullptr;
    hipLaunchKernelGGL((score_head_kernel<false, STOP, TOPK, ENT>), dim3((M + 127) / 128, ns), dim3(256), 0, st, (const bf16_t*)A,
                       (const bf16_t*)W, target, o.part, M, V, K, tps, ns, (float*)nullptr, 0, spart, STOP ? o.eos : 0, STOP ? o.ts_begin : 0,
                       tpart, TOPK ? o.k : 0, epart);
    hipLaunchKernelGGL((score_combine_kernel<STOP, TOPK, ENT>), dim3(TOPK ? (M + 3) / 4 : (M + 255) / 256), dim3(256), 0, st, o.part, M, ns,
                       o.logprob, o.top_id, o.top_logprob, (const ScoreStopPart*)spart, STOP ? o.stop_logprob : nullptr,
                       (const ScoreTopPart*)tpart, TOPK ? o.k : 0, TOPK ? o.alt_id : nullptr, TOPK ? o.alt_logprob : nullptr,
                       (const float*)epart, ENT ? o.entropy : nullptr);
}
// ... and of the row kernel
template <bool STOP, bool TOPK, bool ENT = false>
static void score_rows_form(const float* logits, int ldv, int V, const int* target, int t_stride, int t, int rows, const ScoreRowsOut& o,
                            hipStream_t st) {
    hipLaunchKernelGGL((score_rows_kernel<STOP, TOPK, ENT>), dim3(rows), dim3(256), 0, st, logits, ldv, V, target, t_stride, t, o.logprob,
                       o.top_id, o.top_logprob, STOP ? o.eos : 0, STOP ? o.ts_begin : 0, STOP ? o.stop_logprob : nullptr, TOPK ? o.k : 0,
                       TOPK ? o.alt_id : nullptr, TOPK ? o.alt_logprob : nullptr, ENT ? o.entropy : nullptr);
}

// The code object holds the kernels in the order their instantiations are first asked for.  The forms are asked for here, around
// the unfused launcher, in the order every build so far has held them, so that the device code of a change to the launchers
// compares equal with its parent's.  The ENT forms come last.
#define CW_SCORE_HEAD_FORM(...) \
    template void score_head_form<__VA_ARGS__>(const void*, const void*, const int*, int, int, int, const ScoreHeadOut&, hipStream_t)
#define CW_SCORE_ROWS_FORM(...) \
    template void score_rows_form<__VA_ARGS__>(const float*, int, int, const int*, int, int, int, const ScoreRowsOut&, hipStream_t)
CW_SCORE_HEAD_FORM(false, false);
CW_SCORE_HEAD_FORM(true, false);

// the unfused form of cw_launch_score_head: f32 logits [M][ldv] (ldv >= V) through the same GEMM, then a row-wise pass
int cw_launch_score_head_unfused(const void* A, const void* W, const int* target, float* logits, int ldv, int M, int V, int K,
                                 float* logprob, int* top_id, float* top_logprob, hipStream_t st) {
    if (M < 1 || V < 1 || ldv < V || K < 32 || K % 32) return CW_ERR_INVALID;
    int tps = 0;
    const int ns = cw_score_head_splits(M, V, &tps);
    hipLaunchKernelGGL((score_head_kernel<true, false>), dim3((M + 127) / 128, ns), dim3(256), 0, st, (const bf16_t*)A,
                       (const bf16_t*)W, target, (ScorePart*)nullptr, M, V, K, tps, ns, logits, ldv, (ScoreStopPart*)nullptr, 0, 0, (ScoreTopPart*)nullptr, 0,
                       (float*)nullptr);
    hipLaunchKernelGGL(score_rows_kernel<false>, dim3(M), dim3(256), 0, st, (const float*)logits, ldv, V, target, 1, 0, logprob,
                       top_id, top_logprob, 0, 0, (float*)nullptr, 0, (int*)nullptr, (float*)nullptr, (float*)nullptr);
    return CW_OK;
}

CW_SCORE_ROWS_FORM(false, false);
CW_SCORE_ROWS_FORM(true, false);
CW_SCORE_HEAD_FORM(false, true);
CW_SCORE_HEAD_FORM(true, true);
CW_SCORE_ROWS_FORM(false, true);
CW_SCORE_ROWS_FORM(true, true);
CW_SCORE_HEAD_FORM(false, false, true);
CW_SCORE_HEAD_FORM(true, false, true);
CW_SCORE_HEAD_FORM(false, true, true);
CW_SCORE_HEAD_FORM(true, true, true);
CW_SCORE_ROWS_FORM(false, false, true);
CW_SCORE_ROWS_FORM(true, false, true);
CW_SCORE_ROWS_FORM(false, true, true);
CW_SCORE_ROWS_FORM(true, true, true);
#undef CW_SCORE_HEAD_FORM
#undef CW_SCORE_ROWS_FORM

// The fused head over M rows (kernels.h: ScoreHeadOut).  This and cw_launch_score_rows pick among the STOP / TOPK / ENT forms
template <bool ENT>
static void score_head_pick(bool stop, bool top, const void* A, const void* W, const int* target, int M, int V, int K, const ScoreHeadOut& o, hipStream_t st) {
    if (top) stop ? score_head_form<true, true, ENT>(A, W, target, M, V, K, o, st) : score_head_form<false, true, ENT>(A, W, target, M, V, K, o, st);
    else stop ? score_head_form<true, false, ENT>(A, W, target, M, V, K, o, st) : score_head_form<false, false, ENT>(A, W, target, M, V, K, o, st);
}
int cw_launch_score_head(const void* A, const void* W, const int* target, int M, int V, int K, const ScoreHeadOut& o, hipStream_t st) {
    const bool stop = o.stop_logprob != nullptr, top = o.k != 0, ent = o.entropy != nullptr;
    if (M < 1 || V < 1 || K < 32 || K % 32 || (stop && (o.eos < 0 || o.ts_begin < 0)) || (ent && !o.epart) ||
        (top && (o.k < 1 || o.k > CW_TOP_LOGPROBS_MAX || !o.tpart || !o.alt_id || !o.alt_logprob))) return CW_ERR_INVALID;
    if (ent) score_head_pick<true>(stop, top, A, W, target, M, V, K, o, st);
    else score_head_pick<false>(stop, top, A, W, target, M, V, K, o, st);
    return CW_OK;
}

// the GEMM of cw_launch_score_head_unfused alone: f32 logits [M][ldv] (the accumulators the fused forms reduce)
int cw_launch_score_head_store(const void* A, const void* W, const int* target, float* logits, int ldv, int M, int V, int K, hipStream_t st) {
    if (M < 1 || V < 1 || ldv < V || K < 32 || K % 32 || !logits) return CW_ERR_INVALID;
    int tps = 0;
    const int ns = cw_score_head_splits(M, V, &tps);
    hipLaunchKernelGGL((score_head_kernel<true, false>), dim3((M + 127) / 128, ns), dim3(256), 0, st, (const bf16_t*)A,
                       (const bf16_t*)W, target, (ScorePart*)nullptr, M, V, K, tps, ns, logits, ldv,
                       (ScoreStopPart*)nullptr, 0, 0, (ScoreTopPart*)nullptr, 0, (float*)nullptr);
    return CW_OK;
}

// The loop path's row kernel at column t of [rows][t_stride] outputs (alternatives: [rows][t_stride][CW_TOP_LOGPROBS_MAX])
template <bool ENT>
static void score_rows_pick(bool stop, bool top, const float* logits, int ldv, int V, const int* target, int t_stride, int t, int rows,
                            const ScoreRowsOut& o, hipStream_t st) {
    if (top) stop ? score_rows_form<true, true, ENT>(logits, ldv, V, target, t_stride, t, rows, o, st) : score_rows_form<false, true, ENT>(logits, ldv, V, target, t_stride, t, rows, o, st);
    else stop ? score_rows_form<true, false, ENT>(logits, ldv, V, target, t_stride, t, rows, o, st) : score_rows_form<false, false, ENT>(logits, ldv, V, target, t_stride, t, rows, o, st);
}
int cw_launch_score_rows(const float* logits, int ldv, int V, const int* target, int t_stride, int t, int rows, const ScoreRowsOut& o,
                         hipStream_t st) {
    const bool stop = o.stop_logprob != nullptr, top = o.k != 0, ent = o.entropy != nullptr;
    if (rows < 1 || V < 1 || ldv < V || t < 0 || t >= t_stride || (stop && (o.eos < 0 || o.ts_begin < 0)) ||
        (top && (o.k < 1 || o.k > CW_TOP_LOGPROBS_MAX || !o.alt_id || !o.alt_logprob))) return CW_ERR_INVALID;
    if (ent) score_rows_pick<true>(stop, top, logits, ldv, V, target, t_stride, t, rows, o, st);
    else score_rows_pick<false>(stop, top, logits, ldv, V, target, t_stride, t, rows, o, st);
    return CW_OK;
}

}  // namespace CW_NS
