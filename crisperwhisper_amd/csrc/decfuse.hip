// Six-launch decoder layer of the 16-bit engine (batch rows <= 16; 17..64 greedy rows run the same stage in groups of 16 rows,
// gemv_stack_kernel's grid y, inside their ten-launch layer): LayerNorm is linear up to two per-row scalars,
//     W LN(x) = rstd * (W' x - mean * (W' 1)) + b',      W' = W diag(gamma),  b' = b + W beta,
// so a projection that follows "residual add -> LayerNorm" can be applied to the *summands* of the residual before
// the statistics exist, and the statistics are applied by the consumer.  With x1 = x + Wo a + bo (self-attention
// out-projection, TF modeling_whisper.py:471-476) and q_c = Wq_c LN_c(x1) (:485-493)
//     q_c = rstd(x1) * ( W'q_c x + (W'q_c Wo) a + W'q_c bo - mean(x1) * (W'q_c 1) ) + b'q_c
// the two dependent GEMVs "out-projection" and "cross-attention query" become ONE stage over the stacked matrix
// [W'q_c ; W'q_c Wo ; Wo] (inputs x, a, a), and in the same way cross-attention out-projection + fc1 (:498-502) become one
// stage over [W'1 ; W'1 Wo_c ; Wo_c].  The product matrices are formed once at weight-load time in f32
// (fold_product_kernel) and rounded to the engine's 16-bit type once.  A decoder layer is then 6 dependent launches
// instead of 8:  qkv | self-attention | X1 | cross-attention (finishes q_c) | X2 | fc2 (finishes gelu(fc1)).
// Cost: the product matrices add 16.4 MB of weight stream per layer at large-v3 (56.6 -> 73 MB); what it buys is two
// launch boundaries + kernel ramps per layer on a chain that is latency-bound.
//
//   fold_product_kernel / fold_rowvec_kernel   load-time: C = (A diag(s) scale) B in f32 -> 16 bit;  c = A' v,  w = W16 1
//   gemv_stack_kernel    one launch over a row-stacked weight matrix: up to 3 segments, each with its own f32 input rows
//                        and epilogue (plain store, or residual add on the 2^-12 grid into a second buffer); NT 16-column
//                        tiles per block share the activation rows; same weight streaming as gemv2_bf16_kernel (gemm.hip)
//   gemv_fc2x_kernel     fc2 whose activation load finishes fc1: mid = gelu(rstd (u_a + u_b - mean w1) + b1') from the two
//                        partial projections and the LayerNorm statistics of the residual row it computes wave-locally
#include "common.h"
#include "kernels.h"

namespace CW_NS {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
__device__ static inline f32x4_t mfma16x(bf16x8_t a, bf16x8_t b, f32x4_t c) { return cw_mfma_16x16x32(a, b, c); }

// ---------------------------------------------------------------------------------------------------
// load-time products (f32 VALU, 64 x 64 output tile per block, run once per checkpoint)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_product_kernel(const float* __restrict__ A, const float* __restrict__ s,
                                                           float scale, const float* __restrict__ B, int N, int J, int K,
                                                           bf16_t* __restrict__ C) {
    __shared__ float As[16][65];
    __shared__ float Bs[16][64];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
    float acc[4][4] = {};
    for (int j0 = 0; j0 < J; j0 += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            const int n = idx >> 4, j = idx & 15;
            As[j][n] = A[(size_t)(n0 + n) * J + j0 + j] * (s ? s[j0 + j] : 1.0f) * scale;
            const int jb = idx >> 6, k = idx & 63;
            Bs[jb][k] = B[(size_t)(j0 + jb) * K + k0 + k];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[j][ty * 4 + i]; b[i] = Bs[j][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[i][jj] = fmaf(a[i], b[jj], acc[i][jj]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) C[(size_t)(n0 + ty * 4 + i) * K + k0 + tx * 4 + jj] = f32_to_bf16(acc[i][jj]);
}

// one wave per output row n:  c[n] = sum_j A[n][j] s[j] scale v[j]  (f32; optional),  w[n] = sum_j float(W16[n][j])
__global__ __launch_bounds__(256) void fold_rowvec_kernel(const float* __restrict__ A, const float* __restrict__ s, float scale,
                                                          const float* __restrict__ v, const bf16_t* __restrict__ W16, int N,
                                                          int J, float* __restrict__ c_out, float* __restrict__ w_out) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float c = 0.f, w = 0.f;
    for (int j = lane; j < J; j += 64) {
        if (c_out) c = fmaf(A[(size_t)n * J + j] * (s ? s[j] : 1.0f) * scale, v[j], c);
        if (w_out) w += bf16_to_f32(W16[(size_t)n * J + j]);
    }
    c = wave_sum(c);
    w = wave_sum(w);
    if (lane == 0) {
        if (c_out) c_out[n] = c;
        if (w_out) w_out[n] = w;
    }
}

int cw_launch_fold_product(const float* A, const float* s, float scale, const float* B, int N, int J, int K, void* C16,
                           hipStream_t st) {
    if (N % 64 || K % 64 || J % 16) return CW_ERR_INVALID;
    hipLaunchKernelGGL(fold_product_kernel, dim3(K / 64, N / 64), dim3(256), 0, st, A, s, scale, B, N, J, K, (bf16_t*)C16);
    return CW_OK;
}
int cw_launch_fold_rowvec(const float* A, const float* s, float scale, const float* v, const void* W16, int N, int J,
                          float* c_out, float* w_out, hipStream_t st) {
    hipLaunchKernelGGL(fold_rowvec_kernel, dim3((N + 3) / 4), dim3(256), 0, st, A, s, scale, v, (const bf16_t*)W16, N, J,
                       c_out, w_out);
    return CW_OK;
}

// ---------------------------------------------------------------------------------------------------
// gemv_stack_kernel: Mb <= 16 rows, K <= 1280 (one K slice per block), up to NT column tiles per block (per segment).
// Structure and MFMA fragment conventions are those of gemv2_bf16_kernel (gemm.hip): unconditional clamped loads, a row of
// activations lives in one wave, weights go straight from HBM into B fragments, cross-wave reduction through LDS.
// ---------------------------------------------------------------------------------------------------

// UNI (round 6): every segment streams NT tiles per block from fragment-major weights -- the shape of every launch of the default
// engine.  The weight requests then sit under no branch (`t < snt` and `wpk` are run-time values otherwise: hipcc wraps each tile's
// loads in a block-uniform branch and must answer the first wait behind them with vmcnt(0)).  Same arithmetic.
// WNT (with UNI): the weight stream with non-temporal loads -- launches of one row group (gridDim.y == 1), where every tile is read by
// exactly one block; the 16-row groups of 17..64 rows re-read the tiles from L2 (below) and keep the default policy.
// Kernel arguments (DESIGN.md 6g''): five plain values of 7 dwords lead -- preloaded into user SGPRs at dispatch by the file's
// -amdgpu-kernarg-preload-count -- and they decide the block's segment: W, the buffer to clear, dims = p.K | p.Mb << 16 | p.nseg << 24 |
// (p.wpk != 0) << 26, blocks12 = seg[1].block0 | seg[2].block0 << 16.  The segment's fields then come as ONE batch of scalar loads at
// a block-uniform offset into `p` (two kernarg lines, one wait) instead of a first round for the block starts and a second for the
// picked segment; twelve pointers of three segments do not fit the 14 preloadable dwords, so the requests of this kernel still
// wait for that one round.  A by-value struct is never preloaded and ends the preloaded run: keep the order.
template <int RPW, int NSLOT, int PER_LANE, int NT, bool UNI = false, bool WNT = false>
__global__ __launch_bounds__(256) void gemv_stack_kernel(const void* __restrict__ Wp, float* zero, int zero_n4, unsigned dims, unsigned blocks12, StackParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    // 17..64 rows (round 5): blockIdx.y = group of 16 rows; a group is a 16-row launch of its own over the same weights (its
    // blocks follow the first group's on the same XCD: 240 % 8 == 0, so the tile's weights come out of that L2 from the second
    // group on), per-row arithmetic unchanged -- rows m0 .. m0 + 15 of every operand, pstats one plane per group
    const int K = (int)(dims & 0xffffu), nseg = (int)((dims >> 24) & 3u), m0 = blockIdx.y * 16, Mb = min(16, (int)((dims >> 16) & 0xffu) - m0);
    const int xs_stride = K + 8;
    bf16_t* xs = (bf16_t*)smem_s;                               // [16][K+8]
    float* red = (float*)(smem_s + (size_t)16 * xs_stride * 2);  // [4 waves][NT][4][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int bid = blockIdx.x;
    int si = 0;                                                  // block-uniform segment
    if (nseg > 1 && bid >= (int)(blocks12 & 0xffffu)) si = 1;
    if (nseg > 2 && bid >= (int)(blocks12 >> 16)) si = 2;
    const StackSeg& sg = p.seg[si];                              // ONE batch of scalar loads at a block-uniform offset
    const float* __restrict__ x = sg.x + (size_t)m0 * K;
    const float* __restrict__ bias = sg.bias;
    const int tile0 = sg.tile0, n_tiles = sg.n_tiles, block0 = sg.block0, snt = sg.nt;
    const int steps = K >> 7, nvec = K >> 2;
    const int tl0 = (bid - block0) * snt;                        // first tile of this block inside the segment
    const bf16_t* __restrict__ W = (const bf16_t*)Wp;

    if (zero && blockIdx.y == 0) {                               // clear a buffer that a later launch accumulates into
        const int zi = bid * 256 + tid;
        if (zi < zero_n4) ((float4*)zero)[zi] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float* __restrict__ wsum = sg.wsum;
    float* smean = red + 4 * NT * 4 * 64;                       // [16] row means (segments with wsum)
    int nloc[NT];                                                // this lane's output column inside the segment (or -1)
    float bias_v[NT], wsum_v[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tl = tl0 + t;
        const bool ok = t < snt && tl < n_tiles;
        nloc[t] = ok ? tl * 16 + l15 : -1;
        const int ncl = (ok ? tl : n_tiles - 1) * 16 + l15;
        bias_v[t] = bias ? bias[ncl] : 0.f;
        wsum_v[t] = wsum ? wsum[ncl] : 0.f;
    }
    // the residual elements the x1 segment's epilogue adds to (epi == 1), requested at the head of the queue: at their use they are a
    // dependent load behind the MFMA loop -- an L2 round trip on the tail of the blocks that end the launch.  Unconditional (other
    // segments read an element of their own input instead: a load under a branch would make every later counted wait conservative)
    float resid_pre[NT];
    {
        const float* rsd = sg.resid;
        const int ldo_ = n_tiles * 16, mr = min(g * 4 + (tid >> 6), Mb - 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int nl = nloc[t] >= 0 ? nloc[t] : 0;
            const float* rp = rsd ? rsd + (size_t)(m0 + mr) * ldo_ + nl : x;
            resid_pre[t] = *rp;
        }
    }
    // activation rows -> registers
    float4 xv[RPW][PER_LANE];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        int row = wave + 4 * i;
        row = row < Mb ? row : Mb - 1;
#pragma unroll
        for (int c = 0; c < PER_LANE; ++c) {
            int v4 = lane + 64 * c;
            v4 = v4 < nvec ? v4 : nvec - 1;
            xv[i][c] = *(const float4*)(x + (size_t)row * K + v4 * 4);
        }
    }
    // weight stream: steps wave, wave+4, wave+8 (clamped: a tail wave re-reads a step another wave owns)
    u32x4_t wq[NT][NSLOT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (UNI || t < snt) {                                    // block-uniform: a lighter segment streams fewer tiles
            const int tl = tl0 + t < n_tiles ? tl0 + t : n_tiles - 1;
            const bf16_t* wrow = W + ((size_t)(tile0 + tl) * 16 + l15) * K + g * 8;
#pragma unroll
            for (int s = 0; s < NSLOT; ++s) {
                int step = wave + 4 * s;
                step = step < steps ? step : steps - 1;
                const bool wpk = UNI || ((dims >> 26) & 1u);
                const u32x4_t* wp = wpk ? (const u32x4_t*)(W + ((((size_t)(tile0 + tl) * (K >> 5)) + step * 4) * 64 + lane) * 8)
                                        : (const u32x4_t*)(wrow + step * 128);
                const int sj = wpk ? 64 : 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) wq[t][s][j] = WNT ? CW_STREAM_LD(wp + j * sj) : wp[j * sj];
            }
        } else {
#pragma unroll
            for (int s = 0; s < NSLOT; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) wq[t][s][j] = (u32x4_t){0u, 0u, 0u, 0u};
        }
    }
    // every load above is in flight before the first one is waited for: without the fence hipcc interleaves the weight loads
    // with the conversion of the activation rows as those return, which delays the weight stream by one L2 round trip
    __builtin_amdgcn_sched_barrier(0);
    // Rows that feed a LayerNorm consumer (W' x, the consumer applies rstd (. - mean W'1) + b'): rounding x itself to 16 bits
    // spends the significand on the row's mean, which the consumer subtracts again -- a factor sqrt(1 + mean^2 / var) on the
    // rounding noise of rows with an offset (outlier channels / drifting residual streams of trained checkpoints).  The row
    // lives in this wave, so its moments are a few DPP steps away: rows with |mean| >= std are rounded as x - mean and
    // mean * (W' 1) is added back in f32 in the epilogue.  Below that the factor is < 1.41 (half a bit) and the row is rounded
    // as it is: bit-identical to the uncentred stage, whose parity record the goldens hold (the rows of the synthetic models
    // sit at |mean| / std ~ 0.3-0.9, where the two roundings differ by noise only -- and that noise moves near-tie argmaxes).
    if (wsum) {                                                  // block-uniform
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            float sx = 0.f, sq = 0.f;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c)
                if (lane + 64 * c < nvec) {
                    sx += (xv[i][c].x + xv[i][c].y) + (xv[i][c].z + xv[i][c].w);
                    sq += cw_sumsq4(xv[i][c].x, xv[i][c].y, xv[i][c].z, xv[i][c].w);
                }
            float mu = wave_sum(sx) / (float)K;
            if (2.f * mu * mu < wave_sum(sq) / (float)K) mu = 0.f;    // |mean| < std  <=>  2 mean^2 < E[x^2]
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) { xv[i][c].x -= mu; xv[i][c].y -= mu; xv[i][c].z -= mu; xv[i][c].w -= mu; }
            if (lane == 0) smean[wave + 4 * i] = mu;
        }
    }
    // rows -> 16 bit -> LDS
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int row = wave + 4 * i;
#pragma unroll
        for (int c = 0; c < PER_LANE; ++c) {
            int v4 = lane + 64 * c;
            v4 = v4 < nvec ? v4 : nvec - 1;
            const float4 v = xv[i][c];
            ushort4 o;
            o.x = f32_to_bf16(v.x); o.y = f32_to_bf16(v.y); o.z = f32_to_bf16(v.z); o.w = f32_to_bf16(v.w);
            *(ushort4*)(xs + (size_t)row * xs_stride + v4 * 4) = o;
        }
    }
    __syncthreads();
    f32x4_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const int step = wave + 4 * s;
        if (step < steps) {
            const bf16_t* xr = xs + (size_t)l15 * xs_stride + step * 128 + g * 8;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = mfma16x(a, __builtin_bit_cast(bf16x8_t, wq[t][s][j]), acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((wave * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
    __syncthreads();
    const int epi = sg.epi;
    const int ldo = n_tiles * 16;
    float* __restrict__ out = sg.out + (size_t)m0 * ldo;
    float* __restrict__ out2 = sg.out2;
    if (out2) out2 += (size_t)m0 * ldo;
    const float* __restrict__ resid = sg.resid;
    if (resid) resid += (size_t)m0 * ldo;
    float* __restrict__ pstats = sg.pstats;
    if (pstats) pstats += (size_t)blockIdx.y * ((n_tiles + snt - 1) / snt) * 32;   // [group][blocks of the segment][16][2]
    float ps1 = 0.f, ps2 = 0.f;                                 // this lane's share of (sum, sum of squares) of row g*4 + wave
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int r = tid >> 6;
        const float v = red[((0 * NT + t) * 4 + r) * 64 + lane] + red[((1 * NT + t) * 4 + r) * 64 + lane] +
                        red[((2 * NT + t) * 4 + r) * 64 + lane] + red[((3 * NT + t) * 4 + r) * 64 + lane];
        const int m = g * 4 + r, n = nloc[t];
        if (m < Mb && n >= 0) {
            const size_t o = (size_t)m * ldo + n;
            const float back = wsum ? smean[m] * wsum_v[t] : 0.f;
            if (epi == 0) {
                out[o] = v + bias_v[t] + back;
            } else if (epi == 2) {
                atomicAdd(out + o, v + bias_v[t] + back);
            } else {
                const float rv = resid_pre[t] + resid_grid(v + bias_v[t]);
                out[o] = rv;
                if (out2) out2[o] = rv;
                ps1 += rv; ps2 += rv * rv;
            }
        }
    }
    if (epi == 1 && pstats) {
        // per-block LayerNorm partial sums of the rows just written (the 16 lanes of a DPP row hold the 16 columns of one
        // output row): the consumer adds the blocks' partials in a fixed order instead of re-reading the rows
#pragma unroll
        for (int sft = 0; sft < 4; ++sft) {
            ps1 += sft == 0 ? dpp_mov<0x111, 0xf>(0.f, ps1) : sft == 1 ? dpp_mov<0x112, 0xf>(0.f, ps1) : sft == 2 ? dpp_mov<0x114, 0xf>(0.f, ps1) : dpp_mov<0x118, 0xf>(0.f, ps1);
            ps2 += sft == 0 ? dpp_mov<0x111, 0xf>(0.f, ps2) : sft == 1 ? dpp_mov<0x112, 0xf>(0.f, ps2) : sft == 2 ? dpp_mov<0x114, 0xf>(0.f, ps2) : dpp_mov<0x118, 0xf>(0.f, ps2);
        }
        const int m = g * 4 + (tid >> 6);
        if (l15 == 15) *(float2*)(pstats + ((size_t)(bid - block0) * 16 + m) * 2) = make_float2(ps1, ps2);
    }
}

template <int RPW, int NT>
static int launch_stack_nt(StackParams& p, hipStream_t st) {
    int blocks = 0;
    for (int s = 0; s < p.nseg; ++s) {
        if (p.seg[s].nt <= 0 || p.seg[s].nt > NT) p.seg[s].nt = NT;
        p.seg[s].block0 = blocks;
        blocks += (p.seg[s].n_tiles + p.seg[s].nt - 1) / p.seg[s].nt;
    }
    if (p.zero && (long long)blocks * 256 < p.zero_n4) return CW_ERR_INVALID;
    const size_t lds = (size_t)16 * (p.K + 8) * 2 + (size_t)4 * NT * 4 * 64 * 4 + 16 * 4;
    const dim3 grid(blocks, (p.Mb + 15) / 16);                  // y: groups of 16 rows
    if (p.K > 0xffff || p.Mb > 0xff || blocks > 0xffff) return CW_ERR_INVALID;   // packed into gemv_stack_kernel's leading arguments
#define CW_STACK_LEAD(p)                                                                                                     \
    (p).W, (p).zero, (p).zero_n4, (unsigned)(p).K | (unsigned)(p).Mb << 16 | (unsigned)(p).nseg << 24 | ((p).wpk ? 1u << 26 : 0u), \
        (unsigned)((p).nseg > 1 ? (p).seg[1].block0 : 0) | (unsigned)((p).nseg > 2 ? (p).seg[2].block0 : 0) << 16, (p)
    if (p.K <= 256) hipLaunchKernelGGL((gemv_stack_kernel<RPW, 1, 1, NT>), grid, dim3(256), lds, st, CW_STACK_LEAD(p));
    else if (p.K <= 768) hipLaunchKernelGGL((gemv_stack_kernel<RPW, 2, 3, NT>), grid, dim3(256), lds, st, CW_STACK_LEAD(p));
    else {
        bool uni = p.wpk != 0;
        for (int s = 0; s < p.nseg; ++s) uni = uni && p.seg[s].nt == NT;
        if (uni && p.wnt && grid.y == 1) hipLaunchKernelGGL((gemv_stack_kernel<RPW, 3, 5, NT, true, true>), grid, dim3(256), lds, st, CW_STACK_LEAD(p));
        else if (uni) hipLaunchKernelGGL((gemv_stack_kernel<RPW, 3, 5, NT, true>), grid, dim3(256), lds, st, CW_STACK_LEAD(p));
        else hipLaunchKernelGGL((gemv_stack_kernel<RPW, 3, 5, NT>), grid, dim3(256), lds, st, CW_STACK_LEAD(p));
    }
#undef CW_STACK_LEAD
    return CW_OK;
}

// nt: most 16-column tiles per block (1..3; segments may ask for fewer through StackSeg::nt); 0 = chosen so that the launch
// is one block per CU at most where possible
int cw_launch_gemv_stack(const StackParams& p_in, int nt, hipStream_t st) {
    StackParams p = p_in;
    if (p.Mb < 1 || p.Mb > 64 || p.K % 128 || p.K > 1280 || p.nseg < 1 || p.nseg > 3) return CW_ERR_INVALID;
    if (nt <= 0) {
        nt = 1;
        for (;;) {
            int blocks = 0;
            for (int s = 0; s < p.nseg; ++s) {
                const int snt = p.seg[s].nt > 0 && p.seg[s].nt < nt ? p.seg[s].nt : nt;
                blocks += (p.seg[s].n_tiles + snt - 1) / snt;
            }
            if (blocks <= 256 || nt == 3) break;
            ++nt;
        }
    }
    if (p.Mb > 8) {                                              // 9..16 rows: four rows per wave
        if (nt == 1) return launch_stack_nt<4, 1>(p, st);
        if (nt == 2) return launch_stack_nt<4, 2>(p, st);
        return launch_stack_nt<4, 3>(p, st);
    }
    if (nt == 1) return launch_stack_nt<2, 1>(p, st);
    if (nt == 2) return launch_stack_nt<2, 2>(p, st);
    return launch_stack_nt<2, 3>(p, st);
}

// ---------------------------------------------------------------------------------------------------
// gemv_stack_a16_kernel: the stage's two `a` segments behind qkv_self_kernel<.., XQ> (declayer.hip), rows <= 8, one tile per block,
// fragment-major weights (DESIGN.md 6g''').  That launch computes the x segment in blocks that finish early and leaves the self-attention
// output in 16 bits -- the rounding the segments' first use of an f32 row was -- so a block here takes in 20 KB of rows instead of 40 and
// the launch is 2 K/16 blocks instead of 3 K/16:
//   block b <  K/16:  qb = (W'q_c Wo) a            tile K/16 + b of W
//   block b >= K/16:  x1 = resid + grid(Wo a + bo)  tile K/16 + b of W, and the LayerNorm partial sums of its 16 columns
// Same K steps per wave, MFMA order, cross-wave sum and epilogues as gemv_stack_kernel<2, NSLOT, 2 PL16 - 1, 1, true, WNT>: bit-identical.
// Kernel arguments: everything a request of the entry is addressed from -- W, the rows, the residual rows, the bias, dims = K | Mb << 16
// -- is 9 leading dwords, preloaded into user SGPRs; the three destinations follow in `p` and arrive under the requests.
// ---------------------------------------------------------------------------------------------------
template <int NSLOT, int PL16, bool WNT>
__global__ __launch_bounds__(256) void gemv_stack_a16_kernel(const void* __restrict__ Wp, const void* a16, const float* resid, const float* bias, unsigned dims,
                                                             StackA16Out p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_a[];
    const int K = (int)(dims & 0xffffu), Mb = (int)(dims >> 16), TD = K >> 4;
    const int xs_stride = K + 8;
    bf16_t* xs = (bf16_t*)smem_a;                               // [16][K+8]
    float* red = (float*)(smem_a + (size_t)16 * xs_stride * 2);  // [4 waves][4][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int bid = blockIdx.x;
    const bool seg_x1 = bid >= TD;                               // block-uniform
    const int tl = seg_x1 ? bid - TD : bid;                      // tile inside the segment
    const int steps = K >> 7, nv8 = K >> 3;
    const int n = tl * 16 + l15;                                 // output column
    // every load is unconditional: the qb segment has no bias and no residual, and reads the x1 segment's in their place
    const float bias_ld = bias[n];
    const float resid_pre = resid[(size_t)min(g * 4 + wave, Mb - 1) * K + n];
    u32x4_t av[2][PL16];                                         // rows wave, wave + 4: 16 bytes per lane per load
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int row = wave + 4 * i;
        row = row < Mb ? row : Mb - 1;
#pragma unroll
        for (int c = 0; c < PL16; ++c) {
            int v8 = lane + 64 * c;
            v8 = v8 < nv8 ? v8 : nv8 - 1;
            av[i][c] = *(const u32x4_t*)((const bf16_t*)a16 + (size_t)row * K + v8 * 8);
        }
    }
    __builtin_amdgcn_sched_barrier(0);                           // the rows are waited for first: their requests go first
    u32x4_t wq[NSLOT][4];
    const bf16_t* __restrict__ W = (const bf16_t*)Wp;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        int step = wave + 4 * s;
        step = step < steps ? step : steps - 1;
        const u32x4_t* wp = (const u32x4_t*)(W + ((((size_t)(TD + bid) * (K >> 5)) + step * 4) * 64 + lane) * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) wq[s][j] = WNT ? CW_STREAM_LD(wp + j * 64) : wp[j * 64];
    }
    __builtin_amdgcn_sched_barrier(0);
    // rows -> LDS as they are
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wave + 4 * i;
#pragma unroll
        for (int c = 0; c < PL16; ++c) {
            int v8 = lane + 64 * c;                             // (unconditional like the load: a tail lane rewrites the last chunk with itself)
            v8 = v8 < nv8 ? v8 : nv8 - 1;
            *(u32x4_t*)(xs + (size_t)row * xs_stride + v8 * 8) = av[i][c];
        }
    }
    float bias_v = bias_ld, resid_v = resid_pre;
    asm volatile("" : "+v"(bias_v), "+v"(resid_v));          // their requests stay at the head of the queue: hipcc otherwise sinks them into the x1 epilogue
    __syncthreads();
    f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        // A tail wave (step >= steps) runs the slot on the clamped step it loaded and drops the result: under a branch hipcc sinks
        // the slot's weight requests into it, behind the barrier (the K steps that count, and their order, are gemv_stack_kernel's)
        const int step = wave + 4 * s, stepc = step < steps ? step : steps - 1;
        const bf16_t* xr = xs + (size_t)l15 * xs_stride + stepc * 128 + g * 8;
        f32x4_t nacc = acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
            nacc = mfma16x(a, __builtin_bit_cast(bf16x8_t, wq[s][j]), nacc);
        }
        acc = step < steps ? nacc : acc;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    __syncthreads();
    const int r = tid >> 6;
    const float v = red[(0 * 4 + r) * 64 + lane] + red[(1 * 4 + r) * 64 + lane] + red[(2 * 4 + r) * 64 + lane] + red[(3 * 4 + r) * 64 + lane];
    const int m = g * 4 + r;
    const size_t o = (size_t)m * K + n;
    if (!seg_x1) {
        if (m < Mb) p.qb[o] = v + 0.f + 0.f;                     // gemv_stack_kernel's epi 0 without bias and add-back (-0 leaves as +0 there too)
        return;
    }
    float ps1 = 0.f, ps2 = 0.f;                                 // this lane's share of (sum, sum of squares) of row g*4 + wave
    if (m < Mb) {
        const float rv = resid_v + resid_grid(v + bias_v);
        p.x1[o] = rv;
        ps1 += rv; ps2 += rv * rv;
    }
#pragma unroll
    for (int sft = 0; sft < 4; ++sft) {
        ps1 += sft == 0 ? dpp_mov<0x111, 0xf>(0.f, ps1) : sft == 1 ? dpp_mov<0x112, 0xf>(0.f, ps1) : sft == 2 ? dpp_mov<0x114, 0xf>(0.f, ps1) : dpp_mov<0x118, 0xf>(0.f, ps1);
        ps2 += sft == 0 ? dpp_mov<0x111, 0xf>(0.f, ps2) : sft == 1 ? dpp_mov<0x112, 0xf>(0.f, ps2) : sft == 2 ? dpp_mov<0x114, 0xf>(0.f, ps2) : dpp_mov<0x118, 0xf>(0.f, ps2);
    }
    if (l15 == 15) *(float2*)(p.pstats + ((size_t)tl * 16 + m) * 2) = make_float2(ps1, ps2);
}

int cw_launch_gemv_stack_a16(const StackA16Params& p, hipStream_t st) {
    if (p.Mb < 1 || p.Mb > 8 || p.K % 128 || p.K < 128 || p.K > 1280 || !p.W || !p.a16 || !p.resid || !p.bias || !p.qb || !p.x1 || !p.pstats) return CW_ERR_INVALID;
    const size_t lds = (size_t)16 * (p.K + 8) * 2 + (size_t)4 * 4 * 64 * 4;
    const dim3 grid(2 * (p.K / 16));
    const unsigned dims = (unsigned)p.K | (unsigned)p.Mb << 16;
    const StackA16Out out{p.qb, p.x1, p.pstats};
#define CW_A16_LAUNCH(NS, PL)                                                                                                        \
    do {                                                                                                                              \
        if (p.wnt) hipLaunchKernelGGL((gemv_stack_a16_kernel<NS, PL, true>), grid, dim3(256), lds, st, p.W, p.a16, p.resid, p.bias, dims, out);  \
        else hipLaunchKernelGGL((gemv_stack_a16_kernel<NS, PL, false>), grid, dim3(256), lds, st, p.W, p.a16, p.resid, p.bias, dims, out);       \
    } while (0)
    if (p.K <= 256) CW_A16_LAUNCH(1, 1);
    else if (p.K <= 768) CW_A16_LAUNCH(2, 2);
    else CW_A16_LAUNCH(3, 3);
#undef CW_A16_LAUNCH
    return CW_OK;
}

// ===================================================================================================
// Measured and rejected: kept as published A/Bs behind -DCW_EXPERIMENTS, not part of the default library.
// ===================================================================================================
#ifdef CW_EXPERIMENTS
#include "decfuse_experiments.inc"   // 600 lines of published A/B kernels, outside the default build
#else   // !CW_EXPERIMENTS: the measured-and-rejected stages are not in the library (make EXTRA=-DCW_EXPERIMENTS builds them)
int cw_launch_gemv_fc2x(const Fc2xParams&, hipStream_t) { return CW_ERR_INVALID; }
int cw_launch_mlp_pair(const MlpPairParams&, hipStream_t) { return CW_ERR_INVALID; }
int cw_launch_rows_prep(const float*, int, int, void*, float*, int, hipStream_t) { return CW_ERR_INVALID; }
int cw_launch_gemv_rows(int, bool, const RowsParams&, hipStream_t) { return CW_ERR_INVALID; }
#endif

}  // namespace CW_NS
