// Persistent decoder-layer kernel of the 16-bit engine, batch rows <= 8 (TF modeling_whisper.py:448-505, the decoder layer's
// forward): ONE 1024-thread workgroup per CU walks the dependent stages of a layer inside one launch.
//
// Why: a decoder layer at 8 rows is a chain of 7 all-to-all dependent stages that move 118 MB; as 7 launches
// it takes 44 us against 18.7 us of streaming, because every launch starts its HBM streams only after its predecessor has
// drained.  The one stream that is worth a layer's time -- the 61.5 MB of cross-attention K/V -- depends on NOTHING the layer
// computes.  Here every CU requests its share of it (up to four (row, head, key split) items = 256 KB, held in the registers of
// 16 waves: 64 VGPRs of payload per lane) at kernel entry, and the latency-bound chain in front of the cross-attention -- the
// fused out-projection / cross-query stage of decfuse.hip -- runs underneath that stream on four "chain" waves whose own memory
// queue stays short: their weights arrive by LDS-DMA (no payload registers), they hand their results to the other CUs as 8-byte
// {tag, value} granules (one write-through store each: data and arrival flag travel together, no fence, no barrier, no separate
// flag -- MI355X_MICROARCH.md, rows handoff-1to1 / allgather), and they poll for theirs.
//
// Arithmetic = gemv_stack_kernel<2, NSLOT, PER_LANE, 1> (decfuse.hip) followed by attn_cross_split_kernel<T, 1, true>
// (attention.hip), operation for operation: same roundings, same summation orders, same key ownership per lane -- the two paths
// are held BIT-IDENTICAL by tests/test_gpu_e2e.py::test_persistent_decoder_layer_is_bit_identical.
//
// Hand-off state: granule buffers live in HBM and are never cleared; a granule is valid when its tag equals
// (epoch << 6 | layer), epoch = a device counter that set_pos_kernel / sample_kernel bump once per decoder forward (so it
// survives graph replay: no per-launch argument changes).  Every spin is bounded and reports through `err`.
#include "common.h"
#include "kernels.h"
#include <mutex>

namespace CW_NS {

typedef __attribute__((ext_vector_type(4))) unsigned int dl_u32x4_t;
typedef unsigned long long dl_u64_t;

#define DL_THREADS 1024
#define DL_SPIN_LIMIT (1 << 17)

// Development aid (make EXTRA=-DCW_PHASE_TIMING, tools/dl_phase_probe.py): lane 0 of waves 0 (chain), 4 and 8 (K/V waves of the two
// groups) of every workgroup stamps the 100 MHz wall clock at the phase boundaries; cw_debug_dl_phases copies the stamps out.
#if defined(CW_PHASE_TIMING) && !defined(CW_F16)
__device__ unsigned long long g_dl_phase[256 * 3 * 16];
#define DLPH(i)                                                                                                     \
    do {                                                                                                            \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 256) {                                                          \
            const int w_ = threadIdx.x >> 6;                                                                        \
            if (w_ == 0 || w_ == 4 || w_ == 8) g_dl_phase[(blockIdx.x * 3 + (w_ >> 2)) * 16 + (i)] = wall_clock64(); \
        }                                                                                                           \
    } while (0)
extern "C" int cw_debug_dl_phases(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dl_phase), sizeof(unsigned long long) * 256 * 3 * 16);
}
#define DLPHV(i, v)                                                                                                 \
    do {                                                                                                            \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 256 && (threadIdx.x >> 6) == 0) g_dl_phase[(blockIdx.x * 3) * 16 + (i)] = (unsigned long long)(v); \
    } while (0)
#else
#define DLPH(i) do { } while (0)
#define DLPHV(i, v) do { } while (0)
#endif

__device__ static inline void dl_glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// The same request in inline assembly, invisible to hipcc: its waitcnt pass cannot count LDS-DMA issued in a loop and answers every
// later LDS read ("may alias the DMA destination") with s_waitcnt vmcnt(0) -- which here would drain the sixteen K/V loads the
// wave carries across the barrier.  The caller orders the destination by its own vmcnt wait + barrier.  lds_wave_base: wave-uniform.
__device__ static inline void dl_glds16_asm(const void* gsrc, void* lds_wave_base) {
    unsigned keep;
    const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)lds_wave_base);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(m0v) : "memory");
}
// workgroup barrier WITHOUT the workgroup-scope fence of __syncthreads(): that fence drains vmcnt, and twelve of the sixteen
// waves carry 16 K/V loads each across every barrier of the chain.  LDS traffic is ordered by lgkmcnt alone.
__device__ static inline void dl_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
__device__ static inline void dl_gran_st(dl_u64_t* g, unsigned tag, unsigned v) {
    __hip_atomic_store(g, ((dl_u64_t)tag << 32) | (dl_u64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ static inline dl_u64_t dl_gran_ld(const dl_u64_t* g) {
    return __hip_atomic_load((dl_u64_t*)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ static inline float dl_row_ror8_add(float v) { return v + dpp_mov<0x128, 0xf>(0.f, v); }

struct DlRaw8 {   // 8 consecutive 16-bit elements held raw so that the load is issued long before its use (attention.hip: Raw8)
    uint4 a;
    __device__ inline void ld(const bf16_t* p) {
        const dl_u32x4_t t = CW_STREAM_LD((const dl_u32x4_t*)p);
        a = make_uint4(t[0], t[1], t[2], t[3]);
    }
    __device__ inline void cvt(float* o) const { h16_unpack8(a, o); }
};

#ifdef CW_EXPERIMENTS   // stage A: measured slower than its two launches (profiles/r05_declayer_phases.txt); A/B builds only (CW_DECLAYER=1)
// ---------------------------------------------------------------------------------------------------
// stage A: [W'q_c ; W'q_c Wo ; Wo] tile (chain waves) -> granules -> cross-attention items (all waves)
// ---------------------------------------------------------------------------------------------------
// Barrier among the four chain waves only (the other twelve are inside their K/V issue loop and must not be waited for):
// a monotonic arrival counter in LDS.  k = 1, 2, 3 ... in program order.
__device__ static inline void dl_chain_sync(unsigned* cb, int k, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(cb, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (__hip_atomic_load(cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned)(4 * k)) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}

struct DlItem { int b, h, sp, nk, klo, aslot, arow; bool valid; };   // aslot: alignment slot of the head (or -1); arow: alignment row (= pos[b])

// The two items of a group, one after the other, both groups in lockstep (hardware barriers): attn_cross_split_kernel<T, 1, true>
// from its K pass on (gt / gw stand for its tid / wave).  Instantiated once per wave role so that each role's vmcnt bookkeeping
// is exact: item 0 starts when ITS rows have landed, item 1's land underneath it.
__device__ __forceinline__ void dl_cross_items(const DecLayerParams& p, const DlItem (&it)[2], DlRaw8 (&kr)[2][4], DlRaw8 (&vr)[2][4],
                                               int grp, int gw, int gt, int lane, const float* c_q, float* c_smax, float* c_redl,
                                               float* c_red) {
    const int sub = gt & 7, kg = gt >> 3;
    const int Mb = p.Mb, H = p.H;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int slot_i = 2 * grp + s;
        const int nk = it[s].nk, h = it[s].h, b0 = it[s].b, sp = it[s].sp, k_lo = it[s].klo;
        float qv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] = c_q[slot_i * 64 + sub * 8 + e];
        float d[4], mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float kv[8];
            kr[s][u].cvt(kv);
            float t = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) t = fmaf(qv[e], kv[e], t);
            t += __shfl_xor(t, 1, 64); t += __shfl_xor(t, 2, 64); t += __shfl_xor(t, 4, 64);
            d[u] = (kg + u * 64 < nk) ? t : -INFINITY;
            mx = fmaxf(mx, d[u]);
        }
        mx = wave_max(mx);
        if (lane == 0) c_smax[slot_i * 8 + gw] = mx;
        dl_barrier();
        {
            float m = c_smax[slot_i * 8];
#pragma unroll
            for (int w = 1; w < 8; ++w) m = fmaxf(m, c_smax[slot_i * 8 + w]);
            mx = m;
        }
        const int aslot = it[s].aslot;                  // fetched at kernel entry: a load issued here would sit BEHIND the K/V rows (in-order return)
        float acc[8];
        float lsum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = kg + u * 64;
            float vv[8];
            vr[s][u].cvt(vv);
            const float pk = (k < nk) ? expf(d[u] - mx) : 0.f;
            if (sub == 0 && k < nk) {
                lsum += pk;
                if (aslot >= 0) {
                    const size_t rowi = ((size_t)b0 * p.n_align + aslot) * p.align_rows + it[s].arow;
                    p.align_out[rowi * p.n_keys + k_lo + k] = pk;
                }
            }
            if (k < nk) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, vv[e], acc[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = xor32_sum(xor16_sum(dl_row_ror8_add(acc[e])));
        lsum = wave_sum(lsum);
        if (lane < 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) c_red[(slot_i * 8 + gw) * 64 + sub * 8 + e] = acc[e];
        }
        if (lane == 0) c_redl[slot_i * 8 + gw] = lsum;
        dl_barrier();
        DLPH(11 + s);
        if (it[s].valid) {
            if (gt < 64) {
                float r = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) r += c_red[(slot_i * 8 + w) * 64 + gt];
                p.part_o[((size_t)sp * Mb + b0) * H * 64 + h * 64 + gt] = r;
            }
            if (gt == 64) {
                float l = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) l += c_redl[slot_i * 8 + w];
                float* ml = p.part_ml + (((size_t)b0 * H + h) * ATT_NS + sp) * 2;
                ml[0] = mx; ml[1] = l;
                if (aslot >= 0) {
                    const size_t rowi = ((size_t)b0 * p.n_align + aslot) * p.align_rows + it[s].arow;
                    p.align_ml[(rowi * ATT_NS + sp) * 2] = mx; p.align_ml[(rowi * ATT_NS + sp) * 2 + 1] = l;
                }
            }
        }
    }
}

// K/V row load number `idx` (0..15) of a lane: item idx / 8, K before V, four rows each -- the order the items consume them in
#define DL_KV_LOAD(idx)                                                                                                      \
    do {                                                                                                                      \
        constexpr int s_ = (idx) >> 3, v_ = ((idx) >> 2) & 1, u_ = (idx) & 3;                                                \
        const size_t ro_ = (size_t)min(kg + u_ * 64, it[s_].nk - 1) * 64;                                                    \
        if (v_) vr[s_][u_].ld(Vp[s_] + ro_); else kr[s_][u_].ld(Kp[s_] + ro_);                                              \
    } while (0)

__device__ static inline DlItem dl_item(const DecLayerParams& p, int i, int n_items, int per) {
    DlItem t;
    t.valid = i < n_items;
    const int ic = t.valid ? i : 0;
    t.h = ic % p.H; t.b = (ic / p.H) % p.Mb; t.sp = ic / (p.H * p.Mb);   // = blockIdx (x, y, z) of attn_cross_split_kernel
    t.klo = t.sp * per;
    t.nk = min(p.n_keys, t.klo + per) - t.klo;
    t.aslot = (p.align_out && t.valid) ? p.align_slot[t.h] : -1;
    t.arow = p.pos[t.b];
    return t;
}

template <int NSLOT, int PER_LANE, int DEPTH>
__global__ __launch_bounds__(DL_THREADS) void dec_layer_a_kernel(DecLayerParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    const int K = p.D, Mb = p.Mb, H = p.H;
    const int TD = K >> 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..15
    const int grp = wave >> 3, gw = wave & 7, gt = tid & 511;       // 8-wave group = one attn_cross_split block
    const bool chain = wave < 4;
    // the chain waves' vector-memory instructions go first: the K/V waves keep the CU's memory queue full from entry to exit, and
    // an instruction of equal priority waits its turn among sixteen waves (phase stamps: 2.9 us to ISSUE 20 requests)
    if (chain) __builtin_amdgcn_s_setprio(3);
    const int l15 = lane & 15, g = lane >> 4;
    const int cu = blockIdx.x, G = gridDim.x;
    const unsigned tag = (p.epoch[0] << 6) | (unsigned)p.layer;

    // ---- LDS carve (one workgroup per CU: 160 KB are ours)
    const int xs_stride = K + 8;
    bf16_t* xs = (bf16_t*)dsm;                                       // [16][K+8] activation rows of the tile, 16 bit
    float* red = (float*)(dsm + (size_t)16 * xs_stride * 2);         // [4 waves][4][64]
    float* smean = red + 4 * 4 * 64;                                 // [16]
    float* c_smax = smean + 16;                                      // [4 items][8 waves]
    float* c_redl = c_smax + 32;                                     // [4][8]
    float* c_q = c_redl + 32;                                        // [4][64] finished queries
    float* c_red = c_q + 4 * 64;                                     // [4][8][64]
    unsigned* cb = (unsigned*)(c_red + 4 * 8 * 64);                  // arrival counter of the chain waves (+ pad to 16 B)
    unsigned char* kvL = (unsigned char*)(cb + 4);                   // [4 chain waves][16 rows][64 lanes][16 B]: their share of K/V

    // ---- work of this CU: cross-attention items cu, cu + G, cu + 2G, cu + 3G (group 0: the first two); one tile, dealt from
    // the END of the grid because the last CUs hold one item less
    const int n_items = Mb * H * ATT_NS;
    const int per = (p.n_keys + ATT_NS - 1) / ATT_NS;
    DlItem it[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) it[s] = dl_item(p, cu + G * (2 * grp + s), n_items, per);
    const int n_tiles = 3 * TD;
    const int my_tile = G - 1 - cu;
    const bool has_tile = my_tile < n_tiles;
    const int si = has_tile ? my_tile / TD : 0;                      // segment: 0 qa = W'q x, 1 qb = (W'q Wo) a, 2 x1 = x + Wo a + bo
    const int tl = has_tile ? my_tile - si * TD : 0;
    const int steps = K >> 7, nvec = K >> 2;
    const int sub = gt & 7, kg = gt >> 3;                            // 8 lanes per key row, 64 key groups per item
    DlRaw8 kr[2][4], vr[2][4];
    DLPH(0);
    if (tid == 0) *cb = 0u;
    dl_barrier();
    DLPH(1);

    if (!chain) {
        // ================= the twelve K/V waves =================
        // A/B (CW_DL_KVWAIT=1|2): the stream starts only when the chain's tile has its rows in LDS (1) / its weights through the
        // matrix cores (2) -- requests issued together with the tile's share the memory system fairly, and the tile then lands
        // when half the stream has, not first
        if (p.kv_wait && has_tile) {
            const unsigned need = p.kv_wait == 1 ? 4u : 8u;
            while (__hip_atomic_load(cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(2);
        }
        // (a) the chain waves' share of group 0's rows goes to LDS by DMA, requested here and FIRST: a chain wave that carried
        // these 16 requests itself would find every poll queued behind them (vector memory returns in order)
        {
            const DlItem ga_ = dl_item(p, cu, n_items, per), gb_ = dl_item(p, cu + G, n_items, per);
            for (int n = wave - 4; n < 64; n += 12) {
                const int w = n >> 4, idx = n & 15;                 // row `idx` of chain wave w
                const int s_ = idx >> 3, v_ = (idx >> 2) & 1, u_ = idx & 3;
                const int cgt = w * 64 + lane, csub = cgt & 7, ckg = cgt >> 3;
                const int gb0 = s_ ? gb_.b : ga_.b, gh0 = s_ ? gb_.h : ga_.h, gk0 = s_ ? gb_.klo : ga_.klo, gn0 = s_ ? gb_.nk : ga_.nk;
                const size_t o = (((size_t)gb0 * H + gh0) * p.n_keys + gk0 + min(ckg + u_ * 64, gn0 - 1)) * 64 + csub * 8;
                dl_glds16_asm((const bf16_t*)(v_ ? p.V : p.K) + o, kvL + (size_t)n * 1024);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // (b) their own 16 rows of 16 B per lane, at most DEPTH in flight (A/B: the depth does not matter, the CU's memory queue
        // is full either way -- profiles/r05_declayer_phases.txt)
        const bf16_t* Kp[2];
        const bf16_t* Vp[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const size_t o = (((size_t)it[s].b * H + it[s].h) * p.n_keys + it[s].klo) * 64 + sub * 8;
            Kp[s] = (const bf16_t*)p.K + o;
            Vp[s] = (const bf16_t*)p.V + o;
        }
#define DL_STEP(idx)                                                                                                          \
        do {                                                                                                                  \
            if ((idx) >= DEPTH) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DEPTH - 1) : "memory");                              \
            DL_KV_LOAD(idx);                                                                                                  \
        } while (0)
        DL_STEP(0); DL_STEP(1); DL_STEP(2); DL_STEP(3); DL_STEP(4); DL_STEP(5); DL_STEP(6); DL_STEP(7);
        DL_STEP(8); DL_STEP(9); DL_STEP(10); DL_STEP(11); DL_STEP(12); DL_STEP(13); DL_STEP(14); DL_STEP(15);
#undef DL_STEP
        DLPH(2);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");           // the DMA (issued first, returned first) is in LDS
        dl_barrier();                                               // queries are in c_q, the chain waves may read their rows
        DLPH(10);
        dl_cross_items(p, it, kr, vr, grp, gw, gt, lane, c_q, c_smax, c_redl, c_red);
        return;
    }

    // ================= chain waves =================
    // ---- (0) the tile exactly as gemv_stack_kernel takes it: per-column constants, activation rows, weight fragments -> registers,
    // every load unconditional and in flight before the first wait
    const float* __restrict__ bias = si == 0 ? p.qa_bias : (si == 2 ? p.bo : nullptr);
    const float* __restrict__ wsum = si == 0 ? p.q_wsum : nullptr;
    const int ncl = tl * 16 + l15;
    float bias_v = 0.f, wsum_v = 0.f, resid_v = 0.f;
    const int it_w = cu + G * wave;                                  // chain wave w finishes the query of item slot w
    const bool q_mine = it_w < n_items;
    const int qh = q_mine ? it_w % H : 0, qb_row = q_mine ? (it_w / H) % Mb : 0;
    const float qw1 = p.qw[(size_t)qh * 64 + lane], qc1 = p.qbias[(size_t)qh * 64 + lane];
    if (has_tile) {
        bias_v = bias ? bias[ncl] : 0.f;
        wsum_v = wsum ? wsum[ncl] : 0.f;
        const int m = g * 4 + wave;
        if (si == 2 && m < Mb) resid_v = p.x[(size_t)m * K + ncl];
        const float* __restrict__ x = si == 0 ? p.x : p.a;
        float4 xv[2][PER_LANE];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int row = wave + 4 * i;
            row = row < Mb ? row : Mb - 1;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                int v4 = lane + 64 * c;
                v4 = v4 < nvec ? v4 : nvec - 1;
                xv[i][c] = *(const float4*)(x + (size_t)row * K + v4 * 4);
            }
        }
        dl_u32x4_t wq[NSLOT][4];
        const bf16_t* __restrict__ W = (const bf16_t*)p.Ws;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            int step = wave + 4 * s;
            step = step < steps ? step : steps - 1;
            const dl_u32x4_t* wp = (const dl_u32x4_t*)(W + ((((size_t)my_tile * (K >> 5)) + step * 4) * 64 + lane) * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) wq[s][j] = wp[j * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        DLPH(2);
        // ---- (1) rows -> 16 bit -> LDS (wave w owns rows w, w + 4; centred rounding of offset rows)
        if (wsum) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float sx = 0.f, sq = 0.f;
#pragma unroll
                for (int c = 0; c < PER_LANE; ++c)
                    if (lane + 64 * c < nvec) {
                        sx += (xv[i][c].x + xv[i][c].y) + (xv[i][c].z + xv[i][c].w);
                        sq += cw_sumsq4(xv[i][c].x, xv[i][c].y, xv[i][c].z, xv[i][c].w);
                    }
                float mu = wave_sum(sx) / (float)K;
                if (2.f * mu * mu < wave_sum(sq) / (float)K) mu = 0.f;
#pragma unroll
                for (int c = 0; c < PER_LANE; ++c) { xv[i][c].x -= mu; xv[i][c].y -= mu; xv[i][c].z -= mu; xv[i][c].w -= mu; }
                if (lane == 0) smean[wave + 4 * i] = mu;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
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
        DLPH(3);
        dl_chain_sync(cb, 1, lane);
        DLPH(5);
        // ---- (2) MFMA over the wave's K steps w, w + 4, w + 8
        {
            f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NSLOT; ++s) {
                const int step = wave + 4 * s;
                if (step < steps) {
                    const bf16_t* xr = xs + (size_t)l15 * xs_stride + step * 128 + g * 8;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
                        acc = cw_mfma_16x16x32(a, __builtin_bit_cast(bf16x8_t, wq[s][j]), acc);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
        }
        dl_chain_sync(cb, 2, lane);
        DLPH(6);
        // ---- (3) epilogue: cross-wave sum in gemv_stack_kernel's order, results leave as granules (qa, qb, LayerNorm partial
        // sums of x1) and as the plain residual rows x1 that later launches read
        {
            const int r = wave;
            const float v = red[(0 * 4 + r) * 64 + lane] + red[(1 * 4 + r) * 64 + lane] + red[(2 * 4 + r) * 64 + lane] + red[(3 * 4 + r) * 64 + lane];
            const int m = g * 4 + r;
            float ps1 = 0.f, ps2 = 0.f;
            if (m < Mb) {
                const size_t o = (size_t)m * K + ncl;
                const float back = wsum ? smean[m] * wsum_v : 0.f;
                if (si < 2) {
                    dl_gran_st(p.gq + ((size_t)si * 16 + m) * K + ncl, tag, __float_as_uint(v + bias_v + back));
                } else {
                    const float rv = resid_v + resid_grid(v + bias_v);
                    p.x1[o] = rv;
                    ps1 += rv; ps2 += rv * rv;
                }
            }
            if (si == 2) {
#pragma unroll
                for (int sft = 0; sft < 4; ++sft) {
                    ps1 += sft == 0 ? dpp_mov<0x111, 0xf>(0.f, ps1) : sft == 1 ? dpp_mov<0x112, 0xf>(0.f, ps1) : sft == 2 ? dpp_mov<0x114, 0xf>(0.f, ps1) : dpp_mov<0x118, 0xf>(0.f, ps1);
                    ps2 += sft == 0 ? dpp_mov<0x111, 0xf>(0.f, ps2) : sft == 1 ? dpp_mov<0x112, 0xf>(0.f, ps2) : sft == 2 ? dpp_mov<0x114, 0xf>(0.f, ps2) : dpp_mov<0x118, 0xf>(0.f, ps2);
                }
                if (l15 == 15) {   // rows >= Mb publish zeros like gemv_stack_kernel (never read)
                    dl_gran_st(p.gps + ((size_t)tl * 16 + m) * 2, tag, __float_as_uint(ps1));
                    dl_gran_st(p.gps + ((size_t)tl * 16 + m) * 2 + 1, tag, __float_as_uint(ps2));
                }
            }
        }
    }
    DLPH(7);
    // ---- (4) chain wave w finishes the query of item slot w (attn_cross_split_kernel<.., FUSED>: lane c = column c of the head):
    //     q = rstd(x1) (qa + qb - mean(x1) qw) + qbias
    // from the granules of the 8 tiles that hold the head's columns and of the TD tiles that hold the row's partial sums.  The
    // wave's own memory queue is empty while it polls.
    {
        const size_t col = (size_t)qh * 64 + lane;
        const dl_u64_t* ga = p.gq + ((size_t)0 * 16 + qb_row) * K + col;
        const dl_u64_t* gb = p.gq + ((size_t)1 * 16 + qb_row) * K + col;
        const dl_u64_t* g0 = p.gps + ((size_t)min(lane, TD - 1) * 16 + qb_row) * 2;
        const dl_u64_t* g1 = p.gps + ((size_t)min(lane + 64, TD - 1) * 16 + qb_row) * 2;
        dl_u64_t va = 0, vb = 0, v00 = 0, v01 = 0, v10 = 0, v11 = 0;
        bool ready = !q_mine;
        int npoll = 0; (void)npoll;
#pragma unroll 1
        for (int spins = 0; !ready; ++spins) {
            if (spins > DL_SPIN_LIMIT) { if (lane == 0) atomicCAS(p.err, 0, 1); break; }
            va = dl_gran_ld(ga); vb = dl_gran_ld(gb);
            v00 = dl_gran_ld(g0); v01 = dl_gran_ld(g0 + 1);
            v10 = dl_gran_ld(g1); v11 = dl_gran_ld(g1 + 1);
            const bool ok = (unsigned)(va >> 32) == tag && (unsigned)(vb >> 32) == tag && (unsigned)(v00 >> 32) == tag &&
                            (unsigned)(v01 >> 32) == tag && (unsigned)(v10 >> 32) == tag && (unsigned)(v11 >> 32) == tag;
            ready = __all(ok); ++npoll;
            if (spins == 0) DLPH(8);
        }
        if (q_mine) {
            const float qa1 = __uint_as_float((unsigned)va), qb1 = __uint_as_float((unsigned)vb);
            const float inv_d = 1.0f / (float)(H * 64);
            const float ps1 = (lane < TD ? __uint_as_float((unsigned)v00) : 0.f) + (lane + 64 < TD ? __uint_as_float((unsigned)v10) : 0.f);
            const float ps2 = (lane < TD ? __uint_as_float((unsigned)v01) : 0.f) + (lane + 64 < TD ? __uint_as_float((unsigned)v11) : 0.f);
            const float mean = wave_sum(ps1) * inv_d;
            const float var = fmaxf(wave_sum(ps2) * inv_d - mean * mean, 0.f);
            const float rstd = 1.0f / sqrtf(var + 1e-5f);
            c_q[wave * 64 + lane] = ((qa1 + qb1) - mean * qw1) * rstd + qc1;
        }
        DLPHV(13, npoll);
    }
    DLPH(9);
    dl_barrier();
    DLPH(10);
    // the wave's rows of group 0's two items: out of LDS, into the registers the items read them from
#pragma unroll
    for (int idx = 0; idx < 16; ++idx) {
        const uint4 t = *(const uint4*)(kvL + ((size_t)(wave * 16 + idx) * 64 + lane) * 16);
        if ((idx >> 2) & 1) vr[idx >> 3][idx & 3].a = t; else kr[idx >> 3][idx & 3].a = t;
    }
    dl_cross_items(p, it, kr, vr, grp, gw, gt, lane, c_q, c_smax, c_redl, c_red);
}
#undef DL_KV_LOAD
#endif  // CW_EXPERIMENTS (stage A)

// A V-tile block of qkv_self_kernel<.., XQ> (blocks 2 D/16 .. 3 D/16 - 1: they never carry an attention item and finish long before the
// item blocks, DESIGN.md 6g'''): its q/k/v tile exactly as in the kernel below, then tile (block - 2 D/16) of the cross-query x term
//     qa = W'q_c x + W'q_c bo
// from the rows of x the block already holds -- the x segment of gemv_stack_kernel<2, NSLOT, PER_LANE, 1> (decfuse.hip) operation for
// operation: rows rounded as x - mean(x) where |mean| >= std, the same K steps per wave, MFMA order and cross-wave sum, mean * (W'q_c 1)
// added back in f32.  A path of its own from the block's first instruction, so that every counted wait is exact: the extra tile's weights
// are requested BEHIND the first tile's (whose data therefore return first) and are waited for only after the V granules are out.
// The second 16-bit image of the rows takes the place of the first once every wave's MFMAs have read that one.
template <int NSLOT, int PER_LANE, bool WNT>
__device__ __forceinline__ void qs_vtile_xq_block(const float* __restrict__ x, const void* __restrict__ Wp, const float* __restrict__ bias,
                                                  void* sv, const int* __restrict__ pos, int Mb, int H, int K, int cap,
                                                  const QkvSelfParams& p, unsigned char* qsm) {
    const int xs_stride = K + 8;
    bf16_t* xs = (bf16_t*)qsm;                                       // [16][K+8]
    float* red = (float*)(qsm + (size_t)16 * xs_stride * 2);         // [4 waves][4][64]
    float* smean = red + 4 * 4 * 64;                                 // [16] (where an item block keeps its query)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 0..7 (waves 4..7 only keep the barriers' count)
    const int l15 = lane & 15, g = lane >> 4;
    const int bid = blockIdx.x;
    const int steps = K >> 7, nvec = K >> 2;
    const int nn = bid * 16 + l15;                                   // a V column: 2 K <= nn < 3 K
    const int tx = bid - 2 * (K >> 4), nx = tx * 16 + l15;           // tile and column of qa
    float bias_v = 0.f, xbias_v = 0.f, xwsum_v = 0.f;
    int pos_m = 0;
    float4 xv[2][PER_LANE];
    dl_u32x4_t wq[NSLOT][4], wx[NSLOT][4];
    if (wave < 4) {
        pos_m = pos[min(g * 4 + wave, Mb - 1)];
        bias_v = bias ? bias[nn] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int row = wave + 4 * i;
            row = row < Mb ? row : Mb - 1;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                int v4 = lane + 64 * c;
                v4 = v4 < nvec ? v4 : nvec - 1;
                xv[i][c] = *(const float4*)(x + (size_t)row * K + v4 * 4);
            }
        }
        const bf16_t* __restrict__ W = (const bf16_t*)Wp;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            int step = wave + 4 * s;
            step = step < steps ? step : steps - 1;
            const dl_u32x4_t* wp = (const dl_u32x4_t*)(W + ((((size_t)bid * (K >> 5)) + step * 4) * 64 + lane) * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) wq[s][j] = WNT ? CW_STREAM_LD(wp + j * 64) : wp[j * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        // the extra tile's requests: their addresses come from `p`, which arrives under the requests above.  Unconditional (a row sum
        // that is not wanted reads the bias instead: a load under a branch would make the counted waits conservative)
        const bf16_t* __restrict__ WX = (const bf16_t*)p.xq_W;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            int step = wave + 4 * s;
            step = step < steps ? step : steps - 1;
            const dl_u32x4_t* wp = (const dl_u32x4_t*)(WX + ((((size_t)tx * (K >> 5)) + step * 4) * 64 + lane) * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) wx[s][j] = WNT ? CW_STREAM_LD(wp + j * 64) : wp[j * 64];
        }
        xbias_v = p.xq_bias[nx];
        xwsum_v = (p.xq_wsum ? p.xq_wsum : p.xq_bias)[nx];
    }
    __builtin_amdgcn_sched_barrier(0);
    const unsigned tag = (p.epoch[0] << 6) | (unsigned)p.layer;
    const bool center = p.xq_wsum != nullptr;                        // block-uniform; read here: `p` must not be waited for in front of the first request
    asm volatile("" : "+v"(pos_m));

    // ---- the V tile: LayerNorm, rows -> 16 bit -> LDS, MFMA, cross-wave sum, cache row and granules (qkv_self_kernel's own lines)
    if (wave < 4) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float sx = 0.f;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                const float ok = (lane + 64 * c < nvec) ? 1.f : 0.f;
                sx += ok * ((xv[i][c].x + xv[i][c].y) + (xv[i][c].z + xv[i][c].w));
            }
            const float mean = wave_sum(sx) / (float)K;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                const float ok = (lane + 64 * c < nvec) ? 1.f : 0.f;
                const float a = xv[i][c].x - mean, b = xv[i][c].y - mean, cc = xv[i][c].z - mean, d = xv[i][c].w - mean;
                q += ok * cw_sumsq4(a, b, cc, d);
            }
            const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + 1e-5f);
            const int row = wave + 4 * i;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                int v4 = lane + 64 * c;
                v4 = v4 < nvec ? v4 : nvec - 1;
                ushort4 o;
                o.x = f32_to_bf16((xv[i][c].x - mean) * rstd); o.y = f32_to_bf16((xv[i][c].y - mean) * rstd);
                o.z = f32_to_bf16((xv[i][c].z - mean) * rstd); o.w = f32_to_bf16((xv[i][c].w - mean) * rstd);
                *(ushort4*)(xs + (size_t)row * xs_stride + v4 * 4) = o;
            }
        }
    }
    dl_barrier();
    if (wave < 4) {
        f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            const int step = wave + 4 * s;
            if (step < steps) {
                const bf16_t* xr = xs + (size_t)l15 * xs_stride + step * 128 + g * 8;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
                    acc = cw_mfma_16x16x32(a, __builtin_bit_cast(bf16x8_t, wq[s][j]), acc);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    }
    dl_barrier();                                                    // every wave's MFMAs have read the first image: xs is free
    if (wave < 4) {
        const int r = wave;
        const float v = (red[(0 * 4 + r) * 64 + lane] + red[(1 * 4 + r) * 64 + lane] + red[(2 * 4 + r) * 64 + lane] + red[(3 * 4 + r) * 64 + lane]) + bias_v;
        const int m = g * 4 + r;
        const int rc = nn - 2 * K;
        const unsigned h16 = f32_to_bf16(v);
        const unsigned other = (unsigned)__shfl_xor((int)h16, 1, 64);          // the neighbouring column's 16 bits
        if (m < Mb) {
            const int hh = rc >> 6, dd = rc & 63;
            if (!(l15 & 1)) dl_gran_st(p.gkv + ((size_t)16 + m) * (K >> 1) + (rc >> 1), tag, h16 | (other << 16));   // the hand-off first
            ((bf16_t*)sv)[(((size_t)m * H + hh) * cap + pos_m) * 64 + dd] = (bf16_t)h16;
        }
        // ---- the second image: gemv_stack_kernel's rounding of its x segment
        if (center) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
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
#pragma unroll
        for (int i = 0; i < 2; ++i) {
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
    }
    dl_barrier();                                                    // the second image is whole, and the first epilogue has read `red`
    if (wave < 4) {
        f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            const int step = wave + 4 * s;
            if (step < steps) {
                const bf16_t* xr = xs + (size_t)l15 * xs_stride + step * 128 + g * 8;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
                    acc = cw_mfma_16x16x32(a, __builtin_bit_cast(bf16x8_t, wx[s][j]), acc);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    }
    dl_barrier();
    if (wave < 4) {
        const int r = wave;
        const float v = red[(0 * 4 + r) * 64 + lane] + red[(1 * 4 + r) * 64 + lane] + red[(2 * 4 + r) * 64 + lane] + red[(3 * 4 + r) * 64 + lane];
        const int m = g * 4 + r;
        if (m < Mb) {
            const float back = center ? smean[m] * xwsum_v : 0.f;
            p.xq_out[(size_t)m * K + nx] = v + xbias_v + back;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// q/k/v projection + self-attention in ONE launch (rows <= 8): grid = 3 D / 16 tiles, 512 threads.
//   waves 0..3 of block t: the LayerNorm + GEMV tile t of gemv2_bf16_kernel<EPI_QKV_CACHE, 2, false, false, NSLOT, PER_LANE>
//   (gemm.hip), operation for operation; the epilogue appends k / v to the self-attention cache as before AND publishes the
//   tile as granules (q: one f32 per granule; k, v: two 16-bit cache values per granule);
//   all 8 waves of block i < rows x heads: attn_decode_kernel<T, false> (attention.hip) for (head i % H, row i / H): the K / V
//   rows of the history are requested at kernel entry (they depend on nothing), the query and THIS step's key / value row come
//   from the granules of the 12 tiles of the head, polled by wave 4 (whose memory queue holds nothing else by then).
// Unlike stage A above the hand-off happens on a quiet memory system: every block has taken in its 80 KB before anybody polls.
// Producers never wait, consumers wait only after they have produced.  RESIDENCY: block i < rows x heads waits for tiles up to
// 3 D / 16 - 1, so all 240 blocks (122 k threads of the chip's 524 k) must get a slot while the first ones poll.  Alone on the GPU
// they always do.  When several processes share it (tests/test_dist_gloo.py runs eight ranks on one device) the polling blocks of
// all of them can hold every slot, the polls run into DL_SPIN_LIMIT and set `err`; the engine then repeats the call with the
// two-launch path (bit-identical) and keeps this context on it (engine.hip: handoff_gave_up).  Two block orders that need no
// co-residency were measured and rejected: item blocks behind all tile blocks 8.35 us per launch (7.9 as it is; the XCDs dispatch
// their shares of a grid independently, so even that order is not a guarantee across processes), items behind the tiles of
// their head 10.7 us.
// ---------------------------------------------------------------------------------------------------
#define QS_THREADS 512
#define QS_GROUPS (QS_THREADS / 8)
#define QS_PRE 2

// WNT: the tiles' weight stream with non-temporal loads (tile t has one reading block: block t).  The granule loads and stores keep their policy.
// Kernel arguments (DESIGN.md 6g''): eight plain values of 14 dwords lead -- preloaded into user SGPRs at dispatch by the file's
// -amdgpu-kernarg-preload-count -- and every request of the entry (cache row, bias, rows, weights, history) is addressed from them alone;
// `p` (a by-value struct is never preloaded, and ends the preloaded run) arrives under those requests.  cw_launch_qkv_self fills both
// from the one struct:  x, Wp, bias, sk, sv, pos = the fields of `p`;  dims = p.Mb | p.H << 8 | p.D << 16;  cap = p.cap
// XQ: the V-tile blocks also compute the cross-query x term and the item blocks also leave their output rows in 16 bits (p.xq_*, p.out16)
template <int NSLOT, int PER_LANE, bool WNT, bool XQ>
__global__ __launch_bounds__(QS_THREADS) void qkv_self_kernel(const float* __restrict__ x, const void* __restrict__ Wp,
                                                              const float* __restrict__ bias, void* sk, void* sv,
                                                              const int* __restrict__ pos, unsigned dims, int cap, QkvSelfParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qsm[];
    const int Mb = (int)(dims & 0xffu), H = (int)((dims >> 8) & 0xffu), K = (int)(dims >> 16), N = 3 * K;
    if (XQ && (int)blockIdx.x >= 2 * (K >> 4)) {                      // block-uniform, decided from preloaded arguments
        qs_vtile_xq_block<NSLOT, PER_LANE, WNT>(x, Wp, bias, sv, pos, Mb, H, K, cap, p, qsm);
        return;
    }
    const int xs_stride = K + 8;
    bf16_t* xs = (bf16_t*)qsm;                                       // [16][K+8]
    float* red = (float*)(qsm + (size_t)16 * xs_stride * 2);         // [4 waves][4][64]
    float* s_q = red + 4 * 4 * 64;                                   // [64] query of the item
    bf16_t* s_kn = (bf16_t*)(s_q + 64);                              // [64] this step's key row, [64] value row
    bf16_t* s_vn = s_kn + 64;
    float* dsm = (float*)(s_vn + 64);                                // attn_decode_kernel's scratch: scores [cap rounded] | red [64][64] | scratch [64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 0..7
    const int l15 = lane & 15, g = lane >> 4;
    const int bid = blockIdx.x;
    const int n0 = bid * 16;
    const int steps = K >> 7, nvec = K >> 2;
    const int nn = n0 + l15, ncl = nn < N ? nn : N - 1;

    // ---- self-attention item of this block (if any): history rows first into the queue?  No: the tile's loads go first, they
    // are the critical path of every OTHER block's item as well
    const int n_items = Mb * H;
    const bool has_item = bid < n_items;
    const int ih = has_item ? bid % H : 0, ib = has_item ? bid / H : 0;
    const int sub = tid & 7, grp = tid >> 3;
    const bf16_t* Kh = (const bf16_t*)sk + ((size_t)ib * H + ih) * cap * 64;
    const bf16_t* Vh = (const bf16_t*)sv + ((size_t)ib * H + ih) * cap * 64;

    float bias_v = 0.f;
    int pos_m = 0;                                                   // cache row of tile row m = g * 4 + wave (waves 0..3): FIRST in the queue --
    float4 xv[2][PER_LANE];                                          // vmcnt retires in order, and behind the history rows its wait would be vmcnt(0)
    dl_u32x4_t wq[NSLOT][4];
    if (wave < 4) {
        pos_m = pos[min(g * 4 + wave, Mb - 1)];
        bias_v = bias ? bias[ncl] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int row = wave + 4 * i;
            row = row < Mb ? row : Mb - 1;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                int v4 = lane + 64 * c;
                v4 = v4 < nvec ? v4 : nvec - 1;
                xv[i][c] = *(const float4*)(x + (size_t)row * K + v4 * 4);
            }
        }
        const bf16_t* __restrict__ W = (const bf16_t*)Wp;
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            int step = wave + 4 * s;
            step = step < steps ? step : steps - 1;
            const dl_u32x4_t* wp = (const dl_u32x4_t*)(W + ((((size_t)(ncl >> 4) * (K >> 5)) + step * 4) * 64 + g * 16 + (ncl & 15)) * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) wq[s][j] = WNT ? CW_STREAM_LD(wp + j * 64) : wp[j * 64];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    DlRaw8 kpre[QS_PRE], vpre[QS_PRE];
#pragma unroll
    for (int u = 0; u < QS_PRE; ++u) kpre[u].ld(Kh + (size_t)min(grp + u * QS_GROUPS, cap - 1) * 64 + sub * 8);
#pragma unroll
    for (int u = 0; u < QS_PRE; ++u) vpre[u].ld(Vh + (size_t)min(grp + u * QS_GROUPS, cap - 1) * 64 + sub * 8);
    const int n_keys = pos[ib] + 1;
    // (the position the give-up word needs, requested here with everything else: at its use it is a scalar round trip in front of wave
    // 4's first poll.  The epilogue's cache row pos_m is requested at the head of the queue above: left at its use it was a dependent
    // load + `s_waitcnt vmcnt(0)` in front of the granule stores, the hand-off every attention item waits for)
    const int pos0 = pos[0];
    __builtin_amdgcn_sched_barrier(0);
    const unsigned tag = (p.epoch[0] << 6) | (unsigned)p.layer;       // from `p`: behind every request of the entry
    asm volatile("" : "+v"(pos_m));                                  // (pins the first use behind the fence: hipcc otherwise sign-extends it -- and waits for it -- in front of the history requests)

    // ---- tile: LayerNorm (gamma / beta folded into W / bias), rows -> 16 bit -> LDS, MFMA, cross-wave sum
    if (wave < 4) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float sx = 0.f;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                const float ok = (lane + 64 * c < nvec) ? 1.f : 0.f;
                sx += ok * ((xv[i][c].x + xv[i][c].y) + (xv[i][c].z + xv[i][c].w));
            }
            const float mean = wave_sum(sx) / (float)K;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                const float ok = (lane + 64 * c < nvec) ? 1.f : 0.f;
                const float a = xv[i][c].x - mean, b = xv[i][c].y - mean, cc = xv[i][c].z - mean, d = xv[i][c].w - mean;
                q += ok * cw_sumsq4(a, b, cc, d);
            }
            const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + 1e-5f);
            const int row = wave + 4 * i;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                int v4 = lane + 64 * c;
                v4 = v4 < nvec ? v4 : nvec - 1;
                ushort4 o;
                o.x = f32_to_bf16((xv[i][c].x - mean) * rstd); o.y = f32_to_bf16((xv[i][c].y - mean) * rstd);
                o.z = f32_to_bf16((xv[i][c].z - mean) * rstd); o.w = f32_to_bf16((xv[i][c].w - mean) * rstd);
                *(ushort4*)(xs + (size_t)row * xs_stride + v4 * 4) = o;
            }
        }
    }
    dl_barrier();
    if (wave < 4) {
        f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) {
            const int step = wave + 4 * s;
            if (step < steps) {
                const bf16_t* xr = xs + (size_t)l15 * xs_stride + step * 128 + g * 8;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
                    acc = cw_mfma_16x16x32(a, __builtin_bit_cast(bf16x8_t, wq[s][j]), acc);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 4 + r) * 64 + lane] = acc[r];
    }
    dl_barrier();
    if (wave < 4) {
        const int r = wave;
        const float v = (red[(0 * 4 + r) * 64 + lane] + red[(1 * 4 + r) * 64 + lane] + red[(2 * 4 + r) * 64 + lane] + red[(3 * 4 + r) * 64 + lane]) + bias_v;
        const int m = g * 4 + r;
        // EPI_QKV_CACHE: which == 0 -> the query (f32), 1 / 2 -> row pos[m] of the self-attention cache (16 bit)
        const int which = nn / K, rc = nn - which * K;
        unsigned h16 = 0;
        if (which != 0) h16 = f32_to_bf16(v);
        const unsigned other = (unsigned)__shfl_xor((int)h16, 1, 64);          // the neighbouring column's 16 bits
        if (m < Mb && nn < N) {
            if (which == 0) {
                dl_gran_st(p.gq + (size_t)m * K + rc, tag, __float_as_uint(v));
                if (p.q_plain) p.q_plain[(size_t)m * K + rc] = v;
            } else {
                const int hh = rc >> 6, dd = rc & 63;
                bf16_t* base = (bf16_t*)(which == 1 ? sk : sv);
                if (!(l15 & 1)) dl_gran_st(p.gkv + ((size_t)(which - 1) * 16 + m) * (K >> 1) + (rc >> 1), tag, h16 | (other << 16));   // the hand-off first
                base[(((size_t)m * H + hh) * cap + pos_m) * 64 + dd] = (bf16_t)h16;
            }
        }
    }
    if (!has_item || p.no_attn) return;                               // (no barrier follows for the block as a whole)

    // ---- the item: wave 4 gathers the query and this step's key / value row of (row ib, head ih)
    if (wave == 4) {
        const dl_u64_t* gqp = p.gq + (size_t)ib * K + ih * 64 + lane;
        const dl_u64_t* gkp = p.gkv + ((size_t)(lane >> 5) * 16 + ib) * (K >> 1) + ih * 32 + (lane & 31);
        dl_u64_t vq = 0, vk = 0;
        bool ready = false;
        // `err` holds 1 + the decoder position of the FIRST forward in which a wait gave up (0: none): forwards run one after the
        // other and the first writer wins, so everything before that position is good and the engine resumes there on the
        // launch-per-stage kernels (engine.hip: decode_once).  Once it is set every later wait gives up after at most 256 polls
        // instead of DL_SPIN_LIMIT: those forwards are discarded anyway.
        const int give_up_tag = pos0 + 1;
        const bool forced_fail = p.fail_pos >= 0 && pos0 == p.fail_pos && p.layer == 0;   // test hook (cw_test_set_option "handoff_fail_pos")
#pragma unroll 1
        for (int spins = 0; !ready; ++spins) {
            if (forced_fail || spins > DL_SPIN_LIMIT || ((spins & 255) == 255 && __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                if (lane == 0) atomicCAS(p.err, 0, give_up_tag);
                if (forced_fail) { vq = 0x3f800000ull; vk = 0; }     // the garbage a starved poll would leave
                break;
            }
            vq = dl_gran_ld(gqp); vk = dl_gran_ld(gkp);
            ready = __all((unsigned)(vq >> 32) == tag && (unsigned)(vk >> 32) == tag);
        }
        s_q[lane] = __uint_as_float((unsigned)vq);
        ((unsigned*)s_kn)[lane] = (unsigned)vk;                      // lanes 0..31: key pairs, 32..63: value pairs (s_vn follows s_kn)
    }
    dl_barrier();
    // ---- attn_decode_kernel<T, false> from here on, with the row at n_keys - 1 taken from LDS instead of the cache (another
    // CU wrote it a microsecond ago with plain stores: not visible to this CU's loads)
    float* sc = dsm;
    float* redd = dsm + ((cap + 63) & ~63);
    float* scratch = redd + QS_GROUPS * 64;
    float qv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = s_q[sub * 8 + e];
    const int kn = n_keys - 1;
    const uint4 kn_raw = *(const uint4*)(s_kn + sub * 8), vn_raw = *(const uint4*)(s_vn + sub * 8);
#pragma unroll
    for (int u = 0; u < QS_PRE; ++u)
        if (grp + u * QS_GROUPS == kn) { kpre[u].a = kn_raw; vpre[u].a = vn_raw; }

    if (n_keys <= QS_PRE * QS_GROUPS) {
        float* s_max = scratch;
        float* red8 = redd;
        float d[QS_PRE], mxl = -INFINITY;
#pragma unroll
        for (int u = 0; u < QS_PRE; ++u) {
            float kv[8];
            kpre[u].cvt(kv);
            float t = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) t = fmaf(qv[e], kv[e], t);
            t += __shfl_xor(t, 1, 64); t += __shfl_xor(t, 2, 64); t += __shfl_xor(t, 4, 64);
            d[u] = (grp + u * QS_GROUPS < n_keys) ? t : -INFINITY;
            mxl = fmaxf(mxl, d[u]);
        }
        mxl = wave_max(mxl);
        if (lane == 0) s_max[wave] = mxl;
        dl_barrier();
        mxl = s_max[0];
#pragma unroll
        for (int w = 1; w < QS_THREADS / 64; ++w) mxl = fmaxf(mxl, s_max[w]);
        float acc[8] = {};
        float lsum = 0.f;
#pragma unroll
        for (int u = 0; u < QS_PRE; ++u) {
            if (grp + u * QS_GROUPS < n_keys) {
                const float pk = expf(d[u] - mxl);
                if (sub == 0) lsum += pk;
                float vv[8];
                vpre[u].cvt(vv);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, vv[e], acc[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = acc[e] + dpp_mov<0x128, 0xf>(0.f, acc[e]);
            acc[e] = xor32_sum(xor16_sum(v));
        }
        lsum = wave_sum(lsum);
        if (lane < 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red8[wave * 64 + sub * 8 + e] = acc[e];
        }
        if (lane == 0) red8[8 * 64 + wave] = lsum;
        dl_barrier();
        if (tid < 64) {
            float r = 0.f, l = 0.f;
#pragma unroll
            for (int w = 0; w < QS_THREADS / 64; ++w) { r += red8[w * 64 + tid]; l += red8[8 * 64 + w]; }
            r *= 1.0f / l;
            p.out[(size_t)ib * H * 64 + ih * 64 + tid] = r;
            if (XQ) ((bf16_t*)p.out16)[(size_t)ib * H * 64 + ih * 64 + tid] = f32_to_bf16(r);   // the rounding gemv_stack_kernel applies to the f32 row
        }
        return;
    }

    // long history (> 128 keys): scores through LDS, the remaining rows four at a time
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < QS_PRE; ++u) {
        const int k = grp + u * QS_GROUPS;
        float kv[8];
        kpre[u].cvt(kv);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(qv[e], kv[e], d);
        d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
        if (k < n_keys) {
            if (sub == 0) sc[k] = d;
            mx = fmaxf(mx, d);
        }
    }
    for (int k0 = grp + QS_PRE * QS_GROUPS; k0 < n_keys; k0 += 4 * QS_GROUPS) {
        float kv[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = min(k0 + u * QS_GROUPS, n_keys - 1);
            uint4 raw = *(const uint4*)(Kh + (size_t)k * 64 + sub * 8);
            if (k == kn) raw = kn_raw;
            h16_unpack8(raw, kv[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * QS_GROUPS;
            if (k < n_keys) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(qv[e], kv[u][e], d);
                d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
                if (sub == 0) sc[k] = d;
                mx = fmaxf(mx, d);
            }
        }
    }
    mx = block_max(mx, scratch);
    float sum = 0.f;
    for (int k = tid; k < n_keys; k += QS_THREADS) { float e = expf(sc[k] - mx); sc[k] = e; sum += e; }
    sum = block_sum(sum, scratch);
    const float inv = 1.0f / sum;
    float acc[8] = {};
#pragma unroll
    for (int u = 0; u < QS_PRE; ++u) {
        const int k = grp + u * QS_GROUPS;
        float vv[8];
        vpre[u].cvt(vv);
        const float pk = (k < n_keys) ? sc[k] * inv : 0.f;
        if (k < n_keys) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, vv[e], acc[e]);
        }
    }
    for (int k0 = grp + QS_PRE * QS_GROUPS; k0 < n_keys; k0 += 4 * QS_GROUPS) {
        float vv[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = min(k0 + u * QS_GROUPS, n_keys - 1);
            uint4 raw = *(const uint4*)(Vh + (size_t)k * 64 + sub * 8);
            if (k == kn) raw = vn_raw;
            h16_unpack8(raw, vv[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * QS_GROUPS;
            if (k < n_keys) {
                const float pk = sc[k] * inv;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pk, vv[u][e], acc[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) redd[grp * 64 + sub * 8 + e] = acc[e];
    __syncthreads();
    if (tid < 64) {
        float r = 0.f;
        for (int gI = 0; gI < QS_GROUPS; ++gI) r += redd[gI * 64 + tid];
        p.out[(size_t)ib * H * 64 + ih * 64 + tid] = r;
        if (XQ) ((bf16_t*)p.out16)[(size_t)ib * H * 64 + ih * 64 + tid] = f32_to_bf16(r);
    }
}

// blocks of qkv_self_kernel a CU holds at once (LDS and thread limits); the engine enables the kernel only where the whole grid --
// 3 D / 16 blocks that wait for each other -- is resident at once on an otherwise idle chip
int cw_qkv_self_blocks_per_cu(int D, int cap) {
    const size_t lds = (size_t)16 * (D + 8) * 2 + (size_t)(4 * 4 * 64 + 64) * 4 + 2 * 64 * 2 + ((size_t)((cap + 63) & ~63) + QS_GROUPS * 64 + 64) * 4;
    const int by_lds = (int)((size_t)160 * 1024 / lds), by_threads = 2048 / QS_THREADS;
    return by_lds < by_threads ? by_lds : by_threads;
}

int cw_launch_qkv_self(const QkvSelfParams& p, hipStream_t st) {
    const int D = p.D;
    if (p.Mb < 1 || p.Mb > 8 || D % 128 || D > 1280 || p.H * 64 != D || p.cap < 1 || p.cap > 512) return CW_ERR_INVALID;
    if (p.Mb * p.H > 3 * (D / 16) || !p.gq || !p.gkv || !p.epoch || !p.err || !p.W || !p.x || !p.pos) return CW_ERR_INVALID;
    if (p.layer < 0 || p.layer >= 64) return CW_ERR_INVALID;          // the granule tag is (epoch << 6) | layer
    if (p.xq_W && (!p.xq_out || !p.xq_bias || !p.out16 || p.no_attn || p.Mb * p.H > 2 * (D / 16))) return CW_ERR_INVALID;   // (the V-tile blocks carry no item)
    const size_t lds = (size_t)16 * (D + 8) * 2 + (size_t)(4 * 4 * 64 + 64) * 4 + 2 * 64 * 2 +
                       ((size_t)((p.cap + 63) & ~63) + QS_GROUPS * 64 + 64) * 4;
    const dim3 grid(3 * (D / 16));
#define QS_LAUNCH_P(NS, PL, NTL, XQ)                                                                                            \
    do {                                                                                                                     \
        static std::once_flag attr;                                                                                          \
        std::call_once(attr, [] { (void)hipFuncSetAttribute((const void*)qkv_self_kernel<NS, PL, NTL, XQ>, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024); }); \
        hipLaunchKernelGGL((qkv_self_kernel<NS, PL, NTL, XQ>), grid, dim3(QS_THREADS), lds, st, p.x, p.W, p.bias, p.sk, p.sv, p.pos, \
                           (unsigned)p.Mb | (unsigned)p.H << 8 | (unsigned)D << 16, p.cap, p);                                \
    } while (0)
#define QS_LAUNCH(NS, PL)                                                                                                   \
    do {                                                                                                                     \
        if (p.xq_W) { if (p.wnt) QS_LAUNCH_P(NS, PL, true, true); else QS_LAUNCH_P(NS, PL, false, true); }                   \
        else { if (p.wnt) QS_LAUNCH_P(NS, PL, true, false); else QS_LAUNCH_P(NS, PL, false, false); }                        \
    } while (0)
    if (D <= 256) QS_LAUNCH(1, 1);
    else if (D <= 768) QS_LAUNCH(2, 3);
    else QS_LAUNCH(3, 5);
#undef QS_LAUNCH
#undef QS_LAUNCH_P
    return CW_OK;
}

#ifdef CW_EXPERIMENTS   // fc1 + fc2 in one launch: measured slower (profiles/r05_mlp_chain_phases.txt); A/B builds only (CW_MLP_CHAIN=1)
// ---------------------------------------------------------------------------------------------------
// fc1 + fc2 in ONE launch (rows <= 8): grid = F / 32 fc1 blocks, then (D / 32) x KS fc2 blocks, 256 threads.
//   fc1 block j:  LayerNorm + two 16-column tiles + GELU of gemv2_bf16_kernel<EPI_GELU, 2, false, false, NS1, PL1, 2> (gemm.hip),
//                 operation for operation; the 16-bit rows leave as write-through (sc1) 4-byte stores; when the block's stores have
//                 drained (vmcnt 0 + block barrier) thread 0 publishes flag j = {tag, 1};
//   fc2 block:    gemv2_bf16_kernel<EPI_RESID_F32, 2, true, false, NS2, .., 2, true> for (column pair, K slice): its 64-80 KB of
//                 weights are requested at kernel entry (they depend on nothing), wave 0 then polls the F / 32 flags, and the rows of
//                 the K slice come in by 8-byte sc1 loads (another CU wrote them a microsecond ago: plain loads could hit a stale L2 line).
// ALL fc1 flags are awaited, not just the 32 producers of the K slice: fc2 accumulates into the residual rows fc1 reads, in place,
// and every fc1 block must have taken its copy first.  A kernel boundary without the boundary: no launch, no cold weight stream
// behind it (MI355X_MICROARCH.md, rows handoff-flag / prefetch-credit).  Blocks are dispatched in index order, producers never wait,
// consumers wait only for lower-numbered blocks: no residency requirement.
// MEASURED (profiles/r05_mlp_chain_phases.txt): 13.1 us against 5.7 + 4.9 for the two launches.  The write-through stores of the
// slowest fc1 block take 2.8 us to drain, the flags are seen 1.5 us after that, the rows arrive 0.55 us later: 4.5-5 us from
// "rows stored" to "rows in the consumer's LDS", where a kernel boundary + cold weight stream costs ~3.  A/B only (CW_MLP_CHAIN=1).
// Bit-identical to the two launches (same K slices, same
// summation orders; the residual updates are on the 2^-12 grid, so the order of the atomics does not matter).
// ---------------------------------------------------------------------------------------------------
template <int NS1, int PL1, int NS2>
__global__ __launch_bounds__(256) void mlp_chain_kernel(MlpChainParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int D = p.D, F = p.F, Mb = p.Mb;
    const int n1 = F >> 5;
    const unsigned tag = (p.epoch[0] << 6) | (unsigned)p.layer;
    const int bid = blockIdx.x;
    constexpr int NT = 2;
    if (bid < n1) {
        // ================= fc1: LN + GEMV tile pair + GELU =================
        DLPH(0);
        const int K = D, N = F;
        const int xs_stride = K + 8;
        bf16_t* xs = (bf16_t*)msm;                                  // [16][K+8]
        float* red = (float*)(msm + (size_t)16 * xs_stride * 2);     // [4 waves][NT][4][64]
        const int n0 = bid * 16 * NT;
        const int steps = K >> 7, nvec = K >> 2;
        int nn[NT], ncl[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { nn[t] = n0 + t * 16 + l15; ncl[t] = nn[t] < N ? nn[t] : N - 1; }
        float bias_v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bias_v[t] = p.b1 ? p.b1[ncl[t]] : 0.f;
        float4 xv[2][PL1];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int row = wave + 4 * i;
            row = row < Mb ? row : Mb - 1;
#pragma unroll
            for (int c = 0; c < PL1; ++c) {
                int v4 = lane + 64 * c;
                v4 = v4 < nvec ? v4 : nvec - 1;
                xv[i][c] = *(const float4*)(p.x + (size_t)row * K + v4 * 4);
            }
        }
        dl_u32x4_t wq[NT][NS1][4];
        const bf16_t* __restrict__ W = (const bf16_t*)p.W1;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int s = 0; s < NS1; ++s) {
                int step = wave + 4 * s;
                step = step < steps ? step : steps - 1;
                const dl_u32x4_t* wp = (const dl_u32x4_t*)(W + ((((size_t)(ncl[t] >> 4) * (K >> 5)) + step * 4) * 64 + g * 16 + (ncl[t] & 15)) * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) wq[t][s][j] = wp[j * 64];
            }
        }
        DLPH(1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float sx = 0.f;
#pragma unroll
            for (int c = 0; c < PL1; ++c) {
                const float ok = (lane + 64 * c < nvec) ? 1.f : 0.f;
                sx += ok * ((xv[i][c].x + xv[i][c].y) + (xv[i][c].z + xv[i][c].w));
            }
            const float mean = wave_sum(sx) / (float)K;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < PL1; ++c) {
                const float ok = (lane + 64 * c < nvec) ? 1.f : 0.f;
                const float a = xv[i][c].x - mean, b = xv[i][c].y - mean, cc = xv[i][c].z - mean, d = xv[i][c].w - mean;
                q += ok * cw_sumsq4(a, b, cc, d);
            }
            const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + 1e-5f);
#pragma unroll
            for (int c = 0; c < PL1; ++c) {
                xv[i][c].x = (xv[i][c].x - mean) * rstd; xv[i][c].y = (xv[i][c].y - mean) * rstd;
                xv[i][c].z = (xv[i][c].z - mean) * rstd; xv[i][c].w = (xv[i][c].w - mean) * rstd;
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wave + 4 * i;
#pragma unroll
            for (int c = 0; c < PL1; ++c) {
                int v4 = lane + 64 * c;
                v4 = v4 < nvec ? v4 : nvec - 1;
                const float4 v = xv[i][c];
                ushort4 o;
                o.x = f32_to_bf16(v.x); o.y = f32_to_bf16(v.y); o.z = f32_to_bf16(v.z); o.w = f32_to_bf16(v.w);
                *(ushort4*)(xs + (size_t)row * xs_stride + v4 * 4) = o;
            }
        }
        DLPH(2);
        __syncthreads();
        DLPH(3);
        f32x4_t acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS1; ++s) {
            const int step = wave + 4 * s;
            if (step < steps) {
                const bf16_t* xr = xs + (size_t)l15 * xs_stride + step * 128 + g * 8;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = cw_mfma_16x16x32(a, __builtin_bit_cast(bf16x8_t, wq[t][s][j]), acc[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[((wave * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
        DLPH(4);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int r = wave;
            const float v = red[((0 * NT + t) * 4 + r) * 64 + lane] + red[((1 * NT + t) * 4 + r) * 64 + lane] +
                            red[((2 * NT + t) * 4 + r) * 64 + lane] + red[((3 * NT + t) * 4 + r) * 64 + lane];
            const int m = g * 4 + r, n = nn[t];
            const unsigned h16 = (unsigned)f32_to_bf16(gelu_erf(v + bias_v[t]));
            const unsigned other = (unsigned)__shfl_xor((int)h16, 1, 64);          // the neighbouring column's 16 bits
            if (m < Mb && n < N && !(l15 & 1))
                __hip_atomic_store((unsigned*)p.mid + (((size_t)m * F + n) >> 1), h16 | (other << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        DLPH(5);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's write-through stores have left the CU ...
        __syncthreads();                                               // ... and so have the other three waves'
        DLPH(6);
        if (tid == 0) dl_gran_st(p.flags + bid, tag, 1u);
        return;
    }
    // ================= fc2: K slice x column pair, weights first =================
    {
        const int K = F, N = D;
        const int nbx = N >> 5;
        const int fb = bid - n1, bx = fb % nbx, by = fb / nbx;
        DLPH(0);
        const int Kb = p.Kb2, kbase = by * Kb;
        const int xs_stride = Kb + 8;
        bf16_t* xs = (bf16_t*)msm;
        float* red = (float*)(msm + (size_t)16 * xs_stride * 2);
        const int n0 = bx * 16 * NT;
        const int steps = Kb >> 7;
        int nn[NT], ncl[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { nn[t] = n0 + t * 16 + l15; ncl[t] = nn[t] < N ? nn[t] : N - 1; }
        float bias_v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bias_v[t] = p.b2 ? p.b2[ncl[t]] : 0.f;
        // A/B (CW_MLP_CHAIN_DELAY, units of 64 clocks): hold the weight requests back so that fc1's loads go first
        for (int dly = p.delay; dly > 0; dly -= 64) __builtin_amdgcn_s_sleep(64);
        dl_u32x4_t wq[NT][NS2][4];
        const bf16_t* __restrict__ W = (const bf16_t*)p.W2;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int s = 0; s < NS2; ++s) {
                int step = wave + 4 * s;
                step = step < steps ? step : steps - 1;
                const dl_u32x4_t* wp = (const dl_u32x4_t*)(W + ((((size_t)(ncl[t] >> 4) * (K >> 5)) + (kbase >> 5) + step * 4) * 64 + g * 16 + (ncl[t] & 15)) * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) wq[t][s][j] = wp[j * 64];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        DLPH(1);
        // every fc1 block has published (and therefore read its copy of the residual rows): up to 512 flags, all eight loads of a
        // round in flight together
        if (wave == 0) {
            bool ready = false;
#pragma unroll 1
            for (int spins = 0; !ready; ++spins) {
                if (spins > DL_SPIN_LIMIT) { if (lane == 0) atomicCAS(p.err, 0, 1); break; }
                dl_u64_t f[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) f[q] = dl_gran_ld(p.flags + min(lane + 64 * q, n1 - 1));
                bool ok = true;
#pragma unroll
                for (int q = 0; q < 8; ++q) ok = ok && (unsigned)(f[q] >> 32) == tag;
                ready = __all(ok);
                if (!ready) __builtin_amdgcn_s_sleep(2);
            }
        }
        DLPH(7);
        __syncthreads();
        DLPH(8);
        // the 16-bit rows of the K slice: rows wave, wave + 4 (clamped like the launch path), 8 bytes per lane per load, every load
        // out before the first LDS write (Kb <= 1024: at most four per row)
        {
            const int per_row = Kb >> 8;
            dl_u64_t mv[2][4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = wave + 4 * i;
                const int rowc = row < Mb ? row : Mb - 1;
                const dl_u64_t* src = (const dl_u64_t*)((const bf16_t*)p.mid + (size_t)rowc * K + kbase);
#pragma unroll
                for (int c = 0; c < 4; ++c) mv[i][c] = dl_gran_ld(src + lane + 64 * min(c, per_row - 1));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = wave + 4 * i;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < per_row) *(dl_u64_t*)(xs + (size_t)row * xs_stride + (lane + 64 * c) * 4) = mv[i][c];
            }
        }
        DLPH(9);
        __syncthreads();
        f32x4_t acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS2; ++s) {
            const int step = wave + 4 * s;
            if (step < steps) {
                const bf16_t* xr = xs + (size_t)l15 * xs_stride + step * 128 + g * 8;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8_t a = *(const bf16x8_t*)(xr + j * 32);
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = cw_mfma_16x16x32(a, __builtin_bit_cast(bf16x8_t, wq[t][s][j]), acc[t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[((wave * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
        DLPH(10);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int r = wave;
            const float v = red[((0 * NT + t) * 4 + r) * 64 + lane] + red[((1 * NT + t) * 4 + r) * 64 + lane] +
                            red[((2 * NT + t) * 4 + r) * 64 + lane] + red[((3 * NT + t) * 4 + r) * 64 + lane];
            const int m = g * 4 + r, n = nn[t];
            if (m < Mb && n < N) atomicAdd(p.xio + (size_t)m * N + n, resid_grid(v + (by == 0 ? bias_v[t] : 0.f)));
        }
        DLPH(11);
    }
}

// K slices of fc2 exactly as launch_gemv2 (gemm.hip) picks them for the in-place residual GEMV with two column tiles per block
static int mlp_chain_ksplit(int D, int F) {
    int ks = 1;
    const int tiles = D / 16, steps = F / 128;
    while (tiles * ks < 256 && steps % (ks * 2) == 0 && steps / (ks * 2) >= 4) ks *= 2;
    while (F / ks > 1280) ks *= 2;
    for (int k2 = ks + 1; (D / 32) * k2 <= 256; ++k2) if (F % (k2 * 128) == 0) ks = k2;
    return ks;
}
bool cw_mlp_chain_ok(int Mb, int D, int F) {
    if (Mb < 1 || Mb > 8 || D % 128 || D <= 768 || D > 1280 || F % 256 || F <= 1280) return false;
    const int ks = mlp_chain_ksplit(D, F);
    if (F % ks || (F / ks) % 256 || F / ks > 1024 || F / ks < 512) return false;     // NS2 = 2 covers 5..8 K steps per slice
    // the launch path must make the same choices: two tiles per fc2 block (grid (D / 16) x ks > 256 blocks) and per fc1 block
    return (D / 16) * ks > 256 && (D / 32) * ks >= 128 && F / 16 > 256 && F / 32 >= 128 && F / 32 <= 512;
}

int cw_launch_mlp_chain(const MlpChainParams& p0, hipStream_t st) {
    MlpChainParams p = p0;
    if (!cw_mlp_chain_ok(p.Mb, p.D, p.F) || !p.flags || !p.epoch || !p.err || !p.mid || !p.x || !p.xio) return CW_ERR_INVALID;
    const int ks = mlp_chain_ksplit(p.D, p.F);
    p.Kb2 = p.F / ks;
    p.delay = cw_sw::cw_switches().mlp_chain_delay;
    const size_t lds1 = (size_t)16 * (p.D + 8) * 2 + 4 * 2 * 4 * 64 * 4, lds2 = (size_t)16 * (p.Kb2 + 8) * 2 + 4 * 2 * 4 * 64 * 4;
    const size_t lds = lds1 > lds2 ? lds1 : lds2;
    const dim3 grid(p.F / 32 + (p.D / 32) * ks);
    static std::once_flag attr;
    std::call_once(attr, [] { (void)hipFuncSetAttribute((const void*)mlp_chain_kernel<3, 5, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024); });
    hipLaunchKernelGGL((mlp_chain_kernel<3, 5, 2>), grid, dim3(256), lds, st, p);
    return CW_OK;
}

size_t cw_dec_layer_lds(int D) {
    return (size_t)16 * (D + 8) * 2 + (size_t)(4 * 4 * 64 + 16 + 32 + 32 + 4 * 64 + 4 * 8 * 64 + 4) * 4 + (size_t)4 * 16 * 1024;
}

// grid: one workgroup per CU (every workgroup must be resident: they wait for each other's granules)
int cw_launch_dec_layer(const DecLayerParams& p, int n_cu, hipStream_t st) {
    const int D = p.D;
    if (p.Mb < 1 || p.Mb > 8 || D % 128 || D > 1280 || p.H * 64 != D || n_cu < 1) return CW_ERR_INVALID;
    if (3 * (D / 16) > n_cu || p.Mb * p.H * ATT_NS > 4 * n_cu || D / 16 > 128) return CW_ERR_INVALID;
    if ((p.n_keys + ATT_NS - 1) / ATT_NS > 4 * 64 || p.n_keys < 1 || (ATT_NS - 1) * ((p.n_keys + ATT_NS - 1) / ATT_NS) >= p.n_keys) return CW_ERR_INVALID;
    if (!p.gq || !p.gps || !p.epoch || !p.err || !p.Ws || !p.qw || !p.qbias) return CW_ERR_INVALID;
    const size_t lds = cw_dec_layer_lds(D);
    if (lds > 160 * 1024) return CW_ERR_INVALID;
#define DL_LAUNCH(NS, PL, DP)                                                                                                    \
    do {                                                                                                                         \
        static std::once_flag attr;                                                                                              \
        std::call_once(attr, [] { (void)hipFuncSetAttribute((const void*)dec_layer_a_kernel<NS, PL, DP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }); \
        hipLaunchKernelGGL((dec_layer_a_kernel<NS, PL, DP>), dim3(n_cu), dim3(DL_THREADS), lds, st, p);                          \
    } while (0)
    // K/V rows in flight per lane of the twelve K/V waves (A/B: CW_DL_DEPTH = 4 | 8 | 16; 16 = everything at kernel entry, the default)
    const int depth = cw_sw::cw_switches().dl_depth;   // default 16
    if (D <= 256) DL_LAUNCH(1, 1, 16);
    else if (D <= 768) DL_LAUNCH(2, 3, 16);
    else if (depth == 4) DL_LAUNCH(3, 5, 4);
    else if (depth == 8) DL_LAUNCH(3, 5, 8);
    else DL_LAUNCH(3, 5, 16);
#undef DL_LAUNCH
    return CW_OK;
}

#else   // default build: the two measured-slower persistent stages are not compiled; the engine never selects them (cw_create refuses their switches)
bool cw_mlp_chain_ok(int, int, int) { return false; }
int cw_launch_mlp_chain(const MlpChainParams&, hipStream_t) { return CW_ERR_INVALID; }
size_t cw_dec_layer_lds(int) { return (size_t)1 << 30; }
int cw_launch_dec_layer(const DecLayerParams&, int, hipStream_t) { return CW_ERR_INVALID; }
#endif  // CW_EXPERIMENTS (mlp_chain_kernel, stage A launcher)

}  // namespace CW_NS
