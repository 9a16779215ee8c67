// Engine + C ABI (include/crisperwhisper.h): owns device memory, the HIP stream, the weights and the
// per-stage orchestration of the CrisperWhisper hot path on one MI355X.  No CPU fallbacks: every entry
// point either runs the HIP kernels or returns an error.
#include "engine_internal.h"

static thread_local char g_err[512] = "";

int fail(cw_ctx* c, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c ? c->err : g_err, 512, fmt, ap);
    va_end(ap);
    if (c) c->err_set = true;
    return code;
}
// outer frames keep the innermost message and only add one when the callee reported a bare code
int fail_ctx(cw_ctx* c, int code, const char* call, const char* file, int line) {
    if (c && c->err_set) return code;
    return fail(c, code, "%s -> %d (%s:%d)", call, code, file, line);
}

// host f32 -> device T (optionally scaled), at element offset `off` of dst
int upload_T(cw_ctx* c, void* dst, size_t off, const float* src, size_t n, float scale) {
    if (c->bf16) {
        std::vector<bf16_t> tmp(n);
        if (c->f16) for (size_t i = 0; i < n; ++i) tmp[i] = cw_host_f32_to_f16(src[i] * scale);
        else for (size_t i = 0; i < n; ++i) tmp[i] = cw_host_f32_to_bf16(src[i] * scale);
        HIPCHK(c, hipMemcpy((bf16_t*)dst + off, tmp.data(), n * 2, hipMemcpyHostToDevice));
    } else if (scale != 1.0f) {
        std::vector<float> tmp(n);
        for (size_t i = 0; i < n; ++i) tmp[i] = src[i] * scale;
        HIPCHK(c, hipMemcpy((float*)dst + off, tmp.data(), n * 4, hipMemcpyHostToDevice));
    } else {
        HIPCHK(c, hipMemcpy((float*)dst + off, src, n * 4, hipMemcpyHostToDevice));
    }
    return CW_OK;
}
static int upload_f32(cw_ctx* c, float* dst, size_t off, const float* src, size_t n, float scale = 1.0f) {
    if (scale != 1.0f) {
        std::vector<float> tmp(n);
        for (size_t i = 0; i < n; ++i) tmp[i] = src[i] * scale;
        HIPCHK(c, hipMemcpy(dst + off, tmp.data(), n * 4, hipMemcpyHostToDevice));
    } else {
        HIPCHK(c, hipMemcpy(dst + off, src, n * 4, hipMemcpyHostToDevice));
    }
    return CW_OK;
}
// device T -> host f32
int download_T(cw_ctx* c, const void* src, size_t off, float* dst, size_t n) {
    if (c->bf16) {
        std::vector<bf16_t> tmp(n);
        HIPCHK(c, hipMemcpy(tmp.data(), (const bf16_t*)src + off, n * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) dst[i] = c->f16 ? cw_host_f16_to_f32(tmp[i]) : cw_host_bf16_to_f32(tmp[i]);
    } else {
        HIPCHK(c, hipMemcpy(dst, (const float*)src + off, n * 4, hipMemcpyDeviceToHost));
    }
    return CW_OK;
}

#ifdef CW_EXPERIMENTS   // measured slower (profiles/r04_prefetch_side_stream_rejected.txt)
// Run-ahead prefetch of a decoder layer's HBM streams (weights + this batch's cross-attention K/V) into the Infinity Cache.
// A decode kernel's first bytes arrive 1.5-2 us after its launch when they come from HBM; on operands the previous launch left
// in the 256 MB Infinity Cache the same kernels run 0.7-1.5 us shorter each (tests/gpu_microbench.py).  The
// layer's 110 MB are therefore touched one layer ahead -- one 4-byte load per 64-byte sector, so the lines go HBM -> Infinity
// Cache and only 1/16 of the bytes travel on to the CU -- by a light launch on a side stream (a parallel branch of the captured
// step graph) that shares the CUs with the layer's own launches.
struct PrefetchRanges { const char* p[8]; unsigned long long n[8]; int count; };
template <int WIDE>
__global__ __launch_bounds__(256) void prefetch_kernel(PrefetchRanges r, unsigned int* sink) {
    unsigned int acc = 0;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthr = (size_t)gridDim.x * 256;
    for (int k = 0; k < r.count; ++k) {
        const char* base = r.p[k];
        if (WIDE) {                                               // every byte, 16 B per lane (A/B)
            const size_t chunks = r.n[k] >> 4;
            size_t s = tid;
            for (; s + 7 * nthr < chunks; s += 8 * nthr) {
                uint4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *(const uint4*)(base + ((s + u * nthr) << 4));
#pragma unroll
                for (int u = 0; u < 8; ++u) acc ^= v[u].x ^ v[u].w;
            }
            for (; s < chunks; s += nthr) acc ^= ((const uint4*)(base))[s].x;
        } else {
            const size_t sectors = r.n[k] >> 6;
            size_t s = tid;
            for (; s + 7 * nthr < sectors; s += 8 * nthr) {      // eight independent loads in flight per lane
                unsigned int v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *(const unsigned int*)(base + ((s + u * nthr) << 6));
#pragma unroll
                for (int u = 0; u < 8; ++u) acc ^= v[u];
            }
            for (; s < sectors; s += nthr) acc ^= *(const unsigned int*)(base + (s << 6));
        }
    }
    if (acc == 0x9e3779b9u && sink) *sink = acc;                  // keeps the loads alive; practically never taken
}


#endif

extern "C" {

int32_t cw_abi_version(void) { return 1; }

const char* cw_last_error(cw_ctx* ctx) {
    if (!ctx) return g_err;
    ctx->err_set = false;
    return ctx->err;
}

int32_t cw_sync(cw_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->st));
    return CW_OK;
}

static int create_impl(cw_ctx* c) {
    const cw_model_desc& d = c->d;
    const int D = d.d_model, H = d.n_heads, F = d.ffn_dim, V = d.vocab_size, Bm = d.max_batch;
    if (D != H * 64) return fail(c, CW_ERR_INVALID, "head_dim must be 64 (d_model=%d heads=%d)", D, H);
    if (D % 128 || F % 128) return fail(c, CW_ERR_INVALID, "d_model/ffn must be multiples of 128");
    // the mel stage runs at any filter count its launcher takes (80 mels: the checkpoints before large-v3); the encoder's conv1 is an
    // implicit GEMM over n_mels-wide rows and needs a multiple of 64: its weight is refused when it is loaded, and so is cw_encode
    if (d.n_mels < 1 || d.n_mels > 256) return fail(c, CW_ERR_INVALID, "n_mels=%d outside 1 .. 256", d.n_mels);
    if (Bm < 1 || Bm > 64) return fail(c, CW_ERR_INVALID, "max_batch must be in 1..64");
    if (d.max_target_positions > 512) return fail(c, CW_ERR_INVALID, "max_target_positions > 512 unsupported");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamCreate(&c->st));
    HIPCHK(c, hipEventCreate(&c->ev0));
    HIPCHK(c, hipEventCreate(&c->ev1));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_step[0], hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_step[1], hipEventDisableTiming));
#ifdef CW_EXPERIMENTS   // side stream of the rejected run-ahead prefetch (CW_PREFETCH)
    HIPCHK(c, hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_pf[0], hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_pf[1], hipEventDisableTiming));
#endif
    HIPCHK(c, hipHostMalloc((void**)&c->h_nunf, 2 * 1024 * sizeof(int), hipHostMallocDefault));   // [step]{running rows, hand-off failure word}
    if (d.dtype != CW_DTYPE_F32 && d.dtype != CW_DTYPE_BF16 && d.dtype != CW_DTYPE_F16) return fail(c, CW_ERR_INVALID, "unknown dtype %d", d.dtype);
    c->f16 = d.dtype == CW_DTYPE_F16;
    c->bf16 = d.dtype == CW_DTYPE_BF16 || c->f16;
    c->sw = cw_sw::read_switches();   // the environment as it is now: a context's switches are its own from here on
#ifndef CW_EXPERIMENTS
    for (int i = 0; i < cw_sw::kNumRows; ++i)
        if (cw_sw::kRows[i].rejected && cw_sw::kRows[i].get(c->sw) != 0)
            return fail(c, CW_ERR_INVALID, "%s selects a measured-and-rejected kernel variant that is not in this build: make EXTRA=-DCW_EXPERIMENTS", cw_sw::kRows[i].env);
#endif
    c->esz = c->bf16 ? 2 : 4;
    c->Bm = Bm;
    c->S_pad = 1536;
    const size_t e = c->esz;
    const int TGT = d.max_target_positions;

    // ---- weights
    CWCHK(c, dmalloc(c, &c->conv1_w, (size_t)D * 3 * d.n_mels * e));
    CWCHK(c, dmalloc(c, &c->conv2_w, (size_t)D * 3 * D * e));
    CWCHK(c, dmalloc(c, &c->conv1_b, (size_t)D * 4));
    CWCHK(c, dmalloc(c, &c->conv2_b, (size_t)D * 4));
    CWCHK(c, dmalloc(c, &c->enc_pos, (size_t)CW_N_CTX * D * 4));
    CWCHK(c, dmalloc(c, &c->dec_pos, (size_t)TGT * D * 4));
    CWCHK(c, dmalloc(c, &c->embed, (size_t)V * D * e));
    CWCHK(c, dmalloc(c, &c->enc_ln_g, D * 4)); CWCHK(c, dmalloc(c, &c->enc_ln_b, D * 4));
    CWCHK(c, dmalloc(c, &c->dec_ln_g, D * 4)); CWCHK(c, dmalloc(c, &c->dec_ln_b, D * 4));
    c->enc.resize(d.enc_layers);
    c->dec.resize(d.dec_layers);
    auto alloc_common = [&](LayerW& L, bool stacked) -> int {
        CWCHK(c, dmalloc(c, &L.wqkv, (size_t)3 * D * D * e)); CWCHK(c, dmalloc(c, &L.bqkv, (size_t)3 * D * 4));
        if (!stacked) CWCHK(c, dmalloc(c, &L.wo, (size_t)D * D * e));
        CWCHK(c, dmalloc(c, &L.bo, D * 4));
        CWCHK(c, dmalloc(c, &L.ln1_g, D * 4)); CWCHK(c, dmalloc(c, &L.ln1_b, D * 4));
        if (!stacked) CWCHK(c, dmalloc(c, &L.w1, (size_t)F * D * e));
        CWCHK(c, dmalloc(c, &L.b1, F * 4));
        CWCHK(c, dmalloc(c, &L.w2, (size_t)D * F * e)); CWCHK(c, dmalloc(c, &L.b2, D * 4));
        CWCHK(c, dmalloc(c, &L.ln2_g, D * 4)); CWCHK(c, dmalloc(c, &L.ln2_b, D * 4));
        return CW_OK;
    };
    for (auto& L : c->enc) CWCHK(c, alloc_common(L, false));
    for (auto& L : c->dec) {
        const bool stacked = c->bf16;   // 16-bit engines: the four projections live inside the two row-stacked matrices
        CWCHK(c, alloc_common(L, stacked));
        if (stacked) {
            CWCHK(c, dmalloc(c, &L.ws3, (size_t)3 * D * D * e));
            CWCHK(c, dmalloc(c, &L.ws5, ((size_t)2 * F + D) * D * e));
            L.wq_c = L.ws3; L.wo = (char*)L.ws3 + (size_t)2 * D * D * e;
            L.w1 = L.ws5;   L.wo_c = (char*)L.ws5 + (size_t)2 * F * D * e;
            CWCHK(c, dmalloc(c, &L.qa_bias, D * 4)); CWCHK(c, dmalloc(c, &L.q_wsum, D * 4));
            CWCHK(c, dmalloc(c, &L.u1_bias, F * 4)); CWCHK(c, dmalloc(c, &L.u1_wsum, F * 4));
            CWCHK(c, dmalloc(c, &L.qkv_wsum, (size_t)3 * D * 4));
        } else {
            CWCHK(c, dmalloc(c, &L.wq_c, (size_t)D * D * e));
            CWCHK(c, dmalloc(c, &L.wo_c, (size_t)D * D * e));
        }
        CWCHK(c, dmalloc(c, &L.bq_c, D * 4));
        CWCHK(c, dmalloc(c, &L.wkv_c, (size_t)2 * D * D * e)); CWCHK(c, dmalloc(c, &L.bkv_c, (size_t)2 * D * 4));
        CWCHK(c, dmalloc(c, &L.bo_c, D * 4));
        CWCHK(c, dmalloc(c, &L.lnc_g, D * 4)); CWCHK(c, dmalloc(c, &L.lnc_b, D * 4));
        CWCHK(c, dmalloc(c, &L.ck, (size_t)Bm * H * CW_N_CTX * 64 * e));
        CWCHK(c, dmalloc(c, &L.cv, (size_t)Bm * H * CW_N_CTX * 64 * e));
        CWCHK(c, dmalloc(c, &L.sk, (size_t)Bm * H * TGT * 64 * e));
        CWCHK(c, dmalloc(c, &L.sv, (size_t)Bm * H * TGT * 64 * e));
    }

    // ---- mel tables (host-computed: identical on every box)
    {
        std::vector<double> ct(400), sn(400), win(400);
        for (int i = 0; i < 400; ++i) {
            ct[i] = cos(2.0 * M_PI * i / 400.0);
            sn[i] = sin(2.0 * M_PI * i / 400.0);
            win[i] = (double)(float)(0.5 - 0.5 * cos(2.0 * M_PI * i / 400.0));  // torch.hann_window is f32
        }
        double *dct, *dsn, *dwin;
        CWCHK(c, dmalloc(c, &dct, 400 * 8)); CWCHK(c, dmalloc(c, &dsn, 400 * 8)); CWCHK(c, dmalloc(c, &dwin, 400 * 8));
        HIPCHK(c, hipMemcpy(dct, ct.data(), 400 * 8, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dsn, sn.data(), 400 * 8, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dwin, win.data(), 400 * 8, hipMemcpyHostToDevice));
        // slaney mel filterbank, TF/audio_utils.py:448-560, 700-720 (float64 maths, cast to f32 at use)
        const int nm = d.n_mels, nb = 201;
        auto hz2mel = [](double f) { return f >= 1000.0 ? 15.0 + log(f / 1000.0) * (27.0 / log(6.4)) : 3.0 * f / 200.0; };
        auto mel2hz = [](double m) { return m >= 15.0 ? 1000.0 * exp((log(6.4) / 27.0) * (m - 15.0)) : 200.0 * m / 3.0; };
        std::vector<double> ff(nm + 2);
        const double m_lo = hz2mel(0.0), m_hi = hz2mel(8000.0);
        for (int i = 0; i < nm + 2; ++i) {
            double step = (m_hi - m_lo) / (nm + 1);          // np.linspace
            double mv = (i == nm + 1) ? m_hi : m_lo + step * i;
            ff[i] = mel2hz(mv);
        }
        std::vector<float> fb((size_t)nb * nm);
        for (int k = 0; k < nb; ++k) {
            double fk = (k == nb - 1) ? 8000.0 : (8000.0 / (nb - 1)) * k;
            for (int m = 0; m < nm; ++m) {
                double down = -(ff[m] - fk) / (ff[m + 1] - ff[m]);
                double up = (ff[m + 2] - fk) / (ff[m + 2] - ff[m + 1]);
                double v = fmax(0.0, fmin(down, up));
                v *= 2.0 / (ff[m + 2] - ff[m]);
                fb[(size_t)k * nm + m] = (float)v;
            }
        }
        float* dfb;
        CWCHK(c, dmalloc(c, &dfb, fb.size() * 4));
        HIPCHK(c, hipMemcpy(dfb, fb.data(), fb.size() * 4, hipMemcpyHostToDevice));
        c->mel.cos_t = dct; c->mel.sin_t = dsn; c->mel.window = dwin; c->mel.filters = dfb;
        // non-zero bin range of every mel filter (mel.hip: mel_mfma_kernel walks only those)
        {
            std::vector<int> lo(nm, nb), hi(nm, -1);
            for (int m = 0; m < nm; ++m)
                for (int k = 0; k < nb; ++k)
                    if (fb[(size_t)k * nm + m] != 0.f) { if (k < lo[m]) lo[m] = k; if (k > hi[m]) hi[m] = k; }
            int *dlo, *dhi;
            CWCHK(c, dmalloc(c, &dlo, nm * 4)); CWCHK(c, dmalloc(c, &dhi, nm * 4));
            HIPCHK(c, hipMemcpy(dlo, lo.data(), nm * 4, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(dhi, hi.data(), nm * 4, hipMemcpyHostToDevice));
            c->mel.fb_lo = dlo; c->mel.fb_hi = dhi;
        }
    }
    CWCHK(c, dmalloc(c, &c->d_pcm, (size_t)Bm * CW_N_SAMPLES * 4));
    CWCHK(c, dmalloc(c, &c->d_logspec, (size_t)Bm * CW_N_FRAMES * d.n_mels * 4));
    CWCHK(c, dmalloc(c, &c->d_gmax, Bm * 4));
    CWCHK(c, dmalloc(c, &c->d_feats_tm, (size_t)Bm * CW_N_FRAMES * d.n_mels * e));
    c->n_frames_items.assign(Bm, CW_N_FRAMES);

    // ---- encoder workspace
    const size_t MR = (size_t)Bm * CW_N_CTX;
    CWCHK(c, dmalloc(c, &c->c1, (size_t)Bm * CW_N_FRAMES * D * e));
    CWCHK(c, dmalloc(c, &c->x, MR * D * 4));
    CWCHK(c, dmalloc(c, &c->h, MR * D * e));
    CWCHK(c, dmalloc(c, &c->ao, MR * D * e));
    CWCHK(c, dmalloc(c, &c->enc_out, MR * D * e));
    CWCHK(c, dmalloc(c, &c->mid, MR * F * e));
    CWCHK(c, dmalloc(c, &c->qb, (size_t)Bm * H * c->S_pad * 64 * e));
    CWCHK(c, dmalloc(c, &c->kb, (size_t)Bm * H * c->S_pad * 64 * e));
    CWCHK(c, dmalloc(c, &c->vb, (size_t)Bm * H * c->S_pad * 64 * e));
    CWCHK(c, dmalloc(c, &c->d_row_off, Bm * 4)); CWCHK(c, dmalloc(c, &c->d_row_valid, Bm * 4));
    CWCHK(c, dmalloc(c, &c->d_row_off2, Bm * 4)); CWCHK(c, dmalloc(c, &c->d_row_valid2, Bm * 4));
    {
        std::vector<int> off2(Bm), val2(Bm, CW_N_FRAMES);
        for (int i = 0; i < Bm; ++i) off2[i] = i * CW_N_FRAMES;
        HIPCHK(c, hipMemcpy(c->d_row_off2, off2.data(), Bm * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_row_valid2, val2.data(), Bm * 4, hipMemcpyHostToDevice));
    }

    // ---- decoder state
    CWCHK(c, dmalloc(c, &c->dx, (size_t)Bm * D * 4)); CWCHK(c, dmalloc(c, &c->dxn, (size_t)Bm * D * 4));
    CWCHK(c, dmalloc(c, &c->dq, (size_t)Bm * D * 4)); CWCHK(c, dmalloc(c, &c->dattn, (size_t)Bm * D * 4));
    CWCHK(c, dmalloc(c, &c->dmid, (size_t)Bm * F * 4));
    CWCHK(c, dmalloc(c, &c->dx1, (size_t)Bm * D * 4)); CWCHK(c, dmalloc(c, &c->dx2c, (size_t)Bm * D * 4));
    CWCHK(c, dmalloc(c, &c->d_qa, (size_t)2 * Bm * D * 4)); c->d_qb = c->d_qa + (size_t)Bm * D;   // one allocation: the cross-attention kernel takes qb as a 32-bit offset from qa
    CWCHK(c, dmalloc(c, &c->d_u1, (size_t)Bm * F * 4)); CWCHK(c, dmalloc(c, &c->d_pstats, (size_t)128 * 64 * 2 * 4));   // [group of 16 rows 4][tile <= 128][16][2]
    CWCHK(c, dmalloc(c, &c->d_rstats, (size_t)((D > F ? D : F) / 16 + 1) * 64 * 2 * 4));
    CWCHK(c, dmalloc(c, &c->d_bar, 64 * 4));
    {   // declayer.hip: granules are valid by tag only (never cleared); epoch 0 is never used
        CWCHK(c, dmalloc(c, &c->d_gq, (size_t)2 * 16 * D * 8)); CWCHK(c, dmalloc(c, &c->d_gps, (size_t)(D / 16) * 16 * 2 * 8));
        CWCHK(c, dmalloc(c, &c->d_gq2, (size_t)16 * D * 8)); CWCHK(c, dmalloc(c, &c->d_gkv, (size_t)2 * 16 * (D / 2) * 8));
        CWCHK(c, dmalloc(c, &c->d_gflag, (size_t)512 * 8));
        CWCHK(c, dmalloc(c, &c->d_attn16, (size_t)8 * D * 2));
        CWCHK(c, dmalloc(c, &c->d_epoch, 4));
        const unsigned int one = 1;
        HIPCHK(c, hipMemcpy(c->d_epoch, &one, 4, hipMemcpyHostToDevice));
        hipDeviceProp_t prop;
        HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
        c->n_cu = prop.multiProcessorCount;
    }
    CWCHK(c, dmalloc(c, &c->d_xfrag, (size_t)64 * 5120 * 2));
#ifdef CW_EXPERIMENTS   // skinny.hip planes (rejected A/B, CW_SKINNY): four K slices of the widest LayerNorm projection for 64 rows (5.2 MB at large-v3)
    if (Bm > 16) {
        c->planes_cap = (size_t)4 * 64 * (3 * D > F ? 3 * D : F);
        CWCHK(c, dmalloc(c, &c->d_planes, c->planes_cap * 4, false));
        CWCHK(c, dmalloc(c, &c->d_sk_stats, (size_t)16 * 64 * 2 * 4));
    }
#endif
    CWCHK(c, dmalloc(c, &c->d_xfrag2, (size_t)64 * 5120 * 2));
    CWCHK(c, dmalloc(c, &c->d_cvec, 64 * 4)); CWCHK(c, dmalloc(c, &c->d_ostats, (size_t)96 * 64 * 2 * 4));   // column-owning out-projection of 33..64 rows
    c->Vpad = (V + 3) & ~3;
    CWCHK(c, dmalloc(c, &c->dlogits, (size_t)Bm * c->Vpad * 4));
    CWCHK(c, dmalloc(c, &c->d_ids, (size_t)Bm * TGT * 4)); CWCHK(c, dmalloc(c, &c->d_forced, (size_t)Bm * TGT * 4));
    CWCHK(c, dmalloc(c, &c->d_argmax, (size_t)Bm * TGT * 4));
    CWCHK(c, dmalloc(c, &c->d_last_ts, Bm * 4)); CWCHK(c, dmalloc(c, &c->d_finished, Bm * 4));
    CWCHK(c, dmalloc(c, &c->d_nunf, 8));   // {rows still running, hand-off failure word}: one 8-byte copy per step brings both to the host
    c->d_err = c->d_nunf + 1;
#ifdef CW_EXPERIMENTS
    CWCHK(c, dmalloc(c, &c->d_pf_sink, 4));
#endif
    CWCHK(c, dmalloc(c, &c->d_pos, 64 * 4)); CWCHK(c, dmalloc(c, &c->d_cfg, 4 * 4));
    CWCHK(c, dmalloc(c, &c->d_mask, (size_t)V + 16));
    CWCHK(c, dmalloc(c, &c->d_sample_part, (size_t)Bm * 16 * 32));
    CWCHK(c, dmalloc(c, &c->d_sample_pert, (size_t)Bm * 16 * 16));
    CWCHK(c, dmalloc(c, &c->d_samp, (size_t)(4 + 2 * Bm) * 4));
    c->samp_host.assign((size_t)4 + 2 * Bm, 0u);
    CWCHK(c, dmalloc(c, &c->d_lp_sum, (size_t)Bm * 4)); CWCHK(c, dmalloc(c, &c->d_lp_cnt, (size_t)Bm * 4));
    CWCHK(c, dmalloc(c, &c->d_align_slot, (size_t)d.dec_layers * H * 4));
    {
        std::vector<int> slot((size_t)d.dec_layers * H, -1);
        for (int a = 0; a < d.n_align; ++a) {
            int l = c->align_layers[a], hh = c->align_heads[a];
            if (l < 0 || l >= d.dec_layers || hh < 0 || hh >= H) return fail(c, CW_ERR_INVALID, "bad alignment head (%d,%d)", l, hh);
            slot[(size_t)l * H + hh] = a;
        }
        HIPCHK(c, hipMemcpy(c->d_align_slot, slot.data(), slot.size() * 4, hipMemcpyHostToDevice));
    }
    const int Ha = d.n_align > 0 ? d.n_align : 1;
    c->align_rows = TGT;
    CWCHK(c, dmalloc(c, &c->d_align, (size_t)Bm * Ha * TGT * CW_N_CTX * 4));
    CWCHK(c, dmalloc(c, &c->d_part_o, (size_t)ATT_NS * Bm * D * 4));
    CWCHK(c, dmalloc(c, &c->d_part_ml, (size_t)Bm * H * ATT_NS * 2 * 4));
    CWCHK(c, dmalloc(c, &c->d_align_ml, (size_t)Bm * Ha * TGT * ATT_NS * 2 * 4));

    // ---- timestamps workspace
    CWCHK(c, dmalloc(c, &c->d_mean, (size_t)Bm * Ha * CW_N_CTX * 4));
    CWCHK(c, dmalloc(c, &c->d_std, (size_t)Bm * Ha * CW_N_CTX * 4));
    CWCHK(c, dmalloc(c, &c->d_mat, (size_t)Bm * TGT * CW_N_CTX * 4));
    CWCHK(c, dmalloc(c, &c->d_trace, (size_t)Bm * TGT * CW_N_CTX));
    CWCHK(c, dmalloc(c, &c->d_first_col, (size_t)Bm * TGT * 4));
    CWCHK(c, dmalloc(c, &c->d_path_text, (size_t)Bm * (TGT + CW_N_CTX + 2) * 4));
    CWCHK(c, dmalloc(c, &c->d_path_time, (size_t)Bm * (TGT + CW_N_CTX + 2) * 4));
    CWCHK(c, dmalloc(c, &c->d_path_len, Bm * 4));
    CWCHK(c, dmalloc(c, &c->d_ncols, Bm * 4));
    HIPCHK(c, hipDeviceSynchronize());
    return CW_OK;
}

cw_ctx* cw_create(const cw_model_desc* desc, int32_t device) {
    if (!desc) { fail(nullptr, CW_ERR_INVALID, "null desc"); return nullptr; }
    cw_ctx* c = new cw_ctx();
    c->d = *desc;
    c->device = device;
    c->align_layers.assign(desc->align_layers, desc->align_layers + desc->n_align);
    c->align_heads.assign(desc->align_heads, desc->align_heads + desc->n_align);
    c->d.align_layers = c->align_layers.data();
    c->d.align_heads = c->align_heads.data();
    int r = create_impl(c);
    if (r != CW_OK) {
        snprintf(g_err, sizeof(g_err), "%s", c->err);
        cw_destroy(c);
        return nullptr;
    }
    return c;
}

void cw_destroy(cw_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->st) hipStreamSynchronize(c->st);
    for (auto& ge : c->step_graph) if (ge) hipGraphExecDestroy(ge);
    for (auto& f : c->folds) hipFree(f.stage);
    for (auto& o : c->out_stages) hipFree(o.stage);
    for (void* p : c->allocs) hipFree(p);
    for (void* p : {(void*)c->pf_x, c->pf_a, c->pf_q, c->pf_o, c->pf_h}) if (p) hipFree(p);
    for (void* p : {(void*)c->sc_src, (void*)c->sc_tgt, (void*)c->sc_ti, c->sc_a, (void*)c->sc_part, (void*)c->sc_lp, (void*)c->sc_tl,
                    (void*)c->sc_stop, (void*)c->sc_spart, (void*)c->sc_tpart, (void*)c->sc_alt_id, (void*)c->sc_alt_lp,
                    (void*)c->sc_epart, (void*)c->sc_ent}) if (p) hipFree(p);
    if (c->h_nunf) hipHostFree(c->h_nunf);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    for (auto& e : c->ev_step) if (e) hipEventDestroy(e);
    for (auto& e : c->ev_pf) if (e) hipEventDestroy(e);
    if (c->st2) hipStreamDestroy(c->st2);
    if (c->st) hipStreamDestroy(c->st);
    delete c;
}

// ------------------------------------------------------------------------------------------------
// weights
// ------------------------------------------------------------------------------------------------
static int load_tensor_impl(cw_ctx* c, const char* name, const float* data, const int64_t* shape, int32_t ndim);
static int apply_folds(cw_ctx* c);
static int pack_decoder_weights(cw_ctx* c);

int32_t cw_load_tensor(cw_ctx* c, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!name || !data || !shape) return fail(c, CW_ERR_INVALID, "cw_load_tensor: null argument");
    const int r = load_tensor_impl(c, name, data, shape, ndim);
    if (r == CW_OK) { c->loaded.insert(name); c->weights_ok = false; c->enc8_stale = true; }   // e4m3 copies follow the weights
    return r;
}

// Every tensor of WhisperForConditionalGeneration.state_dict() for this geometry (k_proj has no bias,
// modeling_whisper.py:279; proj_out is tied).  Device buffers start zero-filled, so a checkpoint with a missing shard
// would otherwise run and return garbage: the first cw_encode refuses to start until the list is complete.
int32_t cw_check_weights(cw_ctx* c) {
    if (c->weights_ok) return CW_OK;
    std::vector<std::string> want = {
        "model.encoder.conv1.weight", "model.encoder.conv1.bias", "model.encoder.conv2.weight", "model.encoder.conv2.bias",
        "model.encoder.embed_positions.weight", "model.encoder.layer_norm.weight", "model.encoder.layer_norm.bias",
        "model.decoder.embed_tokens.weight", "model.decoder.embed_positions.weight", "model.decoder.layer_norm.weight",
        "model.decoder.layer_norm.bias"};
    auto attn = [&](const std::string& p) {
        for (const char* t : {".q_proj.weight", ".q_proj.bias", ".k_proj.weight", ".v_proj.weight", ".v_proj.bias",
                              ".out_proj.weight", ".out_proj.bias"}) want.push_back(p + t);
    };
    auto pair = [&](const std::string& p) { want.push_back(p + ".weight"); want.push_back(p + ".bias"); };
    for (int stack = 0; stack < 2; ++stack) {
        const int nl = stack ? c->d.dec_layers : c->d.enc_layers;
        for (int l = 0; l < nl; ++l) {
            const std::string p = std::string(stack ? "model.decoder.layers." : "model.encoder.layers.") + std::to_string(l);
            attn(p + ".self_attn"); pair(p + ".self_attn_layer_norm");
            if (stack) { attn(p + ".encoder_attn"); pair(p + ".encoder_attn_layer_norm"); }
            pair(p + ".fc1"); pair(p + ".fc2"); pair(p + ".final_layer_norm");
        }
    }
    std::string missing; int n_missing = 0;
    for (const auto& w : want)
        if (!c->loaded.count(w)) { if (n_missing < 4) missing += (n_missing ? ", " : "") + w; ++n_missing; }
    if (n_missing) return fail(c, CW_ERR_STATE, "%d of %zu weight tensors were never loaded (e.g. %s): incomplete checkpoint", n_missing, want.size(), missing.c_str());
    CWCHK(c, apply_folds(c));
    CWCHK(c, pack_decoder_weights(c));
    c->weights_ok = true;
    return CW_OK;
}

// which: 0 = self-attention LN (q/k/v), 1 = cross-attention LN (q), 2 = final LN (fc1)
static int stage_fold(cw_ctx* c, int layer, int which, const float* data, int N, int K, void* w_dst, size_t w_off, float* b_dst,
                      size_t b_off, float scale) {
    cw_ctx::Fold f{nullptr, N, K, w_dst, w_off, b_dst, b_off, scale, layer, which};
    HIPCHK(c, hipMalloc((void**)&f.stage, (size_t)N * K * 4));
    HIPCHK(c, hipMemcpy(f.stage, data, (size_t)N * K * 4, hipMemcpyHostToDevice));
    c->folds.push_back(f);
    return CW_OK;
}

static int apply_folds(cw_ctx* c) {
    for (auto& f : c->folds) {
        LayerW& L = c->dec[f.layer];
        const float* g = f.which == 0 ? L.ln1_g : (f.which == 1 ? L.lnc_g : L.ln2_g);
        const float* b = f.which == 0 ? L.ln1_b : (f.which == 1 ? L.lnc_b : L.ln2_b);
        CWCHK(c, KD(c, cw_launch_fold_layernorm, f.stage, f.N, f.K, g, b, f.scale, (bf16_t*)f.w_dst + f.w_off, f.b_dst + f.b_off, c->st));
    }
    // six-launch layer: product matrices W'q_c Wo and W'1 Wo_c (f32 from the checkpoint values, one 16-bit rounding), the
    // constants W'q_c bo / W'1 bo_c and the row sums of the folded 16-bit weights (what the MFMAs actually multiply by)
    const int D = c->d.d_model, F = c->d.ffn_dim;
    bool all = !c->folds.empty() && !c->sw.no_fuse6 && F % D == 0 && D <= 1280 && D % 64 == 0 && F % 64 == 0 && c->d.n_heads <= 20;
    if (all) {
        for (int l = 0; l < c->d.dec_layers && all; ++l) {
            const cw_ctx::Fold *fq = nullptr, *f1 = nullptr;
            const float *so = nullptr, *sc = nullptr;
            for (auto& f : c->folds) if (f.layer == l) { if (f.which == 1) fq = &f; else if (f.which == 2) f1 = &f; }
            for (auto& o : c->out_stages) if (o.layer == l) { if (o.which == 0) so = o.stage; else sc = o.stage; }
            if (!fq || !f1 || !so || !sc) { all = false; break; }
            LayerW& L = c->dec[l];
            const size_t e = c->esz;
            CWCHK(c, KD(c, cw_launch_fold_product, fq->stage, L.lnc_g, fq->scale, so, D, D, D, (char*)L.ws3 + (size_t)D * D * e, c->st));
            CWCHK(c, KD(c, cw_launch_fold_rowvec, fq->stage, L.lnc_g, fq->scale, L.bo, L.wq_c, D, D, L.qa_bias, L.q_wsum, c->st));
            CWCHK(c, KD(c, cw_launch_fold_product, f1->stage, L.ln2_g, f1->scale, sc, F, D, D, (char*)L.ws5 + (size_t)F * D * e, c->st));
            CWCHK(c, KD(c, cw_launch_fold_rowvec, f1->stage, L.ln2_g, f1->scale, L.bo_c, L.w1, F, D, L.u1_bias, L.u1_wsum, c->st));
        }
    }
    // 17..64-row path: row sums of the folded 16-bit matrices (row-major here: packing comes after the folds)
    bool rows_ok = !c->folds.empty() && c->bf16 && D % 128 == 0 && F % 128 == 0 && F <= 5120;
    for (int l = 0; l < c->d.dec_layers && rows_ok; ++l) {
        LayerW& L = c->dec[l];
        if (!L.qkv_wsum || !L.q_wsum || !L.u1_wsum) { rows_ok = false; break; }
        CWCHK(c, KD(c, cw_launch_fold_rowvec, nullptr, nullptr, 1.0f, nullptr, L.wqkv, 3 * D, D, nullptr, L.qkv_wsum, c->st));
        if (!all) {
            CWCHK(c, KD(c, cw_launch_fold_rowvec, nullptr, nullptr, 1.0f, nullptr, L.wq_c, D, D, nullptr, L.q_wsum, c->st));
            CWCHK(c, KD(c, cw_launch_fold_rowvec, nullptr, nullptr, 1.0f, nullptr, L.w1, F, D, nullptr, L.u1_wsum, c->st));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    KCHK(c);
    c->fuse6_ready = all;
    c->rows_ln_ready = rows_ok;
    for (auto& f : c->folds) hipFree(f.stage);
    for (auto& o : c->out_stages) hipFree(o.stage);
    c->out_stages.clear();
    if (!c->folds.empty()) c->ln_folded = true;
    c->folds.clear();
    return CW_OK;
}

// 16-bit engines: the decoder's GEMV weight matrices go fragment-major once every tensor is in and folded (gemm.hip:
// wfrag_pack_kernel) -- in place through one scratch buffer -- and the tied embedding gets a packed copy for the logits GEMV.
// A tensor loaded afterwards would land row-major in a packed matrix: refused like a load after folding.
static int pack_decoder_weights(cw_ctx* c) {
    if (!c->bf16 || c->sw.no_wpack || c->wpacked) return CW_OK;
    const int D = c->d.d_model, F = c->d.ffn_dim, V = c->d.vocab_size;
    // packed weights are read by gemv2_bf16_kernel / gemv_mt_kernel / gemv_stack_kernel only (the first-generation GEMV reads
    // row-major): pack exactly when those kernels take every decoder shape -- K = d_model in one K slice (<= 1280), fc2's
    // K = ffn_dim in power-of-two slices of <= 1280 that are multiples of 128 (gemm.hip: gemv2_ok).  Wider geometries
    // (d_model up to 2048 is accepted by cw_create) keep row-major weights and the fallback kernel.
    int fks = 1;
    while (F / fks > 1280) fks *= 2;
    if (D % 128 || D > 1280 || F % 128 || F > 5120 || F % fks || (F / fks) % 128) return CW_OK;
    const size_t emb_elems = KD(c, cw_wfrag_elems, V, D);
    size_t tmp_elems = (size_t)(2 * F + D) * D;
    if ((size_t)3 * D * D > tmp_elems) tmp_elems = (size_t)3 * D * D;
    void* tmp = nullptr;
    HIPCHK(c, hipMalloc(&tmp, tmp_elems * 2));
    auto pack = [&](void* w, int N, int K) -> int {
        CWCHK(c, KD(c, cw_launch_wfrag_pack, w, N, K, tmp, c->st));
        HIPCHK(c, hipMemcpyAsync(w, tmp, (size_t)N * K * 2, hipMemcpyDeviceToDevice, c->st));
        return CW_OK;
    };
    int r = CW_OK;
    for (auto& L : c->dec) {
        if (r == CW_OK) r = pack(L.wqkv, 3 * D, D);
        if (r == CW_OK) r = pack(L.ws3, 3 * D, D);            // [W'q_c ; W'q_c Wo ; Wo]: wq_c / wo point into it
        if (r == CW_OK) r = pack(L.ws5, 2 * F + D, D);        // [W'1 ; W'1 Wo_c ; Wo_c]: w1 / wo_c point into it
        if (r == CW_OK) r = pack(L.w2, D, F);
    }
    if (r == CW_OK && !c->embed_pk) r = dmalloc(c, &c->embed_pk, emb_elems * 2, false);
    if (r == CW_OK) r = KD(c, cw_launch_wfrag_pack, c->embed, V, D, c->embed_pk, c->st);
    hipStreamSynchronize(c->st);
    hipFree(tmp);
    if (r != CW_OK) return r;
    KCHK(c);
    c->wpacked = true;
    return CW_OK;
}

static int load_tensor_impl(cw_ctx* c, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    const int D = c->d.d_model, F = c->d.ffn_dim, V = c->d.vocab_size, NM = c->d.n_mels;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    auto expect = [&](size_t want) -> int {
        if (n != want) return fail(c, CW_ERR_INVALID, "tensor %s: %zu elements, expected %zu", name, n, want);
        return CW_OK;
    };
    std::string s(name);
    if (s == "proj_out.weight") return CW_OK;  // tied to embed_tokens (modeling_whisper.py:965)
    if (s == "model.encoder.conv1.weight" || s == "model.encoder.conv2.weight") {
        const bool first = s == "model.encoder.conv1.weight";
        const int C = first ? NM : D;
        if (C % 64) return fail(c, CW_ERR_INVALID, "tensor %s: the encoder needs n_mels to be a multiple of 64 (n_mels=%d runs the mel stage only)", name, NM);
        CWCHK(c, expect((size_t)D * C * 3));
        std::vector<float> re((size_t)D * 3 * C);  // [O][C][3] -> [O][3][C]
        for (int o = 0; o < D; ++o)
            for (int ci = 0; ci < C; ++ci)
                for (int k = 0; k < 3; ++k) re[((size_t)o * 3 + k) * C + ci] = data[((size_t)o * C + ci) * 3 + k];
        return upload_T(c, first ? c->conv1_w : c->conv2_w, 0, re.data(), re.size());
    }
    if (s == "model.encoder.conv1.bias") { CWCHK(c, expect(D)); return upload_f32(c, c->conv1_b, 0, data, n); }
    if (s == "model.encoder.conv2.bias") { CWCHK(c, expect(D)); return upload_f32(c, c->conv2_b, 0, data, n); }
    if (s == "model.encoder.embed_positions.weight") { CWCHK(c, expect((size_t)CW_N_CTX * D)); return upload_f32(c, c->enc_pos, 0, data, n); }
    if (s == "model.decoder.embed_positions.weight") { CWCHK(c, expect((size_t)c->d.max_target_positions * D)); return upload_f32(c, c->dec_pos, 0, data, n); }
    if (s == "model.decoder.embed_tokens.weight") {
        CWCHK(c, expect((size_t)V * D));
        if (c->wpacked) return fail(c, CW_ERR_STATE, "decoder weights were already packed for the decode GEMVs: create a new context to load another checkpoint");
        return upload_T(c, c->embed, 0, data, n);
    }
    if (s == "model.encoder.layer_norm.weight") { CWCHK(c, expect(D)); return upload_f32(c, c->enc_ln_g, 0, data, n); }
    if (s == "model.encoder.layer_norm.bias") { CWCHK(c, expect(D)); return upload_f32(c, c->enc_ln_b, 0, data, n); }
    if (s == "model.decoder.layer_norm.weight") { CWCHK(c, expect(D)); return upload_f32(c, c->dec_ln_g, 0, data, n); }
    if (s == "model.decoder.layer_norm.bias") { CWCHK(c, expect(D)); return upload_f32(c, c->dec_ln_b, 0, data, n); }

    int li = -1; char rest[128] = "";
    bool is_dec = false;
    if (sscanf(name, "model.encoder.layers.%d.%127s", &li, rest) == 2) is_dec = false;
    else if (sscanf(name, "model.decoder.layers.%d.%127s", &li, rest) == 2) is_dec = true;
    else return fail(c, CW_ERR_INVALID, "unknown tensor name %s", name);
    if (li < 0 || li >= (is_dec ? c->d.dec_layers : c->d.enc_layers)) return fail(c, CW_ERR_INVALID, "layer index out of range in %s", name);
    LayerW& L = is_dec ? c->dec[li] : c->enc[li];
    std::string r(rest);
    const float qs = 0.125f;  // head_dim ** -0.5, folded into q projections (exact: power of two)
    const size_t DD = (size_t)D * D;
    if (c->wpacked && is_dec)
        return fail(c, CW_ERR_STATE, "decoder weights were already packed for the decode GEMVs: create a new context to load another checkpoint");
    if (is_dec && c->bf16 && !c->sw.no_ln_fold) {   // LayerNorm-fed decode projections: folded once all tensors are in
        if (c->ln_folded) return fail(c, CW_ERR_STATE, "weights were already folded: create a new context to load another checkpoint");
        if (r == "self_attn.q_proj.weight") { CWCHK(c, expect(DD)); return stage_fold(c, li, 0, data, D, D, L.wqkv, 0, L.bqkv, 0, qs); }
        if (r == "self_attn.k_proj.weight") { CWCHK(c, expect(DD)); return stage_fold(c, li, 0, data, D, D, L.wqkv, DD, L.bqkv, (size_t)D, 1.f); }
        if (r == "self_attn.v_proj.weight") { CWCHK(c, expect(DD)); return stage_fold(c, li, 0, data, D, D, L.wqkv, 2 * DD, L.bqkv, 2 * (size_t)D, 1.f); }
        if (r == "encoder_attn.q_proj.weight") { CWCHK(c, expect(DD)); return stage_fold(c, li, 1, data, D, D, L.wq_c, 0, L.bq_c, 0, qs); }
        if (r == "fc1.weight") { CWCHK(c, expect((size_t)F * D)); return stage_fold(c, li, 2, data, F, D, L.w1, 0, L.b1, 0, 1.f); }
        if (!c->sw.no_fuse6 && (r == "self_attn.out_proj.weight" || r == "encoder_attn.out_proj.weight")) {   // f32 copy for the products
            CWCHK(c, expect(DD));
            cw_ctx::OutStage o{nullptr, li, r[0] == 's' ? 0 : 1};
            HIPCHK(c, hipMalloc((void**)&o.stage, DD * 4));
            HIPCHK(c, hipMemcpy(o.stage, data, DD * 4, hipMemcpyHostToDevice));
            c->out_stages.push_back(o);
        }
    }
    if (r == "self_attn.q_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wqkv, 0, data, n, qs); }
    if (r == "self_attn.k_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wqkv, DD, data, n); }
    if (r == "self_attn.v_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wqkv, 2 * DD, data, n); }
    if (r == "self_attn.q_proj.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.bqkv, 0, data, n, qs); }
    if (r == "self_attn.v_proj.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.bqkv, 2 * (size_t)D, data, n); }
    if (r == "self_attn.out_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wo, 0, data, n); }
    if (r == "self_attn.out_proj.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.bo, 0, data, n); }
    if (r == "self_attn_layer_norm.weight") { CWCHK(c, expect(D)); return upload_f32(c, L.ln1_g, 0, data, n); }
    if (r == "self_attn_layer_norm.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.ln1_b, 0, data, n); }
    if (r == "fc1.weight") { CWCHK(c, expect((size_t)F * D)); return upload_T(c, L.w1, 0, data, n); }
    if (r == "fc1.bias") { CWCHK(c, expect(F)); return upload_f32(c, L.b1, 0, data, n); }
    if (r == "fc2.weight") { CWCHK(c, expect((size_t)F * D)); return upload_T(c, L.w2, 0, data, n); }
    if (r == "fc2.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.b2, 0, data, n); }
    if (r == "final_layer_norm.weight") { CWCHK(c, expect(D)); return upload_f32(c, L.ln2_g, 0, data, n); }
    if (r == "final_layer_norm.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.ln2_b, 0, data, n); }
    if (is_dec) {
        if (r == "encoder_attn.q_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wq_c, 0, data, n, qs); }
        if (r == "encoder_attn.q_proj.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.bq_c, 0, data, n, qs); }
        if (r == "encoder_attn.k_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wkv_c, 0, data, n); }
        if (r == "encoder_attn.v_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wkv_c, DD, data, n); }
        if (r == "encoder_attn.v_proj.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.bkv_c, (size_t)D, data, n); }
        if (r == "encoder_attn.out_proj.weight") { CWCHK(c, expect(DD)); return upload_T(c, L.wo_c, 0, data, n); }
        if (r == "encoder_attn.out_proj.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.bo_c, 0, data, n); }
        if (r == "encoder_attn_layer_norm.weight") { CWCHK(c, expect(D)); return upload_f32(c, L.lnc_g, 0, data, n); }
        if (r == "encoder_attn_layer_norm.bias") { CWCHK(c, expect(D)); return upload_f32(c, L.lnc_b, 0, data, n); }
    }
    return fail(c, CW_ERR_INVALID, "unknown tensor name %s", name);
}

int32_t cw_set_generation(cw_ctx* c, const cw_gen_cfg* g) {
    const int V = c->d.vocab_size;
    std::vector<unsigned char> mask(V, 0);
    for (int i = 0; i < g->n_suppress; ++i) {
        int t = g->suppress_tokens[i];
        if (t < 0 || t >= V) return fail(c, CW_ERR_INVALID, "suppress token %d out of range", t);
        mask[t] |= 1;
    }
    for (int i = 0; i < g->n_begin_suppress; ++i) {
        int t = g->begin_suppress_tokens[i];
        if (t < 0 || t >= V) return fail(c, CW_ERR_INVALID, "begin-suppress token %d out of range", t);
        mask[t] |= 2;
    }
    if (g->no_timestamps_token_id < 0 || g->no_timestamps_token_id + 1 >= V) return fail(c, CW_ERR_INVALID, "no_timestamps_token_id out of range");
    mask[g->no_timestamps_token_id] |= 1;  // logits_process.py:2003
    HIPCHK(c, hipMemcpy(c->d_mask, mask.data(), V, hipMemcpyHostToDevice));
    for (auto& ge : c->step_graph) if (ge) { hipGraphExecDestroy(ge); ge = nullptr; }   // token ids are baked into captured kernel args
    c->gen = *g;
    c->gen.suppress_tokens = nullptr;
    c->gen.begin_suppress_tokens = nullptr;
    c->gen_set = true;
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// front end
// ------------------------------------------------------------------------------------------------
int32_t cw_upload_pcm(cw_ctx* c, const float* pcm, int32_t B, const int32_t* n_samples) {
    if (B < 1 || B > c->Bm) return fail(c, CW_ERR_INVALID, "B=%d out of range (max_batch %d)", B, c->Bm);
    HIPCHK(c, hipMemsetAsync(c->d_pcm, 0, (size_t)B * CW_N_SAMPLES * 4, c->st));
    size_t off = 0;
    for (int b = 0; b < B; ++b) {
        int n = n_samples[b];
        if (n < 0 || n > CW_N_SAMPLES) return fail(c, CW_ERR_INVALID, "n_samples[%d]=%d out of range", b, n);
        HIPCHK(c, hipMemcpyAsync(c->d_pcm + (size_t)b * CW_N_SAMPLES, pcm + off, (size_t)n * 4, hipMemcpyHostToDevice, c->st));
        off += n;
        c->n_frames_items[b] = (n + 159) / 160;  // attention_mask[:, ::hop].sum()  (feature_extraction_whisper.py:332-341)
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return CW_OK;
}

int32_t cw_mel_resident(cw_ctx* c, int32_t B) {
    if (B < 1 || B > c->Bm) return fail(c, CW_ERR_INVALID, "B=%d out of range", B);
    StageTimer tm(c, CW_STAGE_MEL);
    CWCHK(c, KD(c, cw_launch_mel, c->mel, c->d_pcm, B, c->d.n_mels, c->d_logspec, c->d_gmax, c->st));
    CWCHK(c, KD(c, cw_launch_mel_finish, c->d_logspec, c->d_gmax, B, c->d.n_mels, c->d_feats_tm, c->bf16 ? 1 : 0, c->d_feats_hf, c->st));
    KCHK(c);
    tm.stop();
    return CW_OK;
}

int32_t cw_mel(cw_ctx* c, const float* pcm, int32_t B, const int32_t* n_samples, float* feats_out, int32_t* n_frames_out) {
    CWCHK(c, cw_upload_pcm(c, pcm, B, n_samples));
    if (feats_out && !c->d_feats_hf) CWCHK(c, dmalloc(c, &c->d_feats_hf, (size_t)c->Bm * CW_N_FRAMES * c->d.n_mels * 4));
    float* keep = c->d_feats_hf;
    if (!feats_out) c->d_feats_hf = nullptr;
    int r = cw_mel_resident(c, B);
    c->d_feats_hf = keep;
    if (r != CW_OK) return r;
    if (feats_out) HIPCHK(c, hipMemcpy(feats_out, c->d_feats_hf, (size_t)B * CW_N_FRAMES * c->d.n_mels * 4, hipMemcpyDeviceToHost));
    if (n_frames_out) for (int b = 0; b < B; ++b) n_frames_out[b] = c->n_frames_items[b];
    return CW_OK;
}

int32_t cw_set_features(cw_ctx* c, const float* feats, int32_t B) {
    if (B < 1 || B > c->Bm) return fail(c, CW_ERR_INVALID, "B=%d out of range", B);
    const int NM = c->d.n_mels;
    std::vector<float> tmaj((size_t)B * CW_N_FRAMES * NM);
    for (int b = 0; b < B; ++b)
        for (int m = 0; m < NM; ++m)
            for (int t = 0; t < CW_N_FRAMES; ++t)
                tmaj[((size_t)b * CW_N_FRAMES + t) * NM + m] = feats[((size_t)b * NM + m) * CW_N_FRAMES + t];
    return upload_T(c, c->d_feats_tm, 0, tmaj.data(), tmaj.size());
}

// ------------------------------------------------------------------------------------------------
// encoder
// ------------------------------------------------------------------------------------------------
extern "C++" { template <class T> static T zeroed() { T p; memset(&p, 0, sizeof(p)); return p; } }   // launch parameters start from all-zero bytes
EpiParams epi0() { return zeroed<EpiParams>(); }
DecAttnParams dec_attn(const float* q, const void* K, const void* V, int cap, int n_keys, const int* pos, float* out,
                              int B, int H) {
    DecAttnParams p;
    memset(&p, 0, sizeof(p));
    p.q = q; p.K = K; p.V = V; p.cap = cap; p.n_keys = n_keys; p.pos = pos; p.out = out; p.B = B; p.H = H;
    return p;
}

static int enc8_quantise(cw_ctx* c);

int32_t cw_encode(cw_ctx* c, int32_t nb, const int32_t* item, const int32_t* seek, const int32_t* n_frames) {
    const int D = c->d.d_model, H = c->d.n_heads, F = c->d.ffn_dim, NM = c->d.n_mels, S = CW_N_CTX;
    if (nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "nb=%d out of range", nb);
    if (NM % 64) return fail(c, CW_ERR_INVALID, "encode: the encoder needs n_mels to be a multiple of 64 (n_mels=%d runs the mel stage only)", NM);
    std::vector<int> off(nb), val(nb);
    for (int i = 0; i < nb; ++i) {
        if (item[i] < 0 || item[i] >= c->Bm || seek[i] < 0 || n_frames[i] < 0 || seek[i] + n_frames[i] > CW_N_FRAMES)
            return fail(c, CW_ERR_INVALID, "bad window %d: item=%d seek=%d n=%d", i, item[i], seek[i], n_frames[i]);
        off[i] = item[i] * CW_N_FRAMES + seek[i];
        val[i] = n_frames[i];
    }
    CWCHK(c, cw_check_weights(c));
    if (c->enc8 && c->enc8_stale) CWCHK(c, enc8_quantise(c));
    HIPCHK(c, hipMemcpyAsync(c->d_row_off, off.data(), nb * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->d_row_valid, val.data(), nb * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));  // host vectors go out of scope
    const bool bf = c->bf16;
    StageTimer tm(c, CW_STAGE_ENCODER);
    {   // conv1 + GELU (modeling_whisper.py:618) as implicit GEMM over time-major features
        AParams ap{c->d_feats_tm, 0, 1, CW_N_FRAMES, NM, 1, c->d_row_off, c->d_row_valid};
        EpiParams ep = epi0(); ep.out = c->c1; ep.bias = c->conv1_b; ep.ldo = D;
        CWCHK(c, KD(c, cw_launch_gemm, bf, EPI_GELU, ap, c->conv1_w, nb * CW_N_FRAMES, D, 3 * NM, ep, c->st));
    }
    {   // conv2 (stride 2) + GELU + sinusoidal positions (:619-624) -> f32 residual stream
        AParams ap{c->c1, 0, 1, S, D, 2, c->d_row_off2, c->d_row_valid2};
        EpiParams ep = epi0(); ep.outf = c->x; ep.bias = c->conv2_b; ep.ldo = D; ep.pos = c->enc_pos; ep.T = S;
        CWCHK(c, KD(c, cw_launch_gemm, bf, EPI_GELU_POS_F32, ap, c->conv2_w, nb * S, D, 3 * D, ep, c->st));
    }
    const int M = nb * S;
    for (int l = 0; l < c->d.enc_layers; ++l) {
        LayerW& L = c->enc[l];
        if (c->enc8_mask & 1) CWCHK(c, KD(c, cw_launch_layernorm_fp8, c->x, L.ln1_g, L.ln1_b, c->h8, c->sa8, M, D, c->st));
        else CWCHK(c, KD(c, cw_launch_layernorm, bf, c->x, L.ln1_g, L.ln1_b, c->h, M, D, c->st));
        {
            AParams ap{c->h, D, 0, 0, 0, 0, nullptr, nullptr};
            EpiParams ep = epi0(); ep.out = c->qb; ep.out1 = c->kb; ep.out2 = c->vb; ep.bias = L.bqkv;
            ep.T = S; ep.S_pad = c->S_pad; ep.H = H; ep.d_model = D;
            if (c->enc8_mask & 1) CWCHK(c, KD(c, cw_launch_gemm_fp8, EPI_HEADS, c->h8, D, L.wqkv8, M, 3 * D, D, c->sa8, L.sqkv, ep, c->st));
            else CWCHK(c, KD(c, cw_launch_gemm, bf, EPI_HEADS, ap, L.wqkv, M, 3 * D, D, ep, c->st));
        }
        CWCHK(c, KD(c, cw_launch_attn_encoder, bf, c->qb, c->kb, c->vb, c->ao, nb, H, S, c->S_pad, c->st));
        {
            AParams ap{c->ao, D, 0, 0, 0, 0, nullptr, nullptr};
            EpiParams ep = epi0(); ep.outf = c->x; ep.resid = c->x; ep.bias = L.bo; ep.ldo = D;
            CWCHK(c, KD(c, cw_launch_gemm, bf, EPI_RESID_F32, ap, L.wo, M, D, D, ep, c->st));
        }
        if (c->enc8_mask & 2) CWCHK(c, KD(c, cw_launch_layernorm_fp8, c->x, L.ln2_g, L.ln2_b, c->h8, c->sa8, M, D, c->st));
        else CWCHK(c, KD(c, cw_launch_layernorm, bf, c->x, L.ln2_g, L.ln2_b, c->h, M, D, c->st));
        {
            AParams ap{c->h, D, 0, 0, 0, 0, nullptr, nullptr};
            EpiParams ep = epi0(); ep.out = c->mid; ep.bias = L.b1; ep.ldo = F;
            if (c->enc8_mask & 2) CWCHK(c, KD(c, cw_launch_gemm_fp8, EPI_GELU, c->h8, D, L.w18, M, F, D, c->sa8, L.s1, ep, c->st));
            else CWCHK(c, KD(c, cw_launch_gemm, bf, EPI_GELU, ap, L.w1, M, F, D, ep, c->st));
        }
        {
            AParams ap{c->mid, F, 0, 0, 0, 0, nullptr, nullptr};
            EpiParams ep = epi0(); ep.outf = c->x; ep.resid = c->x; ep.bias = L.b2; ep.ldo = D;
            if (c->enc8_mask & 4) {   // GELU output: its row maxima are only known once fc1 is complete -> one row-wise quantisation pass
                CWCHK(c, KD(c, cw_launch_quant_rows_fp8, c->mid, M, F, c->mid8, c->smid8, c->st));
                CWCHK(c, KD(c, cw_launch_gemm_fp8, EPI_RESID_F32, c->mid8, F, L.w28, M, D, F, c->smid8, L.s2, ep, c->st));
            } else CWCHK(c, KD(c, cw_launch_gemm, bf, EPI_RESID_F32, ap, L.w2, M, D, F, ep, c->st));
        }
    }
    CWCHK(c, KD(c, cw_launch_layernorm, bf, c->x, c->enc_ln_g, c->enc_ln_b, c->enc_out, M, D, c->st));   // cw_get_encoder_output
    if (c->enc8_mask & 8) CWCHK(c, KD(c, cw_launch_layernorm_fp8, c->x, c->enc_ln_g, c->enc_ln_b, c->h8, c->sa8, M, D, c->st));
    KCHK(c);
    tm.stop();
    StageTimer tk(c, CW_STAGE_CROSS_KV);
    for (int l = 0; l < c->d.dec_layers; ++l) {   // cross-attention K/V, once per window (:322-335)
        LayerW& L = c->dec[l];
        AParams ap{c->enc_out, D, 0, 0, 0, 0, nullptr, nullptr};
        EpiParams ep = epi0(); ep.out = L.ck; ep.out1 = L.cv; ep.bias = L.bkv_c;
        ep.T = S; ep.S_pad = S; ep.H = H; ep.d_model = D;
        if (c->enc8_mask & 8) CWCHK(c, KD(c, cw_launch_gemm_fp8, EPI_HEADS, c->h8, D, L.wkv_c8, M, 2 * D, D, c->sa8, L.skv_c, ep, c->st));
        else CWCHK(c, KD(c, cw_launch_gemm, bf, EPI_HEADS, ap, L.wkv_c, M, 2 * D, D, ep, c->st));
        if (c->kv8) CWCHK(c, KD(c, cw_launch_kv_quant_fp8, L.ck, L.cv, L.ck8, L.cv8, L.kvs, nb, H, S, c->st));
    }
    KCHK(c);
    tk.stop();
    c->nb_encoded = nb;
    return CW_OK;
}

int32_t cw_get_encoder_output(cw_ctx* c, float* out, int32_t nb) {
    if (nb < 1 || nb > c->nb_encoded) return fail(c, CW_ERR_STATE, "only %d windows encoded", c->nb_encoded);
    HIPCHK(c, hipStreamSynchronize(c->st));
    return download_T(c, c->enc_out, 0, out, (size_t)nb * CW_N_CTX * c->d.d_model);
}

// ------------------------------------------------------------------------------------------------
// decoder
// ------------------------------------------------------------------------------------------------
int gemv_ln(cw_ctx* c, int epi, const float* x, int Mb, int K, const void* W, int N, const float* g,
                   const float* b, const EpiParams& ep) {
    // (17..64 rows over row-major weights -- CW_NO_WPACK=1, or a geometry pack_decoder_weights does not take: no scratch, i.e. groups of
    // 16 rows on the <= 16-row kernels; gemv_mt_kernel reads fragment-major weights only)
    if (c->bf16 || !g) return KD(c, cw_launch_gemv, c->bf16, epi, x, Mb, K, W, N, g, b, ep, c->st, nullptr, (Mb <= 16 || c->wpacked) ? c->d_xfrag : nullptr, c->bf16 && c->wpacked, !c->sw.no_wnt);
    int r = KD(c, cw_launch_layernorm_f32, x, g, b, c->dxn, Mb, K, c->st);   // f32 parity mode: unfused LN
    if (r != CW_OK) return r;
    return KD(c, cw_launch_gemv, false, epi, c->dxn, Mb, K, W, N, nullptr, nullptr, ep, c->st);
}

int launch_logits(cw_ctx* c, int nb, const float* x) {   // final LN + tied proj_out (:790, :1080), logits in f32 (utils.py:2894)
    EpiParams ep = epi0(); ep.outf = c->dlogits; ep.ldo = c->Vpad;
    return gemv_ln(c, EPI_STORE_F32, x, nb, c->d.d_model, (c->bf16 && c->wpacked) ? c->embed_pk : c->embed, c->d.vocab_size, c->dec_ln_g, c->dec_ln_b, ep);
}

// ---- the decode step: plan, layers, logits.  Which launches a decoder layer has is constant over the layers of one forward: plan_step settles it
// once per (context, nb), every predicate in one place; decode_step, run_step (graph slot) and the stage bookkeeping of cw_time_decode_stage read it.
struct StepPlan {
    bool frag, fuse, own, qs, xq, short_hist, mid16; int nt3;
#ifdef CW_EXPERIMENTS
    bool fuse_mlp, mlp_pair, mlp_chain, dl, sk_ok, skinny, xfull, rows, pf; int lo_off;
#else   // the measured-and-rejected variants are not in this build: create_impl and cw_set_option refuse their switches
    static constexpr bool fuse_mlp = false, mlp_pair = false, mlp_chain = false, dl = false, sk_ok = false, skinny = false, xfull = false, rows = false, pf = false;
    static constexpr int lo_off = 0;
#endif
};
static StepPlan plan_step(const cw_ctx* c, int nb) {
    const int D = c->d.d_model, H = c->d.n_heads, F = c->d.ffn_dim, TGT = c->d.max_target_positions;
    StepPlan P{};
    // 17..64 rows (bf16): producers hand activations to the next GEMV already in MFMA fragment order (no prep launch)
    P.frag = c->bf16 && nb > 16 && c->wpacked;      // (row-major weights: groups of 16 rows on the <= 16-row kernels, see gemv_ln)
    // fused out-projection / cross-query stage (decfuse.hip): greedy rows of one MFMA half tile, 16-bit caches.  The residual
    // stream then alternates between two buffers: a layer reads x from `xin` and leaves x1, x2, x3 in `xalt`.
    // (e4m3 cache: the fp8 matrix-core kernel finishes the fused query too; its VALU fallback does not)
    // 17..64 greedy rows (round 5): the same stage in groups of 16 rows (gemv_stack_kernel's grid y) replaces out-projection,
    // LayerNorm preparation and query projection -- three of the layer's twelve launches -- by one; the rest of the layer keeps its
    // preparation + gemv_mt launches, on the alternating buffers.  CW_NO_FUSE_ROWS=1: the twelve launches (A/B).  Batch 64: decode
    // 4.43 -> 4.28 ms per token step, 64 / 64 clips; over the e4m3 cache 3.47 -> 3.41 once the cross-attention kernel lets wave 0 alone
    // finish the query (attn_cross_mfma8_kernel<1, 2>; every wave doing it, as at <= 16 rows, measured flat).  CW_NO_FUSE_ROWS8=1: A/B
    // (the rejected 17..64-row A/B variants of -DCW_EXPERIMENTS builds -- rows path, skinny GEMMs, full-key cross-attention -- keep their
    // own twelve / nine launches: they read c->dx and d_xfrag, which the fused stage's alternating buffers would leave stale)
    const bool ab17 = nb > 16 && (c->sw.rows_ln || c->sw.skinny != 0);
    P.fuse = c->bf16 && c->fuse6_ready && !c->sw.no_fuse6 && c->ln_folded && !ab17 && (nb <= 16 || P.frag) && (nb <= 16 || (!c->sw.no_fuse_rows && nb <= 64 && (!c->kv8 || !c->sw.no_fuse_rows8))) &&
             // beam search (round 6): the hypotheses of an item share a cross-attention block that finishes their queries
             // (attn_cross_mfma_kernel<.., FUSED>, 16-bit cache); CW_NO_FUSE_BEAM=1: the twelve launches
             (c->beam_K == 0 || (!c->sw.no_fuse_beam && !c->kv8 && c->beam_K <= 16 && !c->sw.fuse_mlp)) &&
             (!c->kv8 || (KD(c, cw_cross8_is_mfma, CW_N_CTX) && !c->sw.fuse_mlp)) && !((c->sw.fuse_mlp || c->sw.mlp_pair) && nb > 8);
    // 33..64 rows behind the fused stage (round 6): the cross-attention out-projection owns whole columns (no K split, no atomics) and
    // leaves fc1 its 16-bit rows and LayerNorm partial sums -- one preparation launch less per layer (gemm.hip: gemv_mt_kernel OWN / LNA)
    P.own = !c->sw.no_own_cols && P.fuse && P.frag && nb > 32 && !c->sw.fuse_mlp && !c->sw.mlp_pair && c->rows_ln_ready && D % 32 == 0 && D / 16 <= 96 && D <= 1536 &&
            D % 128 == 0 && F % 32 == 0;
    // column tiles per X1 block (3 * TD blocks at 1: 240 at large-v3).  17..64 rows: two -- a block's 16 f32 rows are twice the bytes
    // of a weight tile, and a pair of tiles shares them (64 rows, 4 groups: 11.2 us at one tile, 10.5 at two, 15.5 at three)
    P.nt3 = c->sw.stack_nt3 > 0 ? c->sw.stack_nt3 : (nb > 16 ? 2 : 1);
    // rows <= 8, 16-bit engines: LN + q/k/v projection + self-attention as ONE launch (declayer.hip: qkv_self_kernel; the tiles
    // reach the attention blocks as granules, the history rows of the cache are requested at kernel entry); bit-identical
    // (its 3 D / 16 blocks wait for each other: only where the whole grid is resident at once on this part; layer < 64: granule tag)
    P.qs = !c->sw.no_qkv_self && c->bf16 && c->ln_folded && c->wpacked && nb <= 8 && c->beam_K == 0 && D <= 1280 && nb * H <= 3 * (D / 16) && TGT <= 512 &&
           c->d.dec_layers <= 64 && 3 * (D / 16) <= c->n_cu * KD(c, cw_qkv_self_blocks_per_cu, D, TGT);
    // behind qkv_self and in front of the fused stage, one tile per block, packed weights: the x segment of the stage (qa = W'q_c x, which depends on
    // nothing the self-attention produces) rides in the V-tile blocks of qkv_self_kernel, which finish early; the attention epilogue leaves the 16-bit
    // rows the stage would round itself, and the stage is two segments over them (gemv_stack_a16_kernel).  Bit-identical (tests/test_xq_in_qkv.py).
    // The hand-off fallback (sw.no_qkv_self set), two-launch q/k/v, 9..64 rows, beam search, f32 and row-major weights keep the three segments.
    P.xq = !c->sw.no_xq_in_qkv && P.qs && P.fuse && P.nt3 == 1 && cw_sw::cw_switches().qkv_self_dbg == 0 && !c->sw.fuse_mlp && !c->sw.declayer && !c->sw.mlp_pair && !c->sw.mlp_chain;
    P.short_hist = c->hist_short && !c->sw.no_short_hist && nb > 8;   // bytes matter from 9 rows up (<= 8: latency-bound, qkv_self)
    // <= 16 rows behind the fused stage: fc1 writes gelu(.) in the 16-bit type fc2 would round it to anyway (bit-identical): fc2's activation load halves
    P.mid16 = P.fuse && !P.frag && F > 1280 && !c->sw.no_mid16;
#ifdef CW_EXPERIMENTS
    P.fuse_mlp = c->sw.fuse_mlp;
    P.mlp_pair = c->sw.mlp_pair && F % D == 0 && D % 32 == 0 && F / 32 <= 256 && F / D <= 32;
    P.mlp_chain = c->sw.mlp_chain && c->wpacked && !c->sw.no_mid16 && nb <= 8 && KD(c, cw_mlp_chain_ok, nb, D, F);
    // rows <= 8: X1 and the cross-attention as ONE persistent launch (declayer.hip): the K/V rows are requested at kernel
    // entry and stream under the GEMV tile; qa / qb / the partial sums cross CUs as granules.  Bit-identical to the two launches.
    P.dl = P.fuse && c->sw.declayer && !c->kv8 && !c->sw.fuse_mlp && P.nt3 == 1 && c->wpacked && nb <= 8 && 3 * (D / 16) <= c->n_cu &&
           nb * H * ATT_NS <= 4 * c->n_cu && D / 16 <= 128 && KD(c, cw_dec_layer_lds, D) <= (size_t)160 * 1024;
    // 17..64 rows without preparation launches (decfuse.hip: gemv_rows_kernel): the residual GEMVs own whole columns and leave
    // the stream in f32, its 16-bit fragment-major copy in d_xfrag and LayerNorm partial sums in d_rstats; the LayerNorm
    // GEMVs read that copy and normalise their outputs.  d_xfrag2 carries attention outputs and the GELU'd MLP rows.
    // 17..64 rows, DEFAULT (sw.skinny 0): the round-3 path -- gemv_prep_kernel (LayerNorm / combine -> fragment-major rows) +
    // gemv_mt_kernel per projection.  A/B only (-DCW_EXPERIMENTS builds, CW_SKINNY=1|2; measured slower in the step,
    // profiles/r04_b64_skinny_planes_rejected_*): the LayerNorm projections as skinny-M GEMMs (skinny.hip): f32 rows -> K-split
    // partial planes, finished (statistics, bias, cache / GELU epilogue) by one light launch.  The residual projections stay on
    // the 16-column K-split GEMV either way: their cost is the f32 atomics (7 ps each), which a wider tile with more K slices multiplies.
    P.sk_ok = P.frag && c->wpacked && c->ln_folded && c->rows_ln_ready && c->d_planes;
    P.skinny = P.sk_ok && c->sw.skinny >= 2;
    // greedy rows over the 16-bit cache: one cross-attention block per (row, head) over all keys writes the out-projection's
    // 16-bit rows itself (1280 blocks at 64 rows: the chip is full without key splits)
    P.xfull = P.frag && c->sw.skinny >= 1 && c->beam_K == 0 && !c->kv8 && !c->sw.rows_ln && H <= 20 && CW_N_CTX <= 24 * 64;
    P.rows = !P.skinny && P.frag && c->rows_ln_ready && c->sw.rows_ln && c->ln_folded && D <= 1280;
    // bf16 only: the 16-bit copy of the residual rows keeps 8 mantissa bits of values that are NOT normalised yet; carried as
    // hi + lo halves (two MFMAs per fragment) the LayerNorm GEMVs see 16 bits, more than the rounded LN(x) of the prepared path
    P.lo_off = (!c->sw.no_rows_hilo && !c->f16) ? 64 * (D / 8) : 0;
    P.pf = c->sw.prefetch > 0 && c->bf16 && c->beam_K == 0 && !c->kv8;
#endif
    return P;
}
bool step_plan_xq(const cw_ctx* c, int nb) { return plan_step(c, nb).xq; }   // cw_test_decode_state: which stack launch nb rows take
// kernel launches behind a stage.  17..64 rows: a LayerNorm / combining GEMV is gemv_prep_kernel + gemv_mt_kernel
static int stage_launches(const StepPlan& P, int kind) {
    const bool prepared = kind == DST_QKV || kind == DST_CROSS_Q || kind == DST_FC1 || kind == DST_CROSS_O, owned = P.own && (kind == DST_FC1 || kind == DST_CROSS_O);
    return (P.frag && !P.skinny && !P.rows && !P.xfull && prepared && !owned) ? 2 : 1;
}
// Books the next launch of the layer and tells whether to issue it.  cw_time_decode_stage runs ONE launch (stage_sel) of ONE layer (layer_sel)
// through this very code: the kernels it times are the ones the step launches, with the step's arguments; `call` is evaluated for no other launch.
static bool stage(cw_ctx* c, const StepPlan& P, int kind) {
    const int s = c->stage_count++;
    if (s < CW_MAX_DEC_STAGES) { c->stage_kind[s] = kind; c->stage_launches[s] = stage_launches(P, kind); }
    return c->stage_sel < 0 || c->stage_sel == s;
}
#define STG(kind, call) do { if (stage(c, P, (kind))) CWCHK(c, call); } while (0)
static EpiParams resid_epi(float* x, const float* bias, int D) { EpiParams ep = epi0(); ep.outf = x; ep.resid = x; ep.bias = bias; ep.ldo = D; return ep; }   // x += W a + bias
EpiParams qkv_epi(cw_ctx* c, LayerW& L) {   // q -> c->dq; k, v appended to the self-attention cache at pos[b]
    EpiParams ep = epi0(); ep.outf = c->dq; ep.out1 = L.sk; ep.out2 = L.sv; ep.bias = L.bqkv;
    ep.H = c->d.n_heads; ep.S_pad = c->d.max_target_positions; ep.d_model = c->d.d_model; ep.row_pos = c->d_pos;
    return ep;
}
EpiParams cross_q_epi(cw_ctx* c, LayerW& L) { EpiParams ep = epi0(); ep.outf = c->dq; ep.bias = L.bq_c; ep.ldo = c->d.d_model; return ep; }
static EpiParams fc1_epi(cw_ctx* c, LayerW& L) { EpiParams ep = epi0(); ep.outf = c->dmid; ep.out = c->d_xfrag2; ep.bias = L.b1; ep.ldo = c->d.ffn_dim; return ep; }
// x += W a + bias.  frag: a = the 16-bit fragment-major rows a producer left in xf; otherwise the f32 (x16: 16-bit) rows `a`
int gemv_resid(cw_ctx* c, bool frag, const float* a, void* xf, int nb, int K, const void* W, const float* bias, float* x, int x16) {
    const int D = c->d.d_model;
    EpiParams ep = resid_epi(x, bias, D); ep.x16 = x16;
    if (frag) return KD(c, cw_launch_gemv, true, EPI_RESID_F32, nullptr, nb, K, W, D, nullptr, nullptr, ep, c->st, nullptr, xf, c->wpacked);
    return gemv_ln(c, EPI_RESID_F32, a, nb, K, W, D, nullptr, nullptr, ep);
}
// keys split over ATT_NS blocks per (row, head).  q null (fused layer): the kernel finishes q_c = rstd(x1) (qa + qb - mean(x1) W'q_c 1) + b'q_c
static CrossSplitParams cross_params(cw_ctx* c, const StepPlan& P, LayerW& L, int l, int nb, const float* q) {
    const int H = c->d.n_heads;
    CrossSplitParams p{q, L.ck, L.cv, CW_N_CTX, c->d_part_o, c->d_part_ml, c->d.n_align > 0 ? c->d_align : nullptr, c->d_align_ml,
                       c->d_align_slot + (size_t)l * H, c->d_pos, c->d.n_align, c->align_rows, nb, H};
    p.kv_div = c->beam_K > 0 ? c->beam_K : 1;
    if (!q) { p.qa = c->d_qa; p.qb = c->d_qb; p.qw = L.q_wsum; p.qbias = L.bq_c; p.pstats = c->d_pstats; p.n_pstats = (c->d.d_model / 16 + P.nt3 - 1) / P.nt3; }
    return p;
}
int cross_attn(cw_ctx* c, LayerW& L, CrossSplitParams p) {   // over the 16-bit cache or its e4m3 copy
    if (c->kv8) { p.K = L.ck8; p.V = L.cv8; p.kv_scale = L.kvs; return KD(c, cw_launch_attn_cross_split_fp8, p, c->st); }
    return KD(c, cw_launch_attn_cross_split, true, p, c->st);
}
// the out-projection GEMV combines the key-split partials; x += Wo_c a_c + bo_c in place
static int cross_out(cw_ctx* c, const StepPlan& P, LayerW& L, int nb, float* x) {
    const int D = c->d.d_model;
    const CombineParams cb{c->d_part_ml, c->d.n_heads, nb * D};
    return KD(c, cw_launch_gemv, true, EPI_RESID_F32, c->d_part_o, nb, D, L.wo_c, D, nullptr, nullptr, resid_epi(x, L.bo_c, D), c->st, &cb, (nb <= 16 || P.frag) ? c->d_xfrag : nullptr, c->wpacked);
}
// LN + fc1 + GELU, fc2 + residual on the stream in x.  17..64 rows: LayerNorm preparation + gemv_mt launches, GELU rows fragment-major
static int launch_mlp(cw_ctx* c, const StepPlan& P, LayerW& L, int nb, float* x) {
    const int D = c->d.d_model, F = c->d.ffn_dim;
    STG(DST_FC1, gemv_ln(c, P.frag ? EPI_GELU_FRAG : P.mid16 ? EPI_GELU : EPI_GELU_F32, x, nb, D, L.w1, F, L.ln2_g, c->ln_folded ? nullptr : L.ln2_b, fc1_epi(c, L)));
    STG(DST_FC2, gemv_resid(c, P.frag, P.mid16 ? (const float*)c->d_xfrag2 : c->dmid, c->d_xfrag2, nb, F, L.w2, L.b2, x, P.mid16 ? 1 : 0));
    return CW_OK;
}
// self-attention over the cache rows the q/k/v projection just appended to: c->dq -> c->dattn
static int self_attn(cw_ctx* c, const StepPlan& P, LayerW& L, int nb) {
    DecAttnParams p = dec_attn(c->dq, L.sk, L.sv, c->d.max_target_positions, 0, c->d_pos, c->dattn, nb, c->d.n_heads);
    if (P.frag && !P.fuse) p.out_frag = (unsigned short*)c->d_xfrag2;   // the fused stage reads the f32 rows
    if (c->beam_K > 0) p.anc = c->d_anc;
    p.short_hist = P.short_hist ? 1 : 0;
    return KD(c, cw_launch_attn_decode, c->bf16, p, c->st);
}
// Self-attention front of layer l on the stream in x: qkv_self in one launch, or LN + fused q/k/v projection and attn_decode
static int layer_self_attention(cw_ctx* c, const StepPlan& P, int l, int nb, const float* x) {
    const int D = c->d.d_model, H = c->d.n_heads, TGT = c->d.max_target_positions;
    LayerW& L = c->dec[l];
    if (!P.qs) {
        STG(DST_QKV, gemv_ln(c, EPI_QKV_CACHE, x, nb, D, L.wqkv, 3 * D, L.ln1_g, c->ln_folded ? nullptr : L.ln1_b, qkv_epi(c, L)));
        STG(DST_SELF_ATTN, self_attn(c, P, L, nb));
        return CW_OK;
    }
    QkvSelfParams qp = zeroed<QkvSelfParams>();
    qp.x = x; qp.W = L.wqkv; qp.bias = L.bqkv; qp.sk = L.sk; qp.sv = L.sv; qp.cap = TGT; qp.pos = c->d_pos; qp.out = c->dattn;
    qp.gq = c->d_gq2; qp.gkv = c->d_gkv; qp.epoch = c->d_epoch; qp.layer = l; qp.err = c->d_err; qp.Mb = nb; qp.D = D; qp.H = H; qp.fail_pos = c->fail_pos; qp.wnt = !c->sw.no_wnt ? 1 : 0;
    const int dbg = cw_sw::cw_switches().qkv_self_dbg;   // 1: tiles fused, attention by attn_decode_kernel behind it (bisecting aid)
    if (dbg) { qp.q_plain = c->dq; qp.no_attn = 1; }
    if (P.xq) { qp.xq_W = L.ws3; qp.xq_bias = L.qa_bias; qp.xq_wsum = !c->sw.no_stack_center ? L.q_wsum : nullptr; qp.xq_out = c->d_qa; qp.out16 = c->d_attn16; }
    STG(DST_QKV_SELF, KD(c, cw_launch_qkv_self, qp, c->st));
    if (dbg) STG(DST_SELF_ATTN, self_attn(c, P, L, nb));
    return CW_OK;
}
// X1 over [W'q_c ; W'q_c Wo ; Wo]:  qa = W'q_c x + W'q_c bo,  qb = (W'q_c Wo) a,  x1 = x + Wo a + bo
static StackParams stack_params(cw_ctx* c, LayerW& L, int nb, const float* xin, float* xalt) {
    const int D = c->d.d_model, TD = D / 16;
    StackParams sp = zeroed<StackParams>();
    sp.W = L.ws3; sp.wpk = c->wpacked ? 1 : 0; sp.wnt = !c->sw.no_wnt ? 1 : 0; sp.K = D; sp.Mb = nb; sp.nseg = 3;
    sp.seg[0].x = xin;      sp.seg[0].bias = L.qa_bias; sp.seg[0].out = c->d_qa; sp.seg[0].tile0 = 0;      sp.seg[0].n_tiles = TD; sp.seg[0].epi = 0;
    sp.seg[0].wsum = !c->sw.no_stack_center ? L.q_wsum : nullptr;   // x is rounded as x - mean(x): the operand the cross-attention LayerNorm is sensitive to
    sp.seg[1].x = c->dattn; sp.seg[1].bias = nullptr;   sp.seg[1].out = c->d_qb; sp.seg[1].tile0 = TD;     sp.seg[1].n_tiles = TD; sp.seg[1].epi = 0;
    sp.seg[2].x = c->dattn; sp.seg[2].bias = L.bo;      sp.seg[2].out = xalt;    sp.seg[2].tile0 = 2 * TD; sp.seg[2].n_tiles = TD; sp.seg[2].epi = 1;
    sp.seg[2].resid = xin; sp.seg[2].pstats = c->d_pstats;   // LayerNorm partial sums of x1 for the cross-attention
    return sp;
}
// The fused layer behind the self-attention front (<= 16 rows; 17..64 rows in row groups): stack stage, cross-attention, then the column-owning
// tail (33..64 rows) or the combining out-projection + fc1 / fc2.  Reads the stream from xin, leaves x1, x2, x3 in xalt and exchanges the two.
static int layer_fused(cw_ctx* c, const StepPlan& P, int l, int nb, float*& xin, float*& xalt) {
    const int D = c->d.d_model, H = c->d.n_heads, F = c->d.ffn_dim;
    LayerW& L = c->dec[l];
    if (P.xq) {   // qa came out of qkv_self_kernel: qb = (W'q_c Wo) a, x1 = x + Wo a + bo over the 16-bit rows of a
        StackA16Params sp = zeroed<StackA16Params>();
        sp.W = L.ws3; sp.a16 = c->d_attn16; sp.resid = xin; sp.bias = L.bo; sp.qb = c->d_qb; sp.x1 = xalt; sp.pstats = c->d_pstats; sp.K = D; sp.Mb = nb; sp.wnt = !c->sw.no_wnt ? 1 : 0;
        STG(DST_STACK, KD(c, cw_launch_gemv_stack_a16, sp, c->st));
    } else STG(DST_STACK, KD(c, cw_launch_gemv_stack, stack_params(c, L, nb, xin, xalt), P.nt3, c->st));
    const CrossSplitParams p = cross_params(c, P, L, l, nb, nullptr);
    STG(DST_CROSS_ATTN, cross_attn(c, L, p));
    if (P.own) {
        // combine (+ the rows' centres) -> d_xfrag;  x2 = x1 + Wo_c a_c + bo_c in place, y = x2 - c -> d_xfrag2, partial sums;
        // fc1 normalises on its accumulator, GELU rows -> d_xfrag;  fc2 as before
        const CombineParams cb{c->d_part_ml, H, nb * D, c->d_pstats, p.n_pstats, c->d_cvec};
        STG(DST_OTHER, KD(c, cw_launch_rows_combine, c->d_part_o, nb, D, cb, c->d_xfrag, c->st));
        STG(DST_CROSS_O, KD(c, cw_launch_gemv_own, c->d_xfrag, nb, D, L.wo_c, D, resid_epi(xalt, L.bo_c, D), c->d_cvec, c->d_xfrag2, c->d_ostats, c->st, c->wpacked));
        EpiParams ep = epi0(); ep.out = c->d_xfrag; ep.bias = L.b1; ep.ldo = F;
        STG(DST_FC1, KD(c, cw_launch_gemv_lna, c->d_xfrag2, nb, D, L.w1, F, ep, c->d_ostats, D / (16 * KD(c, cw_gemv_own_nt, D)), L.u1_wsum, c->st, c->wpacked));
        STG(DST_FC2, gemv_resid(c, true, nullptr, c->d_xfrag, nb, F, L.w2, L.b2, xalt));
    } else {
        STG(DST_CROSS_O, cross_out(c, P, L, nb, xalt));
        CWCHK(c, launch_mlp(c, P, L, nb, xalt));
    }
    std::swap(xin, xalt);
    return CW_OK;
}
// The unfused layer behind the self-attention front (f32 parity engine, CW_NO_FUSE6, row-major weights above 16 rows, beam search over
// the e4m3 cache, ...): gemv_ln everywhere; the f32 engine's cross-attention is attn_decode.  The stream stays in c->dx.
static int layer_unfused(cw_ctx* c, const StepPlan& P, int l, int nb) {
    const int D = c->d.d_model, H = c->d.n_heads;
    LayerW& L = c->dec[l];
    STG(DST_O_PROJ, gemv_resid(c, P.frag, c->dattn, c->d_xfrag2, nb, D, L.wo, L.bo, c->dx));
    // cross-attention: LN + q projection, attention over the cached encoder K/V
    STG(DST_CROSS_Q, gemv_ln(c, EPI_STORE_F32, c->dx, nb, D, L.wq_c, D, L.lnc_g, c->ln_folded ? nullptr : L.lnc_b, cross_q_epi(c, L)));
    if (c->bf16) {
        STG(DST_CROSS_ATTN, cross_attn(c, L, cross_params(c, P, L, l, nb, c->dq)));
        STG(DST_CROSS_O, cross_out(c, P, L, nb, c->dx));
    } else {
        DecAttnParams p = dec_attn(c->dq, L.ck, L.cv, CW_N_CTX, CW_N_CTX, c->d_pos, c->dattn, nb, H);
        p.align_out = c->d.n_align > 0 ? c->d_align : nullptr; p.align_slot = c->d_align_slot + (size_t)l * H;
        p.n_align = c->d.n_align; p.align_rows = c->align_rows; p.kv_div = c->beam_K > 0 ? c->beam_K : 1;
        STG(DST_CROSS_ATTN, KD(c, cw_launch_attn_decode, c->bf16, p, c->st));
        STG(DST_CROSS_O, gemv_resid(c, false, c->dattn, nullptr, nb, D, L.wo_c, L.bo_c, c->dx));
    }
    return launch_mlp(c, P, L, nb, c->dx);
}
// persistent decoder-layer launch of layer l (declayer.hip): fused out-projection / cross-query stage + cross-attention
DecLayerParams dec_layer_params(cw_ctx* c, int l, int nb, const float* xin, float* xalt) {
    const int D = c->d.d_model, H = c->d.n_heads, TGT = c->d.max_target_positions;
    LayerW& L = c->dec[l];
    DecLayerParams dp = zeroed<DecLayerParams>();
    dp.Ws = L.ws3; dp.x = xin; dp.a = c->dattn; dp.qa_bias = L.qa_bias; dp.q_wsum = !c->sw.no_stack_center ? L.q_wsum : nullptr;
    dp.bo = L.bo; dp.x1 = xalt;
    dp.K = L.ck; dp.V = L.cv; dp.n_keys = CW_N_CTX; dp.part_o = c->d_part_o; dp.part_ml = c->d_part_ml;
    dp.align_out = c->d.n_align > 0 ? c->d_align : nullptr; dp.align_ml = c->d_align_ml;
    dp.align_slot = c->d_align_slot + (size_t)l * H; dp.pos = c->d_pos; dp.n_align = c->d.n_align; dp.align_rows = c->align_rows;
    dp.qw = L.q_wsum; dp.qbias = L.bq_c;
    dp.gq = c->d_gq; dp.gps = c->d_gps; dp.epoch = c->d_epoch; dp.layer = l; dp.err = c->d_err;
    dp.Mb = nb; dp.D = D; dp.H = H;
    dp.kv_wait = cw_sw::cw_switches().dl_kvwait;
    return dp;
}

#ifdef CW_EXPERIMENTS
// ---- the measured-and-rejected variants (A/B and differential tests only; DESIGN.md "A/B switches") ----------------------------------
// layer l's streams are touched while layer l - 1 runs (side stream: a parallel graph branch)
static int launch_prefetch_layer(cw_ctx* c, const StepPlan& P, int l, int nb) {
    HIPCHK(c, hipEventRecord(c->ev_pf[0], c->st));
    HIPCHK(c, hipStreamWaitEvent(c->st2, c->ev_pf[0], 0));
    const int D = c->d.d_model, F = c->d.ffn_dim, H = c->d.n_heads;
    const size_t e = c->esz;
    LayerW& L = c->dec[l];
    PrefetchRanges r = zeroed<PrefetchRanges>();
    auto add = [&](const void* p, size_t bytes) { if (p && bytes && r.count < 8) { r.p[r.count] = (const char*)p; r.n[r.count] = bytes; ++r.count; } };
    add(L.wqkv, (size_t)3 * D * D * e);
    if (P.fuse) add(L.ws3, (size_t)3 * D * D * e);
    else { add(L.wo, (size_t)D * D * e); add(L.wq_c, (size_t)D * D * e); }
    add(L.ck, (size_t)nb * H * CW_N_CTX * 64 * e);
    add(L.cv, (size_t)nb * H * CW_N_CTX * 64 * e);
    add(L.wo_c, (size_t)D * D * e);
    add(L.w1, (size_t)F * D * e);
    add(L.w2, (size_t)D * F * e);
    const int wide = cw_sw::cw_switches().prefetch_wide;
    const int what = cw_sw::cw_switches().prefetch_what;   // 1 weights, 2 cross K/V, 3 both
    if (!(what & 1)) { int k = 0; for (int i = 0; i < r.count; ++i) if (r.p[i] == (const char*)L.ck || r.p[i] == (const char*)L.cv) { r.p[k] = r.p[i]; r.n[k] = r.n[i]; ++k; } r.count = k; }
    if (!(what & 2)) { int k = 0; for (int i = 0; i < r.count; ++i) if (r.p[i] != (const char*)L.ck && r.p[i] != (const char*)L.cv) { r.p[k] = r.p[i]; r.n[k] = r.n[i]; ++k; } r.count = k; }
    if (wide) hipLaunchKernelGGL(prefetch_kernel<1>, dim3(c->sw.prefetch), dim3(256), 0, c->st2, r, c->d_pf_sink);
    else hipLaunchKernelGGL(prefetch_kernel<0>, dim3(c->sw.prefetch), dim3(256), 0, c->st2, r, c->d_pf_sink);
    return CW_OK;
}

// 17..64 rows, unfused, with the rows path (CW_ROWS_LN), the skinny GEMMs (CW_SKINNY=2) and / or the full-key cross-attention (CW_SKINNY=1|2):
// the whole layer, self-attention front included; the stream stays in c->dx.  ln_nblk: statistics planes the rows path's last producer left.
static int layer_unfused_ab(cw_ctx* c, const StepPlan& P, int l, int nb, int& ln_nblk) {
    const int D = c->d.d_model, H = c->d.n_heads, F = c->d.ffn_dim;
    LayerW& L = c->dec[l];
    auto sk_ln = [&](int epi, const void* W, int N, const float* wsum, const EpiParams& ep) -> int {
        SkinnyParams sp = zeroed<SkinnyParams>();
        sp.x = c->dx; sp.W = W; sp.Mb = nb; sp.K = D; sp.N = N; sp.planes = c->d_planes; sp.stats = c->d_sk_stats;
        int smax = (int)(c->planes_cap / ((size_t)nb * N));
        if (smax > 16) smax = 16;
        const int nks = KD(c, cw_skinny_pick_nks, N, D, smax);
        if (nks < 1) return CW_ERR_INVALID;
        int r = KD(c, cw_launch_skinny, 0, sp, nks, c->st);
        if (r != CW_OK) return r;
        SkinnyFinishParams fp = zeroed<SkinnyFinishParams>();
        fp.planes = c->d_planes; fp.S = (D / 32) / nks; fp.Mb = nb; fp.N = N; fp.x = c->dx; fp.K = D; fp.wsum = wsum; fp.ep = ep; fp.stats = c->d_sk_stats;
        return KD(c, cw_launch_skinny_finish, epi, fp, c->st);
    };
    auto rows_params = [&](const void* xf, const void* W, int K, int N, const EpiParams& ep) {
        RowsParams rp = zeroed<RowsParams>();
        rp.xf = xf; rp.W = W; rp.Mb = nb; rp.K = K; rp.N = N; rp.wpk = c->wpacked ? 1 : 0; rp.ep = ep; rp.lo_off = P.lo_off;
        return rp;
    };
    auto rows_consume = [&](int epi, const void* W, int N, const EpiParams& ep, const float* wsum) -> int {
        RowsParams rp = rows_params(c->d_xfrag, W, D, N, ep);
        rp.ln_pstats = c->d_rstats; rp.ln_nblk = ln_nblk; rp.ln_wsum = wsum;
        return KD(c, cw_launch_gemv_rows, epi, false, rp, c->st);
    };
    auto rows_produce = [&](const void* W, int K, const float* bias) -> int {   // x += W a + b over the rows in d_xfrag2
        RowsParams rp = rows_params(c->d_xfrag2, W, K, D, resid_epi(c->dx, bias, D));
        rp.xf_out = c->d_xfrag; rp.pstats_out = c->d_rstats;
        ln_nblk = D / 16;
        return KD(c, cw_launch_gemv_rows, (int)EPI_RESID_F32, true, rp, c->st);
    };
    auto ln_gemv = [&](int epi, const void* W, int N, const float* wsum, const float* g, const float* b, const EpiParams& ep) -> int {   // W LN(x)
        if (P.skinny) return sk_ln(epi, W, N, wsum, ep);
        if (P.rows) return rows_consume(epi, W, N, ep, wsum);
        return gemv_ln(c, epi, c->dx, nb, D, W, N, g, c->ln_folded ? nullptr : b, ep);
    };
    auto resid_gemv = [&](const void* W, int K, const float* bias) -> int { return P.rows ? rows_produce(W, K, bias) : gemv_resid(c, true, nullptr, c->d_xfrag2, nb, K, W, bias, c->dx); };
    STG(DST_QKV, ln_gemv(EPI_QKV_CACHE, L.wqkv, 3 * D, L.qkv_wsum, L.ln1_g, L.ln1_b, qkv_epi(c, L)));
    STG(DST_SELF_ATTN, self_attn(c, P, L, nb));
    STG(DST_O_PROJ, resid_gemv(L.wo, D, L.bo));
    CrossSplitParams p = cross_params(c, P, L, l, nb, c->dq);
    if (P.xfull && P.sk_ok) {   // W'q_c (x - c) over K slices -> planes; the attention blocks apply rstd (sum - mean W'q_c 1) + b'q_c
        SkinnyParams sp = zeroed<SkinnyParams>();
        sp.x = c->dx; sp.W = L.wq_c; sp.Mb = nb; sp.K = D; sp.N = D; sp.planes = c->d_planes;
        const int nks = KD(c, cw_skinny_pick_nks, D, D, (int)(c->planes_cap / ((size_t)nb * D)));
        if (nks < 1) return fail(c, CW_ERR_INVALID, "no K split for the cross-attention query GEMM");
        STG(DST_OTHER, KD(c, cw_launch_skinny, 0, sp, nks, c->st));
        p.q = nullptr; p.xstat = c->dx; p.qa = c->d_planes; p.q_planes = (D / 32) / nks; p.q_plane_stride = nb * D;
        p.qw = L.q_wsum; p.qbias = L.bq_c;
    } else STG(DST_CROSS_Q, ln_gemv(EPI_STORE_F32, L.wq_c, D, L.q_wsum, L.lnc_g, L.lnc_b, cross_q_epi(c, L)));   // (xfull excludes the rows path)
    if (P.xfull) {   // one block per (row, head) over all keys, 16-bit cache; writes the out-projection's fragment-major rows itself
        p.a_frag = c->d_xfrag;
        STG(DST_CROSS_ATTN, KD(c, cw_launch_attn_cross_split, true, p, c->st));
        STG(DST_CROSS_O, gemv_resid(c, true, nullptr, c->d_xfrag, nb, D, L.wo_c, L.bo_c, c->dx));
    } else {
        STG(DST_CROSS_ATTN, cross_attn(c, L, p));
        if (P.rows) {
            const CombineParams cb{c->d_part_ml, H, nb * D};
            STG(DST_OTHER, KD(c, cw_launch_rows_combine, c->d_part_o, nb, D, cb, c->d_xfrag2, c->st));
            STG(DST_CROSS_O, rows_produce(L.wo_c, D, L.bo_c));
        } else STG(DST_CROSS_O, cross_out(c, P, L, nb, c->dx));
    }
    STG(DST_FC1, ln_gemv(EPI_GELU_FRAG, L.w1, F, L.u1_wsum, L.ln2_g, L.ln2_b, fc1_epi(c, L)));
    STG(DST_FC2, resid_gemv(L.w2, F, L.b2));
    return CW_OK;
}

// The fused layer behind the self-attention front with stage A of declayer.hip (CW_DECLAYER), the X2 tail (CW_FUSE_MLP), mlp_pair or
// mlp_chain in it (rows <= 8).  Stream buffers as in layer_fused, except that X2 writes the stream back to xin (no exchange).
static int layer_fused_ab(cw_ctx* c, const StepPlan& P, int l, int nb, float*& xin, float*& xalt) {
    const int D = c->d.d_model, F = c->d.ffn_dim, TD = D / 16, TF = F / 16;
    LayerW& L = c->dec[l];
    if (P.dl) STG(DST_STACK_CROSS, KD(c, cw_launch_dec_layer, dec_layer_params(c, l, nb, xin, xalt), c->n_cu, c->st));
    else {
        StackParams sp = stack_params(c, L, nb, xin, xalt);
        if (P.fuse_mlp) { sp.zero = c->d_u1; sp.zero_n4 = nb * F / 4; }   // X2 below accumulates its two halves into u1
        STG(DST_STACK, KD(c, cw_launch_gemv_stack, sp, P.nt3, c->st));
    }
    CrossSplitParams p = cross_params(c, P, L, l, nb, nullptr);
    if (P.fuse_mlp) {
        // A/B (CW_FUSE_MLP=1), measured slower: cross out-projection + fc1 fused the same way.  Needs the
        // finished attention output in one plane (one block per (row, head): 17 us against 12) and makes every fc2 block
        // redo the statistics and the GELU of its K slice.
        p.a_out = c->dattn; p.xstat = xalt;
        STG(DST_CROSS_ATTN, KD(c, cw_launch_attn_cross_split, true, p, c->st));
        // X2 over [W'1 ; W'1 Wo_c ; Wo_c]:  u1 = W'1 x1 + W'1 bo_c + (W'1 Wo_c) a_c (two halves, atomics into the zeros X1
        // left: two commutative additions, so the order does not matter),  x2 = x1 + Wo_c a_c + bo_c (+ a copy that
        // fc2 takes the LayerNorm statistics of while its atomics are already modifying the stream)
        StackParams sp = zeroed<StackParams>();
        sp.W = L.ws5; sp.wpk = c->wpacked ? 1 : 0; sp.K = D; sp.Mb = nb; sp.nseg = 3;
        sp.seg[0].x = xalt;     sp.seg[0].bias = L.u1_bias; sp.seg[0].out = c->d_u1; sp.seg[0].tile0 = 0;      sp.seg[0].n_tiles = TF; sp.seg[0].epi = 2;
        sp.seg[0].wsum = !c->sw.no_stack_center ? L.u1_wsum : nullptr;
        sp.seg[1].x = c->dattn; sp.seg[1].bias = nullptr;   sp.seg[1].out = c->d_u1; sp.seg[1].tile0 = TF;     sp.seg[1].n_tiles = TF; sp.seg[1].epi = 2;
        sp.seg[2].x = c->dattn; sp.seg[2].bias = L.bo_c;    sp.seg[2].out = xin;     sp.seg[2].tile0 = 2 * TF; sp.seg[2].n_tiles = TD; sp.seg[2].epi = 1;
        sp.seg[2].resid = xalt; sp.seg[2].out2 = c->dx2c;
        STG(DST_STACK, KD(c, cw_launch_gemv_stack, sp, c->sw.stack_nt5, c->st));
        // fc2: mid = gelu(rstd(x2) (u1 - mean(x2) W'1 1) + b'1) on load; x3 = x2 + W2 mid + b2 in place
        Fc2xParams fp{c->dx2c, c->d_u1, L.u1_wsum, L.b1, L.w2, L.b2, xin, nb, D, F, c->wpacked ? 1 : 0};
        STG(DST_FC2, KD(c, cw_launch_gemv_fc2x, fp, c->st));
        return CW_OK;
    }
    if (!P.dl) STG(DST_CROSS_ATTN, cross_attn(c, L, p));
    STG(DST_CROSS_O, cross_out(c, P, L, nb, xalt));
    if (P.mlp_pair) {
        // LN + fc1 + GELU, group barrier, fc2 + residual in one launch (decfuse.hip: mlp_pair_kernel)
        MlpPairParams mp{xalt, L.w1, L.b1, L.w2, L.b2, c->d_xfrag2, c->d_bar, c->d_err, nb, D, F, c->wpacked ? 1 : 0, c->sw.mlp_pair_fence ? 1 : 0};
        STG(DST_MLP_PAIR, KD(c, cw_launch_mlp_pair, mp, c->st));
    } else if (P.mlp_chain) {
        // LN + fc1 + GELU and fc2 + residual in ONE launch: fc2's blocks request their weights at kernel entry and wait for
        // the fc1 blocks' flags instead of a kernel boundary (declayer.hip: mlp_chain_kernel); bit-identical
        MlpChainParams mp = zeroed<MlpChainParams>();
        mp.x = xalt; mp.W1 = L.w1; mp.b1 = L.b1; mp.W2 = L.w2; mp.b2 = L.b2; mp.xio = xalt; mp.mid = c->d_xfrag2;
        mp.flags = c->d_gflag; mp.epoch = c->d_epoch; mp.layer = l; mp.err = c->d_err; mp.Mb = nb; mp.D = D; mp.F = F;
        STG(DST_MLP_CHAIN, KD(c, cw_launch_mlp_chain, mp, c->st));
    } else CWCHK(c, launch_mlp(c, P, L, nb, xalt));
    std::swap(xin, xalt);
    return CW_OK;
}
#endif   // CW_EXPERIMENTS

// One decoder forward for the nb rows at the positions held in c->d_pos (device): plan, layers, logits.  Which launches a layer
// has at nb rows: plan_step and the three layer functions above (tests/golden/decode_stage_tables.json lists them per configuration).
int decode_step(cw_ctx* c, int nb, bool want_logits) {
    const StepPlan P = plan_step(c, nb);
    float *xin = c->dx, *xalt = c->dx1;   // xin holds the residual stream whenever a layer function returns
#ifdef CW_EXPERIMENTS
    int ln_nblk = 1;
    if (P.rows) CWCHK(c, KD(c, cw_launch_rows_prep, c->dx, nb, c->d.d_model, c->d_xfrag, c->d_rstats, P.lo_off, c->st));
#endif
    const int l_lo = c->layer_sel >= 0 ? c->layer_sel : 0, l_hi = c->layer_sel >= 0 ? c->layer_sel + 1 : c->d.dec_layers;
    for (int l = l_lo; l < l_hi; ++l) {
        c->stage_count = 0;
#ifdef CW_EXPERIMENTS
        if (P.pf && l + 1 < c->d.dec_layers) CWCHK(c, launch_prefetch_layer(c, P, l + 1, nb));
        if (P.rows || P.skinny || P.xfull) { CWCHK(c, layer_unfused_ab(c, P, l, nb, ln_nblk)); continue; }
#endif
        CWCHK(c, layer_self_attention(c, P, l, nb, xin));
#ifdef CW_EXPERIMENTS
        if (P.fuse && (P.dl || P.fuse_mlp || P.mlp_pair || P.mlp_chain)) { CWCHK(c, layer_fused_ab(c, P, l, nb, xin, xalt)); continue; }
#endif
        CWCHK(c, P.fuse ? layer_fused(c, P, l, nb, xin, xalt) : layer_unfused(c, P, l, nb));
    }
#ifdef CW_EXPERIMENTS
    if (P.pf && c->d.dec_layers > 1) {           // join the side stream (required before the capture ends; the last prefetch is long done)
        HIPCHK(c, hipEventRecord(c->ev_pf[1], c->st2));
        HIPCHK(c, hipStreamWaitEvent(c->st, c->ev_pf[1], 0));
    }
#endif
    if (want_logits) CWCHK(c, launch_logits(c, nb, xin));
    return CW_OK;
}
#undef STG

int launch_sample(cw_ctx* c, int nb) {
    SampleParams sp = zeroed<SampleParams>();
    sp.logits = c->dlogits; sp.V = c->d.vocab_size; sp.ldv = c->Vpad; sp.B = nb; sp.mask = c->d_mask;
    sp.eos = c->gen.eos_token_id; sp.pad = c->gen.pad_token_id;
    sp.timestamp_begin = c->gen.no_timestamps_token_id + 1;
    sp.max_initial_timestamp_index = c->gen.max_initial_timestamp_index;
    sp.cfg = c->d_cfg; sp.pos = c->d_pos;
    sp.ids_stride = c->d.max_target_positions; sp.ids = c->d_ids; sp.forced = c->d_forced;
    sp.argmax_trace = c->d_argmax; sp.last_ts_tok = c->d_last_ts; sp.finished = c->d_finished;
    sp.n_unfinished = c->d_nunf;
    sp.embed = c->embed; sp.pos_embed = c->dec_pos; sp.x_out = c->dx; sp.d = c->d.d_model; sp.embed_bf16 = c->bf16 ? 1 : 0;
    sp.partials = c->d_sample_part;
    if (c->score_tokens) { sp.lp_sum = c->d_lp_sum; sp.lp_cnt = c->d_lp_cnt; }
    if (c->tok_lp_on) sp.tok_lp = c->d_tok_lp;
    if (c->tok_lp_on && c->top_k > 0) { sp.top_k = c->top_k; sp.top_part = c->d_top_part; sp.top_id = c->d_top_id; sp.top_lp = c->d_top_lp; }
    if (c->tok_lp_on && c->tok_ent_on) { sp.tok_ent = c->d_tok_ent; sp.ent_part = c->d_ent_part; }
    if (c->sb_n > 0) sp.seq_bias = c->d_seq_bias;
    sp.epoch = c->d_epoch;
    sp.samp = c->d_samp; sp.pert = c->d_sample_pert;
    return KD(c, cw_launch_sample, sp, c->st);
}

// decoder forward + logits + sampling for one position, captured once per batch size as a hipGraph
// (~260 launches -> one replay; every per-step value lives in device memory: d_pos, d_cfg).
static int run_step(cw_ctx* c, int nb) {
    const bool graph_ok = !c->sw.no_graph && !c->logits_capture;
    if (!graph_ok) {
        CWCHK(c, decode_step(c, nb, true));
        return launch_sample(c, nb);
    }
    const int gi = nb + (plan_step(c, nb).short_hist ? 65 : 0);
    if (!c->step_graph[gi]) {
        hipGraph_t g = nullptr;
        HIPCHK(c, hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal));
        int r = decode_step(c, nb, true);
        if (r == CW_OK) r = launch_sample(c, nb);
        hipError_t e = hipStreamEndCapture(c->st, &g);
        if (r != CW_OK) { if (g) hipGraphDestroy(g); return r; }
        if (e != hipSuccess) return fail(c, CW_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        e = hipGraphInstantiate(&c->step_graph[gi], g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (e != hipSuccess) return fail(c, CW_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    HIPCHK(c, hipGraphLaunch(c->step_graph[gi], c->st));
    return CW_OK;
}

// ---- in-launch hand-offs that gave up -------------------------------------------------------------------------------------
// The kernels of declayer.hip (and the A/B kernel mlp_pair_kernel) let blocks of ONE launch wait for each other.  That needs the
// waiting blocks and the ones they wait for on the chip together -- always true when the context has the GPU to itself, not
// when other processes fill it (eight ranks on one device: tests/test_dist_gloo.py).  A block that polls DL_SPIN_LIMIT times
// without success sets d_err and carries on with garbage.  The entry points below check the flag when their work has drained
// and, if it is set, switch every such kernel off for this context (for good) and run the call again: the launch-per-stage
// kernels are bit-identical, so the caller sees the result it would have had, late.
#define CW_HANDOFF_RETRY 0x7e57
void drop_step_graphs(cw_ctx* c) { for (auto& ge : c->step_graph) if (ge) { hipGraphExecDestroy(ge); ge = nullptr; } }   // kernel arguments are baked into the graphs
static bool handoffs_on(const cw_ctx* c) { return !c->sw.no_qkv_self || c->sw.mlp_chain || c->sw.declayer || c->sw.mlp_pair; }
static int handoff_gave_up(cw_ctx* c, bool* gave_up, int* word = nullptr) {
    int e = 0;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(&e, c->d_err, 4, hipMemcpyDeviceToHost));
    *gave_up = e != 0;
    if (word) *word = e;
    if (e) { HIPCHK(c, hipMemset(c->d_err, 0, 4)); HIPCHK(c, hipMemset(c->d_bar, 0, 64 * 4)); }
    return CW_OK;
}
static int handoffs_off(cw_ctx* c, const char* where) {
    if (!handoffs_on(c)) return fail(c, CW_ERR_HIP, "%s: an in-launch hand-off gave up although none is enabled", where);
    c->sw.no_qkv_self = true;
    c->sw.mlp_chain = c->sw.declayer = c->sw.mlp_pair = false;
    drop_step_graphs(c);
    if (c->handoff_fallbacks++ == 0)
        fprintf(stderr, "crisperwhisper: %s: blocks of one launch waited for each other in vain (GPU shared with other work?); "
                        "this context continues on the launch-per-stage decoder kernels (same results)\n", where);
    return CW_OK;
}
int32_t cw_handoff_fallbacks(cw_ctx* c) { return c->handoff_fallbacks; }
int32_t cw_align_prefill_runs(cw_ctx* c) { return c->align_prefill_runs; }
int32_t cw_score_prefill_runs(cw_ctx* c) { return c->score_prefill_runs; }
int32_t cw_handoff_resumes(cw_ctx* c) { return c->handoff_resumes; }

// The granule tag is (epoch << 6) | layer in 32 bits: 26 bits of the device's forward counter.  Granules are never cleared, so a
// stale one from exactly 2^26 forwards ago (rows a smaller batch did not rewrite) would pass for valid -- about a day of continuous
// decoding.  Entry points that run decoder forwards announce an upper bound here; long before the tag can repeat the granules are
// zeroed (tag 0 = epoch 0, never used) and the counter starts again at 1.  Called with the stream idle or about to be synchronised.
int epoch_hygiene(cw_ctx* c, long long upcoming_forwards) {
    c->forwards_since_reset += upcoming_forwards;
    if (c->forwards_since_reset < (1ll << 25)) return CW_OK;
    const int D = c->d.d_model;
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemset(c->d_gq, 0, (size_t)2 * 16 * D * 8)); HIPCHK(c, hipMemset(c->d_gps, 0, (size_t)(D / 16) * 16 * 2 * 8));
    HIPCHK(c, hipMemset(c->d_gq2, 0, (size_t)16 * D * 8)); HIPCHK(c, hipMemset(c->d_gkv, 0, (size_t)2 * 16 * (D / 2) * 8));
    HIPCHK(c, hipMemset(c->d_gflag, 0, (size_t)512 * 8));
    const unsigned int one = 1;
    HIPCHK(c, hipMemcpy(c->d_epoch, &one, 4, hipMemcpyHostToDevice));
    c->forwards_since_reset = upcoming_forwards;
    return CW_OK;
}

// ---- decoder prompt prefill: one multi-token forward over the n_prompt - 1 forward-only input positions of every row
// (prefill.hip).  Engages only for a decoder input that carries prompt_ids (cw_set_option "prompt_prefix" = their count, which
// cw_transcribe_prompted sets itself), on the 16-bit engines with the 16-bit cross cache and packed, LN-folded decoder weights;
// every other call keeps the per-position loop.  It writes the self-attention K/V cache rows 0 .. n_prompt-2 of every layer --
// the state the loop leaves; the prompt's logits and alignment rows are never read.
static bool prefill_capable(const cw_ctx* c) {
    return c->bf16 && c->d.d_model == 64 * c->d.n_heads && !c->kv8 && c->wpacked && c->ln_folded && c->layer_sel < 0;
}
static bool prefill_engages(const cw_ctx* c, int n_prompt) {
    return c->pf_prefix > 0 && n_prompt > c->pf_prefix && c->prompt_prefill && prefill_capable(c);
}

// Device buffers that grow on demand behind one capacity: when `want` exceeds it they are freed and allocated anew.  The slots are
// null and the capacity 0 until every allocation succeeded, so a failed regrow leaves what the next call and cw_destroy handle.
struct GrowBuf { void** slot; size_t bytes; };
static int regrow(cw_ctx* c, const char* label, size_t& cap, size_t want, std::initializer_list<GrowBuf> bufs) {
    if (want <= cap) return CW_OK;
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (const GrowBuf& b : bufs) if (*b.slot) { hipFree(*b.slot); *b.slot = nullptr; }
    cap = 0;
    for (const GrowBuf& b : bufs) {
        hipError_t e = hipMalloc(b.slot, b.bytes);
        if (e != hipSuccess) return fail(c, CW_ERR_NOMEM, "%s: hipMalloc(%zu) failed: %s", label, b.bytes, hipGetErrorString(e));
    }
    cap = want;
    return CW_OK;
}

static int prefill_reserve(cw_ctx* c, size_t M) {
    const size_t D = c->d.d_model, F = c->d.ffn_dim;
    return regrow(c, "prefill", c->pf_rows, M, {{(void**)&c->pf_x, M * D * 4}, {&c->pf_a, M * D * 2}, {&c->pf_q, M * D * 2},
                                                 {&c->pf_o, M * D * 2}, {&c->pf_h, M * F * 2}});
}

// What the scoring kernels write, from the context (kernels.h: ScoreHeadOut): the loop's [Bm][TGT] arrays (step) or the head's [M]
// arrays; stop: the STOP form (cw_align_cut_tokens); the TOPK form with cw_set_score_top_logprobs, the ENT form with cw_set_score_entropy
static ScoreHeadOut score_out(cw_ctx* c, bool stop, bool step) {
    ScoreHeadOut o{};
    o.logprob = step ? c->sc_step_lp : c->sc_lp; o.top_id = step ? c->sc_step_ti : c->sc_ti; o.top_logprob = step ? c->sc_step_tl : c->sc_tl;
    if (stop) { o.stop_logprob = step ? c->sc_step_stop : c->sc_stop; o.eos = c->gen.eos_token_id; o.ts_begin = c->gen.no_timestamps_token_id + 1; }
    o.k = c->sc_top_k; o.alt_id = step ? c->sc_step_alt_id : c->sc_alt_id; o.alt_logprob = step ? c->sc_step_alt_lp : c->sc_alt_lp;
    o.part = c->sc_part; o.spart = c->sc_spart; o.tpart = c->sc_tpart;
    if (c->sc_ent_on) { o.entropy = step ? c->sc_step_ent : c->sc_ent; o.epart = c->sc_epart; }
    return o;
}

// rows decoder rows (ids in d_ids [rows][TGT]), cross K/V row = row / kv_div.  Launches per layer: 3 LayerNorms, 6 GEMMs, 2
// attentions (the last layer: LayerNorm + q/k/v only -- its output feeds nothing the loop keeps).
// align (cw_align_tokens): the cross-attention of every layer that holds an alignment head records its rows for positions
// 0 .. n_prompt-2 into d_align / d_align_ml, and the forward stops after the cross-attention of the last such layer: that
// layer's cross out-projection and MLP, the layers above it, the final LayerNorm and the logits feed no alignment row.
static int align_last_layer(const cw_ctx* c) {
    int last = -1;
    for (int a = 0; a < c->d.n_align; ++a) last = c->align_layers[a] > last ? c->align_layers[a] : last;
    return last;
}
// full (cw_score_tokens): every layer runs to its end, the last one included, and leaves the residual stream of every position in
// pf_x for the scoring head; with align the alignment rows are recorded on the way, by the launches the early-stopping
// alignment forward makes.
static int run_prefill(cw_ctx* c, int rows, int n_prompt, int kv_div, bool align = false, bool full = false) {
    const int D = c->d.d_model, F = c->d.ffn_dim, H = c->d.n_heads, TGT = c->d.max_target_positions;
    const int n_pos = n_prompt - 1;
    const int M = rows * n_pos;
    CWCHK(c, prefill_reserve(c, (size_t)M));
    CWCHK(c, KD(c, cw_launch_prefill_embed, c->d_ids, TGT, n_pos, c->embed, c->dec_pos, c->pf_x, M, D, c->st));
    const int NL = (align && !full) ? align_last_layer(c) + 1 : c->d.dec_layers;
    for (int l = 0; l < NL; ++l) {
        LayerW& L = c->dec[l];
        PrefillEpi ep;
        memset(&ep, 0, sizeof(ep));
        CWCHK(c, KD(c, cw_launch_prefill_ln, c->pf_x, c->pf_a, M, D, c->st));
        ep.mode = PF_QKV; ep.bias = L.bqkv; ep.out = c->pf_q; ep.sk = L.sk; ep.sv = L.sv; ep.D = D; ep.H = H; ep.cap = TGT; ep.n_pos = n_pos;
        CWCHK(c, KD(c, cw_launch_prefill_gemm, c->pf_a, L.wqkv, ep, M, 3 * D, D, c->st));
        if (!align && !full && l + 1 == NL) break;
        CWCHK(c, KD(c, cw_launch_prefill_attn, c->pf_q, L.sk, L.sv, c->pf_o, rows, n_pos, H, TGT, n_pos, 1, 1, c->st));
        memset(&ep, 0, sizeof(ep));
        ep.mode = PF_RESID; ep.bias = L.bo; ep.x = c->pf_x;
        CWCHK(c, KD(c, cw_launch_prefill_gemm, c->pf_o, L.wo, ep, M, D, D, c->st));
        CWCHK(c, KD(c, cw_launch_prefill_ln, c->pf_x, c->pf_a, M, D, c->st));
        ep.mode = PF_STORE; ep.bias = L.bq_c; ep.out = c->pf_q; ep.x = nullptr;
        CWCHK(c, KD(c, cw_launch_prefill_gemm, c->pf_a, L.wq_c, ep, M, D, D, c->st));
        PrefillAlign al;
        memset(&al, 0, sizeof(al));
        if (align && std::find(c->align_layers.begin(), c->align_layers.end(), l) != c->align_layers.end()) {
            al.out = c->d_align; al.ml = c->d_align_ml; al.slot = c->d_align_slot + (size_t)l * H; al.n_align = c->d.n_align; al.rows = c->align_rows;
        }
        CWCHK(c, KD(c, cw_launch_prefill_attn_align, c->pf_q, L.ck, L.cv, c->pf_o, rows, n_pos, H, CW_N_CTX, CW_N_CTX, 0, kv_div, al, c->st));
        if (align && !full && l + 1 == NL) break;
        ep.mode = PF_RESID; ep.bias = L.bo_c; ep.out = nullptr; ep.x = c->pf_x;
        CWCHK(c, KD(c, cw_launch_prefill_gemm, c->pf_o, L.wo_c, ep, M, D, D, c->st));
        CWCHK(c, KD(c, cw_launch_prefill_ln, c->pf_x, c->pf_a, M, D, c->st));
        ep.mode = PF_GELU; ep.bias = L.b1; ep.out = c->pf_h; ep.x = nullptr;
        CWCHK(c, KD(c, cw_launch_prefill_gemm, c->pf_a, L.w1, ep, M, F, D, c->st));
        ep.mode = PF_RESID; ep.bias = L.b2; ep.out = nullptr; ep.x = c->pf_x;
        CWCHK(c, KD(c, cw_launch_prefill_gemm, c->pf_h, L.w2, ep, M, D, F, c->st));
    }
    return CW_OK;
}

static int decode_once(cw_ctx* c, int32_t nb, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                       int32_t min_new_tokens, const int32_t* forced, int32_t* sequences, int32_t* lengths,
                       int32_t* argmax_out, const int32_t* row_active);
int32_t cw_decode_rows(cw_ctx* c, int32_t nb, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                       int32_t min_new_tokens, const int32_t* forced, const int32_t* row_active, int32_t* sequences,
                       int32_t* lengths, int32_t* argmax_out) {
    int r = decode_once(c, nb, prompt, n_prompt, max_length, min_new_tokens, forced, sequences, lengths, argmax_out, row_active);
    if (r != CW_HANDOFF_RETRY) return r;
    CWCHK(c, handoffs_off(c, "decode"));
    r = decode_once(c, nb, prompt, n_prompt, max_length, min_new_tokens, forced, sequences, lengths, argmax_out, row_active);
    return r == CW_HANDOFF_RETRY ? fail(c, CW_ERR_HIP, "decode: an in-kernel wait timed out on the launch-per-stage path") : r;
}
int32_t cw_decode(cw_ctx* c, int32_t nb, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                  int32_t min_new_tokens, const int32_t* forced, int32_t* sequences, int32_t* lengths,
                  int32_t* argmax_out) {
    return cw_decode_rows(c, nb, prompt, n_prompt, max_length, min_new_tokens, forced, nullptr, sequences, lengths, argmax_out);
}

// row_active (cw_decode_rows): a row with row_active[b] == 0 starts finished (state 2 of d_finished: sample_kernel neither writes
// its ids nor adds to its log-probability sums), so what the previous decode left in d_ids / d_lp_sum / d_lp_cnt for it stays.
static int decode_once(cw_ctx* c, int32_t nb, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                       int32_t min_new_tokens, const int32_t* forced, int32_t* sequences, int32_t* lengths,
                       int32_t* argmax_out, const int32_t* row_active) {
    const int D = c->d.d_model, V = c->d.vocab_size, TGT = c->d.max_target_positions;
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (nb < 1 || nb > c->nb_encoded) return fail(c, CW_ERR_STATE, "nb=%d but %d windows encoded", nb, c->nb_encoded);
    if (n_prompt < 1 || n_prompt >= TGT) return fail(c, CW_ERR_INVALID, "n_prompt=%d out of range", n_prompt);
    if (max_length <= n_prompt || max_length > TGT) return fail(c, CW_ERR_INVALID, "max_length=%d out of range (n_prompt %d, max_target %d)", max_length, n_prompt, TGT);
    c->beam_K = 0;
    c->align_cur = c->d_align;
    CWCHK(c, epoch_hygiene(c, 2 * (long long)max_length + 4));   // (a resumed call runs some positions twice)
    std::vector<int> ids((size_t)nb * TGT, c->gen.pad_token_id);
    std::vector<int> fin0(nb, 0);
    int n_live = 0;
    if (row_active) {
        for (int b = 0; b < nb; ++b) { fin0[b] = row_active[b] ? 0 : 2; n_live += row_active[b] ? 1 : 0; }
        if (n_live == 0) return fail(c, CW_ERR_INVALID, "decode_rows: no active row");
        if (n_live < nb) {                     // masked rows keep the ids of the decode before
            HIPCHK(c, hipStreamSynchronize(c->st));
            HIPCHK(c, hipMemcpy(ids.data(), c->d_ids, ids.size() * 4, hipMemcpyDeviceToHost));
        }
    }
    for (int b = 0; b < nb; ++b) {
        if (fin0[b]) continue;
        for (int t = 0; t < TGT; ++t) ids[(size_t)b * TGT + t] = c->gen.pad_token_id;
        for (int t = 0; t < n_prompt; ++t) {
            int tok = prompt[(size_t)b * n_prompt + t];
            if (tok < 0 || tok >= V) return fail(c, CW_ERR_INVALID, "prompt token %d out of range", tok);
            ids[(size_t)b * TGT + t] = tok;
        }
    }
    HIPCHK(c, hipMemcpyAsync(c->d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->st));
    if (forced) HIPCHK(c, hipMemcpyAsync(c->d_forced, forced, (size_t)nb * TGT * 4, hipMemcpyHostToDevice, c->st));
    if (!row_active || n_live == nb) {
        HIPCHK(c, hipMemsetAsync(c->d_finished, 0, nb * 4, c->st));
        HIPCHK(c, hipMemsetAsync(c->d_lp_sum, 0, nb * 4, c->st));
        HIPCHK(c, hipMemsetAsync(c->d_lp_cnt, 0, nb * 4, c->st));
        if (c->tok_lp_on) HIPCHK(c, hipMemsetAsync(c->d_tok_lp, 0xff, (size_t)nb * TGT * 4, c->st));   // all-ones = NaN
        if (c->tok_ent_on) HIPCHK(c, hipMemsetAsync(c->d_tok_ent, 0xff, (size_t)nb * TGT * 4, c->st));
        if (c->top_k > 0) {                                                                             // ... and id -1
            HIPCHK(c, hipMemsetAsync(c->d_top_id, 0xff, (size_t)nb * TGT * CW_TOP_LOGPROBS_MAX * 4, c->st));
            HIPCHK(c, hipMemsetAsync(c->d_top_lp, 0xff, (size_t)nb * TGT * CW_TOP_LOGPROBS_MAX * 4, c->st));
        }
    } else {
        HIPCHK(c, hipMemcpyAsync(c->d_finished, fin0.data(), nb * 4, hipMemcpyHostToDevice, c->st));
        for (int b = 0; b < nb; ++b)
            if (!fin0[b]) {
                HIPCHK(c, hipMemsetAsync(c->d_lp_sum + b, 0, 4, c->st));
                HIPCHK(c, hipMemsetAsync(c->d_lp_cnt + b, 0, 4, c->st));
                if (c->tok_lp_on) HIPCHK(c, hipMemsetAsync(c->d_tok_lp + (size_t)b * TGT, 0xff, (size_t)TGT * 4, c->st));
                if (c->tok_ent_on) HIPCHK(c, hipMemsetAsync(c->d_tok_ent + (size_t)b * TGT, 0xff, (size_t)TGT * 4, c->st));
                if (c->top_k > 0) {
                    const size_t row = (size_t)TGT * CW_TOP_LOGPROBS_MAX;
                    HIPCHK(c, hipMemsetAsync(c->d_top_id + (size_t)b * row, 0xff, row * 4, c->st));
                    HIPCHK(c, hipMemsetAsync(c->d_top_lp + (size_t)b * row, 0xff, row * 4, c->st));
                }
            }
    }
    HIPCHK(c, hipMemsetAsync(c->d_last_ts, 0xff, nb * 4, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_argmax, 0xff, (size_t)nb * TGT * 4, c->st));
    const int cfg[4] = {n_prompt, min_new_tokens, max_length, forced ? 1 : 0};
    HIPCHK(c, hipMemcpyAsync(c->d_cfg, cfg, sizeof(cfg), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    StageTimer tm(c, CW_STAGE_DECODE);

    // prompt positions 0 .. n_prompt-2: forward only (their alignment rows are recorded, :254-256) -- one prefill when the input
    // carries prompt_ids
    if (prefill_engages(c, n_prompt)) CWCHK(c, run_prefill(c, nb, n_prompt, 1));
    else for (int pos = 0; pos + 1 < n_prompt; ++pos) {
        c->hist_short = pos + 1 <= 64;
        CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, pos, nb, c->st, c->d_epoch));
        CWCHK(c, KD(c, cw_launch_embed, c->d_ids, TGT, pos, c->embed, c->bf16 ? 1 : 0, c->dec_pos, c->dx, nb, D, c->st));
        CWCHK(c, decode_step(c, nb, false));
    }
    CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, n_prompt - 1, nb, c->st, c->d_epoch));
    CWCHK(c, KD(c, cw_launch_embed, c->d_ids, TGT, n_prompt - 1, c->embed, c->bf16 ? 1 : 0, c->dec_pos, c->dx, nb, D, c->st));
    int t = n_prompt, step = 0;
    // Host/device overlap: the "rows still running" counter of step s lands in its own pinned slot and is only
    // *read* after step s+1 has been queued (one step of lag, so the GPU never waits for the host; at most one
    // harmless extra step runs: it only writes cache / alignment rows beyond the ones that are used), and it
    // is not even copied while no row can finish yet (fewer than min_new_tokens generated: eos is masked).
    // The same 8-byte copy carries the hand-off failure word (d_err sits behind d_nunf): a wait that gave up (GPU shared
    // with other work) is seen one step later, and the call RESUMES at the position of the first failed forward on the
    // launch-per-stage kernels instead of running to the end on garbage and starting over.
    int first_copied = -1;
    for (;;) {
        int gave_up_word = 0;
        for (;;) {
            // forward at position t-1, logits, fused processors + argmax -> ids[t], x for position t, pos := t
            c->hist_short = t <= 64;               // keys 0 .. t-1
            CWCHK(c, run_step(c, nb));
            if (c->score_hook)   // cw_score_tokens' loop: log-softmax / target / arg-max of the raw logits that predict ids[t]; with score_stop
                                 // (cw_align_cut_tokens) stop_logprob too, with cw_set_score_top_logprobs the alternatives
                CWCHK(c, KD(c, cw_launch_score_rows, c->dlogits, c->Vpad, V, c->d_forced, TGT, t, nb, score_out(c, c->score_stop, true), c->st));
            if (c->logits_capture && step < c->logits_capture_steps)
                HIPCHK(c, hipMemcpy2DAsync(c->logits_capture + (size_t)step * nb * V, (size_t)V * 4, c->dlogits, (size_t)c->Vpad * 4, (size_t)V * 4, nb, hipMemcpyDeviceToHost, c->st));
            ++t;                               // sequence length is now t
            const bool can_finish = (t - n_prompt) >= min_new_tokens;
            if (can_finish) {
                if (first_copied < 0) first_copied = step;
                c->h_nunf[2 * step] = 1; c->h_nunf[2 * step + 1] = 0;
                HIPCHK(c, hipMemcpyAsync(c->h_nunf + 2 * step, c->d_nunf, 8, hipMemcpyDeviceToHost, c->st));
                HIPCHK(c, hipEventRecord(c->ev_step[step & 1], c->st));
            }
            ++step;
            if (t >= max_length) break;
            if (first_copied >= 0 && step - 2 >= first_copied) {   // counter of the step before the one just queued
                HIPCHK(c, hipEventSynchronize(c->ev_step[(step - 2) & 1]));
                if (c->h_nunf[2 * (step - 2) + 1] != 0) { gave_up_word = c->h_nunf[2 * (step - 2) + 1]; break; }
                if (c->h_nunf[2 * (step - 2)] == 0) break;
            }
        }
        HIPCHK(c, hipStreamSynchronize(c->st));
        {   // a block of a launch with an in-kernel wait gave up (GPU shared with other work)
            bool gave_up = false;
            int word = 0;
            CWCHK(c, handoff_gave_up(c, &gave_up, &word));
            if (gave_up) gave_up_word = word;
        }
        if (!gave_up_word) break;
        // word = 1 + decoder position P of the first forward that ran on a missed hand-off: ids[0 .. P], the cache rows and alignment
        // rows below P are good.  Resume there when the sampler's state can be rebuilt from the ids alone (no log-probability sums, no
        // logits capture, P inside the generated part); otherwise cw_decode repeats the whole call.
        const int P = gave_up_word - 1;
        if (P < n_prompt || P + 1 >= max_length || c->score_tokens || c->tok_lp_on || c->logits_capture || c->score_hook) { tm.stop(); return CW_HANDOFF_RETRY; }
        CWCHK(c, handoffs_off(c, "decode"));
        HIPCHK(c, hipMemcpy(ids.data(), c->d_ids, ids.size() * 4, hipMemcpyDeviceToHost));
        std::vector<int> fin(nb), lts(nb);
        const int tb = c->gen.no_timestamps_token_id + 1;
        for (int b = 0; b < nb; ++b) {                                  // sample_kernel's per-row state after it wrote ids[P]
            fin[b] = 0; lts[b] = -1;
            if (fin0[b]) { fin[b] = 2; continue; }
            for (int k = n_prompt; k <= P; ++k) {
                const int tok = ids[(size_t)b * TGT + k];
                if (!fin[b] && tok >= tb) lts[b] = tok;
                if (tok == c->gen.eos_token_id) fin[b] = 1;
            }
        }
        HIPCHK(c, hipMemcpy(c->d_finished, fin.data(), nb * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_last_ts, lts.data(), nb * 4, hipMemcpyHostToDevice));
        CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, P, nb, c->st, c->d_epoch));
        CWCHK(c, KD(c, cw_launch_embed, c->d_ids, TGT, P, c->embed, c->bf16 ? 1 : 0, c->dec_pos, c->dx, nb, D, c->st));
        t = P + 1; step = t - n_prompt; first_copied = -1;
        ++c->handoff_resumes;
    }
    if (first_copied >= 0)                 // true end = first step after which no row was running
        for (int s2 = first_copied; s2 < step; ++s2)
            if (c->h_nunf[2 * s2] == 0) { t = n_prompt + s2 + 1; break; }
    KCHK(c);
    tm.stop();
    HIPCHK(c, hipMemcpy(ids.data(), c->d_ids, ids.size() * 4, hipMemcpyDeviceToHost));
    memcpy(sequences, ids.data(), ids.size() * 4);
    // per-row length: up to and including the first eos among generated tokens, else t
    for (int b = 0; b < nb; ++b) {
        int len = t;
        for (int k = n_prompt; k < t; ++k)
            if (ids[(size_t)b * TGT + k] == c->gen.eos_token_id) { len = k + 1; break; }
        lengths[b] = fin0[b] ? 0 : len;            // a masked row did not run
    }
    if (argmax_out) HIPCHK(c, hipMemcpy(argmax_out, c->d_argmax, (size_t)nb * TGT * 4, hipMemcpyDeviceToHost));
    c->last_L = t - 1;   // attention rows retained: one per decoder input position
    c->align_unnormalized = c->bf16 && c->d.n_align > 0;
    c->last_nb = nb;
    return CW_OK;
}

// ---- deterministic half of generate_with_fallback (generation_whisper.py:970-1116, 1243-1287)
int32_t cw_set_thresholds(cw_ctx* c, float logprob_threshold, float no_speech_threshold) {
    if (!isnan(no_speech_threshold) && isnan(logprob_threshold))
        return fail(c, CW_ERR_INVALID, "no_speech_threshold needs logprob_threshold (generation_whisper.py:1275-1285 compares both)");
    c->logprob_thr = logprob_threshold; c->no_speech_thr = no_speech_threshold;
    const bool want = !isnan(logprob_threshold);
    if (want != c->score_tokens) { c->score_tokens = want; drop_step_graphs(c); }
    return CW_OK;
}

// ---- per-token log-probabilities of the free-running decode (include/crisperwhisper.h) -------------------------------------
int32_t cw_set_token_logprobs(cw_ctx* c, int32_t on) {
    const bool want = on != 0;
    if (!want && c->top_k > 0) CWCHK(c, cw_set_top_logprobs(c, 0));   // the alternatives share this switch's normaliser
    if (!want && c->tok_ent_on) CWCHK(c, cw_set_token_entropy(c, 0)); // ... and so does the entropy
    const size_t n = (size_t)c->Bm * c->d.max_target_positions;
    if (want && !c->d_tok_lp) {
        CWCHK(c, dmalloc(c, &c->d_tok_lp, n * 4, false));
        HIPCHK(c, hipMemset(c->d_tok_lp, 0xff, n * 4));
    }
    if (want != c->tok_lp_on) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (want) HIPCHK(c, hipMemset(c->d_tok_lp, 0xff, n * 4));   // nothing decoded under this switch yet
        c->tok_lp_on = want;
        c->tr_lp.clear();
        drop_step_graphs(c);
    }
    return CW_OK;
}
int32_t cw_get_token_logprobs(cw_ctx* c, float* out, int32_t nb) {
    if (!c->tok_lp_on) return fail(c, CW_ERR_STATE, "token log-probabilities are off (cw_set_token_logprobs)");
    if (!out || nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "get_token_logprobs: nb=%d outside 1 .. %d", nb, c->Bm);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(out, c->d_tok_lp, (size_t)nb * c->d.max_target_positions * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}
int32_t cw_get_transcribe_token_logprobs(cw_ctx* c, float* out, int32_t B, int32_t cap) {
    if (!c->tok_lp_on) return fail(c, CW_ERR_STATE, "token log-probabilities are off (cw_set_token_logprobs)");
    if (!out || B < 1 || (size_t)B != c->tr_lp.size()) return fail(c, CW_ERR_STATE, "get_transcribe_token_logprobs: B=%d but the last cw_transcribe had %d items", B, (int)c->tr_lp.size());
    for (int i = 0; i < B; ++i) {
        const int n = (int)c->tr_lp[i].size();
        if (n > cap) return fail(c, CW_ERR_INVALID, "item %d holds %d tokens, capacity %d", i, n, cap);
        memcpy(out + (size_t)i * cap, c->tr_lp[i].data(), (size_t)n * 4);
        for (int k = n; k < cap; ++k) out[(size_t)i * cap + k] = NAN;
    }
    return CW_OK;
}

// ---- token entropy: predictive entropy of every step's raw distribution (include/crisperwhisper.h) -------------------------
int32_t cw_set_token_entropy(cw_ctx* c, int32_t on) {
    const bool want = on != 0;
    if (want && !c->tok_lp_on) return fail(c, CW_ERR_STATE, "token entropy needs token log-probabilities (cw_set_token_logprobs)");
    const size_t n = (size_t)c->Bm * c->d.max_target_positions;
    if (want && !c->d_ent_part) CWCHK(c, dmalloc(c, &c->d_ent_part, (size_t)c->Bm * 16 * 4));
    if (want && !c->d_tok_ent) CWCHK(c, dmalloc(c, &c->d_tok_ent, n * 4, false));
    if (want != c->tok_ent_on) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (want) HIPCHK(c, hipMemset(c->d_tok_ent, 0xff, n * 4));   // nothing decoded under this switch yet
        c->tok_ent_on = want;
        c->tr_ent.clear();
        drop_step_graphs(c);
    }
    return CW_OK;
}
int32_t cw_get_token_entropy(cw_ctx* c, float* out, int32_t nb) {
    if (!c->tok_ent_on) return fail(c, CW_ERR_STATE, "token entropy is off (cw_set_token_entropy)");
    if (!out || nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "get_token_entropy: nb=%d outside 1 .. %d", nb, c->Bm);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(out, c->d_tok_ent, (size_t)nb * c->d.max_target_positions * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}
int32_t cw_get_transcribe_token_entropy(cw_ctx* c, float* out, int32_t B, int32_t cap) {
    if (!c->tok_ent_on) return fail(c, CW_ERR_STATE, "token entropy is off (cw_set_token_entropy)");
    if (!out || B < 1 || (size_t)B != c->tr_ent.size()) return fail(c, CW_ERR_STATE, "get_transcribe_token_entropy: B=%d but the last cw_transcribe had %d items", B, (int)c->tr_ent.size());
    for (int i = 0; i < B; ++i) {
        const int n = (int)c->tr_ent[i].size();
        if (n > cap) return fail(c, CW_ERR_INVALID, "item %d holds %d tokens, capacity %d", i, n, cap);
        memcpy(out + (size_t)i * cap, c->tr_ent[i].data(), (size_t)n * 4);
        for (int k = n; k < cap; ++k) out[(size_t)i * cap + k] = NAN;
    }
    return CW_OK;
}

// ---- top_logprobs: the k best raw logits of every step of the free-running decode (include/crisperwhisper.h) ---------------
int32_t cw_set_top_logprobs(cw_ctx* c, int32_t k) {
    if (k < 0 || k > CW_TOP_LOGPROBS_MAX) return fail(c, CW_ERR_INVALID, "set_top_logprobs: k=%d outside 0 .. %d", k, CW_TOP_LOGPROBS_MAX);
    if (k > 0 && !c->tok_lp_on) return fail(c, CW_ERR_STATE, "top_logprobs needs token log-probabilities (cw_set_token_logprobs)");
    const size_t n = (size_t)c->Bm * c->d.max_target_positions * CW_TOP_LOGPROBS_MAX;
    if (k > 0 && !c->d_top_id) {
        CWCHK(c, dmalloc(c, &c->d_top_part, (size_t)c->Bm * 16 * CW_TOP_LOGPROBS_MAX * 8));
        CWCHK(c, dmalloc(c, &c->d_top_lp, n * 4, false));
        CWCHK(c, dmalloc(c, &c->d_top_id, n * 4, false));
    }
    if (k != c->top_k) {
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (k > 0) {                                                  // nothing decoded under this value yet
            HIPCHK(c, hipMemset(c->d_top_id, 0xff, n * 4));          // all-ones: id -1, value NaN
            HIPCHK(c, hipMemset(c->d_top_lp, 0xff, n * 4));
        }
        c->top_k = k;
        c->tr_top_id.clear(); c->tr_top_lp.clear();
        drop_step_graphs(c);
    }
    return CW_OK;
}
int32_t cw_get_top_logprobs(cw_ctx* c, int32_t* ids_out, float* lp_out, int32_t nb) {
    if (c->top_k < 1) return fail(c, CW_ERR_STATE, "top_logprobs is off (cw_set_top_logprobs)");
    if (!ids_out || !lp_out || nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "get_top_logprobs: nb=%d outside 1 .. %d", nb, c->Bm);
    const size_t n = (size_t)nb * c->d.max_target_positions, k = (size_t)c->top_k;
    std::vector<int> hi(n * CW_TOP_LOGPROBS_MAX); std::vector<float> hl(n * CW_TOP_LOGPROBS_MAX);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(hi.data(), c->d_top_id, hi.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hl.data(), c->d_top_lp, hl.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {                                  // device rows are CW_TOP_LOGPROBS_MAX wide, the caller's k
        memcpy(ids_out + i * k, &hi[i * CW_TOP_LOGPROBS_MAX], k * 4);
        memcpy(lp_out + i * k, &hl[i * CW_TOP_LOGPROBS_MAX], k * 4);
    }
    return CW_OK;
}
int32_t cw_get_transcribe_top_logprobs(cw_ctx* c, int32_t* ids_out, float* lp_out, int32_t B, int32_t cap) {
    if (c->top_k < 1) return fail(c, CW_ERR_STATE, "top_logprobs is off (cw_set_top_logprobs)");
    if (!ids_out || !lp_out || B < 1 || (size_t)B != c->tr_top_id.size())
        return fail(c, CW_ERR_STATE, "get_transcribe_top_logprobs: B=%d but the last cw_transcribe had %d items", B, (int)c->tr_top_id.size());
    const size_t k = (size_t)c->top_k;
    for (int i = 0; i < B; ++i) {
        const size_t n = c->tr_top_id[i].size() / k;
        if (n > (size_t)cap) return fail(c, CW_ERR_INVALID, "item %d holds %d tokens, capacity %d", i, (int)n, cap);
        memcpy(ids_out + (size_t)i * cap * k, c->tr_top_id[i].data(), n * k * 4);
        memcpy(lp_out + (size_t)i * cap * k, c->tr_top_lp[i].data(), n * k * 4);
        for (size_t j = n * k; j < (size_t)cap * k; ++j) { ids_out[(size_t)i * cap * k + j] = -1; lp_out[(size_t)i * cap * k + j] = NAN; }
    }
    return CW_OK;
}

// ---- alignment scores: attention mass on the DTW path and attention spread per token (include/crisperwhisper.h) ------------
int32_t cw_set_alignment_scores(cw_ctx* c, int32_t on, int32_t collar_frames) {
    if (collar_frames < 0) return fail(c, CW_ERR_INVALID, "set_alignment_scores: collar_frames=%d is negative", collar_frames);
    const bool want = on != 0;
    // switching off, or repeating the setting in force, changes nothing and is always accepted: a caller that sets the switch
    // before every decode must not trip over a search that an interrupted caller left open (the next decode closes it)
    if (!want && !c->as_on) return CW_OK;
    if (want && c->as_on && collar_frames == c->as_collar) return CW_OK;
    if (want && c->beam_K > 0) return fail(c, CW_ERR_STATE, "set_alignment_scores: a beam search is open");
    if (want && !c->d_as_mass) {
        const size_t n = (size_t)c->Bm * c->d.max_target_positions;
        CWCHK(c, dmalloc(c, &c->d_as_mass, n * 4, false));
        CWCHK(c, dmalloc(c, &c->d_as_spread, n * 4, false));
    }
    if (want != c->as_on || (want && collar_frames != c->as_collar)) {   // nothing aligned under this setting yet
        c->as_mass.clear(); c->as_spread.clear();
        c->tr_as_mass.clear(); c->tr_as_spread.clear();
    }
    c->as_on = want;
    if (want) c->as_collar = collar_frames;
    return CW_OK;
}
int32_t cw_get_alignment_scores(cw_ctx* c, float* mass, float* spread, int32_t nb, int32_t L) {
    if (!c->as_on) return fail(c, CW_ERR_STATE, "alignment scores are off (cw_set_alignment_scores)");
    if (!mass || !spread) return fail(c, CW_ERR_INVALID, "get_alignment_scores: null argument");
    if (nb < 1 || (size_t)nb > c->as_mass.size() || L < 0)
        return fail(c, CW_ERR_STATE, "get_alignment_scores: asked %d x %d, the last timestamp stage scored %d rows", nb, L, (int)c->as_mass.size());
    for (int b = 0; b < nb; ++b) {
        const size_t n = c->as_mass[b].size();
        if (n > (size_t)L + 1) return fail(c, CW_ERR_STATE, "get_alignment_scores: row %d holds %d positions, asked L=%d", b, (int)n - 1, L);
        memcpy(mass + (size_t)b * (L + 1), c->as_mass[b].data(), n * 4);
        memcpy(spread + (size_t)b * (L + 1), c->as_spread[b].data(), n * 4);
        for (size_t k = n; k <= (size_t)L; ++k) { mass[(size_t)b * (L + 1) + k] = NAN; spread[(size_t)b * (L + 1) + k] = NAN; }
    }
    return CW_OK;
}
int32_t cw_get_transcribe_alignment_scores(cw_ctx* c, float* mass, float* spread, int32_t B, int32_t cap) {
    if (!c->as_on) return fail(c, CW_ERR_STATE, "alignment scores are off (cw_set_alignment_scores)");
    if (!mass || !spread || B < 1 || (size_t)B != c->tr_as_mass.size())
        return fail(c, CW_ERR_STATE, "get_transcribe_alignment_scores: B=%d but the last cw_transcribe had %d items", B, (int)c->tr_as_mass.size());
    for (int i = 0; i < B; ++i) {
        const int n = (int)c->tr_as_mass[i].size();
        if (n > cap) return fail(c, CW_ERR_INVALID, "item %d holds %d tokens, capacity %d", i, n, cap);
        memcpy(mass + (size_t)i * cap, c->tr_as_mass[i].data(), (size_t)n * 4);
        memcpy(spread + (size_t)i * cap, c->tr_as_spread[i].data(), (size_t)n * 4);
        for (int k = n; k < cap; ++k) { mass[(size_t)i * cap + k] = NAN; spread[(size_t)i * cap + k] = NAN; }
    }
    return CW_OK;
}

// ---- sequence_bias: phrase boosting inside the sampler kernels (include/crisperwhisper.h) ------------------------------------
// Checks the caller's table and lays it out as the kernels read it (kernels.h): entries ordered by last token, for one last token
// the length-1 entry first and the longer ones in the caller's order, plus the entry range of each of the 16 vocabulary slices of
// the sampler's stage 1.  Touches no state.
int seq_bias_table(cw_ctx* c, int n_seq, const int32_t* tokens, const int32_t* lengths, const float* bias, std::vector<int>* out,
                          const char* who) {
    out->assign(SB_WORDS, 0);
    if (n_seq < 0 || n_seq > SB_MAX_SEQ) return fail(c, CW_ERR_INVALID, "%s: %d sequences outside 0 .. %d", who, n_seq, SB_MAX_SEQ);
    if (n_seq == 0) return CW_OK;
    if (!tokens || !lengths || !bias) return fail(c, CW_ERR_INVALID, "%s: null argument", who);
    const int V = c->d.vocab_size;
    std::vector<int> start(n_seq), order(n_seq);
    int total = 0;
    for (int i = 0; i < n_seq; ++i) {
        if (lengths[i] < 1 || lengths[i] > SB_MAX_LEN) return fail(c, CW_ERR_INVALID, "%s: sequence %d has %d tokens, outside 1 .. %d", who, i, lengths[i], SB_MAX_LEN);
        if (!std::isfinite(bias[i])) return fail(c, CW_ERR_INVALID, "%s: the bias of sequence %d is not finite", who, i);
        start[i] = total; total += lengths[i]; order[i] = i;
    }
    for (int k = 0; k < total; ++k)
        if (tokens[k] < 0 || tokens[k] >= V) return fail(c, CW_ERR_INVALID, "%s: token %d outside 0 .. %d", who, tokens[k], V - 1);
    for (int i = 0; i < n_seq; ++i)
        for (int j = 0; j < i; ++j)
            if (lengths[i] == lengths[j] && !memcmp(tokens + start[i], tokens + start[j], (size_t)lengths[i] * 4))
                return fail(c, CW_ERR_INVALID, "%s: sequences %d and %d are the same", who, j, i);
    auto last = [&](int i) { return tokens[start[i] + lengths[i] - 1]; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (last(a) != last(b)) return last(a) < last(b);
        return (lengths[a] == 1) > (lengths[b] == 1);
    });
    int* w = out->data();
    const int per4 = ((c->Vpad >> 2) + 15) / 16;                 // float4 groups per slice, as sample_partial_kernel cuts them
    int off = 0;
    for (int e = 0; e < n_seq; ++e) w[SB_SLICE + std::min(15, (last(order[e]) >> 2) / per4) + 1] += 1;
    for (int s = 0; s < 16; ++s) w[SB_SLICE + s + 1] += w[SB_SLICE + s];     // [s]: entries whose last token lies in a slice below s
    for (int e = 0; e < n_seq; ++e) {
        const int i = order[e];
        w[SB_OFF + e] = off;
        memcpy(&w[SB_VAL + e], &bias[i], 4);
        w[SB_LAST + e] = last(i);
        memcpy(&w[SB_TOK + off], tokens + start[i], (size_t)lengths[i] * 4);
        off += lengths[i];
    }
    w[SB_OFF + n_seq] = off;
    return CW_OK;
}
// installs a table laid out by seq_bias_table; only the off <-> on transition changes which kernels the step graphs hold
int seq_bias_install(cw_ctx* c, const std::vector<int>& tab, int n_seq) {
    if (n_seq > 0 && !c->d_seq_bias) CWCHK(c, dmalloc(c, &c->d_seq_bias, (size_t)SB_WORDS * 4));
    HIPCHK(c, hipStreamSynchronize(c->st));                    // no step in flight reads the old contents
    if (n_seq > 0) HIPCHK(c, hipMemcpy(c->d_seq_bias, tab.data(), (size_t)SB_WORDS * 4, hipMemcpyHostToDevice));
    if ((n_seq > 0) != (c->sb_n > 0)) drop_step_graphs(c);
    c->sb_n = n_seq;
    c->sb_host = tab;
    return CW_OK;
}
int32_t cw_set_sequence_bias(cw_ctx* c, int32_t n_seq, const int32_t* tokens, const int32_t* lengths, const float* bias) {
    std::vector<int> tab;
    CWCHK(c, seq_bias_table(c, n_seq, tokens, lengths, bias, &tab, "set_sequence_bias"));
    if (c->beam_K > 0) return fail(c, CW_ERR_STATE, "set_sequence_bias: a beam search is open");
    return seq_bias_install(c, tab, n_seq);
}

// ---- stochastic half: seeded Gumbel-max sampling in the sampler kernels (include/crisperwhisper.h) ----------------------
// The kernels read temperature, seed and stream ids from d_samp, so the captured step graphs stay as they are.
int write_sampling(cw_ctx* c, float temperature, uint64_t seed, const uint64_t* row_streams, int nb, const char* who) {
    if (!(temperature >= 0.f) || std::isinf(temperature)) return fail(c, CW_ERR_INVALID, "%s: temperature must be finite and >= 0", who);
    std::vector<unsigned int> w(c->samp_host.size(), 0u);
    if (temperature > 0.f && row_streams) {
        if (nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "%s: nb=%d outside 1 .. %d", who, nb, c->Bm);
        memcpy(&w[0], &temperature, 4);
        w[1] = (unsigned int)(seed & 0xffffffffu); w[2] = (unsigned int)(seed >> 32);
        for (int b = 0; b < nb; ++b) { w[4 + 2 * b] = (unsigned int)(row_streams[b] & 0xffffffffu); w[5 + 2 * b] = (unsigned int)(row_streams[b] >> 32); }
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(c->d_samp, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    c->samp_host = w;
    return CW_OK;
}
int32_t cw_set_sampling(cw_ctx* c, float temperature, uint64_t seed, const uint64_t* row_streams, int32_t nb) {
    return write_sampling(c, temperature, seed, row_streams, nb, "set_sampling");
}

// average log_softmax(processed scores)[token] over the generated tokens of every row of the last cw_decode, the eos
// included (generation_whisper.py:1958-1974); rows that generated nothing report 0
int32_t cw_get_avg_logprobs(cw_ctx* c, float* out, int32_t nb) {
    if (!c->score_tokens) return fail(c, CW_ERR_STATE, "token scores are only tracked while a logprob threshold is set (cw_set_thresholds)");
    if (nb < 1 || nb > c->last_nb) return fail(c, CW_ERR_INVALID, "nb=%d but the last decode had %d rows", nb, c->last_nb);
    std::vector<float> s(nb); std::vector<int> n(nb);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(s.data(), c->d_lp_sum, nb * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(n.data(), c->d_lp_cnt, nb * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < nb; ++b) out[b] = n[b] > 0 ? s[b] / (float)n[b] : 0.f;
    return CW_OK;
}

// WhisperNoSpeechDetection (logits_process.py:2050-2112): softmax of the raw decoder logits at the <|startoftranscript|>
// position of every encoded window, at token no_timestamps_token_id - 1 (generation_whisper.py:1801-1806).  One decoder
// forward at position 0; call it before cw_decode (which decodes position 0 again).
// The forward shared by cw_no_speech_probs and cw_detect_language: <|startoftranscript|> at position 0 of the nb encoded windows,
// logits left in c->dlogits; a lost in-launch hand-off repeats it once on the launch-per-stage kernels.  short_hist: what
// c->hist_short holds during the forward -- false as cw_no_speech_probs has always run it, true as cw_decode runs its position 0
// (one key: the short-history attention at 9 rows and more), which is what language detection has to reproduce bit for bit.
static int forward_sot(cw_ctx* c, int nb, int sot_token, bool short_hist, const char* who) {
    const int D = c->d.d_model, TGT = c->d.max_target_positions;
    CWCHK(c, epoch_hygiene(c, 4));
    c->beam_K = 0;
    c->align_cur = c->d_align;
    std::vector<int> ids((size_t)nb * TGT, c->gen.pad_token_id);
    for (int b = 0; b < nb; ++b) ids[(size_t)b * TGT] = sot_token;
    HIPCHK(c, hipMemcpyAsync(c->d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (int attempt = 0;; ++attempt) {
        CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, 0, nb, c->st, c->d_epoch));
        CWCHK(c, KD(c, cw_launch_embed, c->d_ids, TGT, 0, c->embed, c->bf16 ? 1 : 0, c->dec_pos, c->dx, nb, D, c->st));
        c->hist_short = short_hist;
        CWCHK(c, decode_step(c, nb, true));
        KCHK(c);
        bool gave_up = false;
        CWCHK(c, handoff_gave_up(c, &gave_up));
        if (!gave_up) break;
        if (attempt) return fail(c, CW_ERR_HIP, "%s: an in-kernel wait timed out on the launch-per-stage path", who);
        CWCHK(c, handoffs_off(c, who));
    }
    return CW_OK;
}

int32_t cw_no_speech_probs(cw_ctx* c, int32_t nb, int32_t sot_token, float* out) {
    const int V = c->d.vocab_size;
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (nb < 1 || nb > c->nb_encoded) return fail(c, CW_ERR_STATE, "nb=%d but %d windows encoded", nb, c->nb_encoded);
    const int tok = c->gen.no_timestamps_token_id - 1;
    if (sot_token < 0 || sot_token >= V || tok < 0) return fail(c, CW_ERR_INVALID, "no_speech_probs: token out of range");
    CWCHK(c, forward_sot(c, nb, sot_token, false, "no_speech_probs"));
    std::vector<float> lg((size_t)nb * V);
    CWCHK(c, cw_get_logits(c, lg.data(), nb));
    for (int b = 0; b < nb; ++b) {
        const float* r = lg.data() + (size_t)b * V;
        float m = r[0];
        for (int v = 1; v < V; ++v) m = r[v] > m ? r[v] : m;
        double z = 0.0;
        for (int v = 0; v < V; ++v) z += exp((double)(r[v] - m));
        out[b] = (float)(exp((double)(r[tok] - m)) / z);
    }
    return CW_OK;
}

// ---- language identification (include/crisperwhisper.h: cw_detect_language; kernel in langid.hip) ---------------------------
int check_lang_ids(cw_ctx* c, const char* who, const int32_t* lang_ids, int n_lang) {
    if (!lang_ids) return fail(c, CW_ERR_INVALID, "%s: lang_ids is null", who);
    if (n_lang < 1 || n_lang > CW_LANG_IDS_MAX) return fail(c, CW_ERR_INVALID, "%s: n_lang=%d outside 1 .. %d", who, n_lang, CW_LANG_IDS_MAX);
    for (int k = 0; k < n_lang; ++k) {
        if (lang_ids[k] < 0 || lang_ids[k] >= c->d.vocab_size)
            return fail(c, CW_ERR_INVALID, "%s: language id %d at %d is outside the vocabulary (%d)", who, lang_ids[k], k, c->d.vocab_size);
        for (int j = 0; j < k; ++j)
            if (lang_ids[j] == lang_ids[k]) return fail(c, CW_ERR_INVALID, "%s: language id %d is listed twice", who, lang_ids[k]);
    }
    return CW_OK;
}
// the kernel over rows 0 .. nb-1 of c->dlogits and the one copy of its records; ns_tok < 0: no no-speech part
int language_probs(cw_ctx* c, int nb, const int32_t* lang_ids, int n_lang, int ns_tok, int32_t* best, float* prob,
                          float* no_speech) {
    if (!c->d_lang_ids) {
        CWCHK(c, dmalloc(c, &c->d_lang_ids, (size_t)CW_LANG_IDS_MAX * 4));
        CWCHK(c, dmalloc(c, &c->d_lang_out, (size_t)c->Bm * (CW_LANG_IDS_MAX + 2) * 4));
    }
    const int rec = n_lang + 2;
    HIPCHK(c, hipMemcpyAsync(c->d_lang_ids, lang_ids, (size_t)n_lang * 4, hipMemcpyHostToDevice, c->st));
    const int r = cw_launch_language_probs(c->dlogits, c->Vpad, c->d.vocab_size, c->d_lang_ids, n_lang, ns_tok, nb, c->d_lang_out, c->st);
    if (r != CW_OK) return fail(c, r, "language_probs: launch rejected");
    KCHK(c);
    std::vector<float> h((size_t)nb * rec);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(h.data(), c->d_lang_out, h.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < nb; ++b) {
        const float* p = h.data() + (size_t)b * rec;
        memcpy(&best[b], p, 4);
        if (no_speech) no_speech[b] = p[1];
        if (prob) memcpy(prob + (size_t)b * n_lang, p + 2, (size_t)n_lang * 4);
    }
    return CW_OK;
}

int32_t cw_detect_language(cw_ctx* c, int32_t nb, int32_t sot_token, const int32_t* lang_ids, int32_t n_lang, int32_t* best,
                           float* prob, float* no_speech) {
    if (!best) return fail(c, CW_ERR_INVALID, "detect_language: best is null");
    CWCHK(c, check_lang_ids(c, "detect_language", lang_ids, n_lang));
    if (sot_token < 0 || sot_token >= c->d.vocab_size) return fail(c, CW_ERR_INVALID, "detect_language: sot_token %d out of range", sot_token);
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (nb < 1 || nb > c->nb_encoded) return fail(c, CW_ERR_STATE, "nb=%d but %d windows encoded", nb, c->nb_encoded);
    const int ns_tok = no_speech ? c->gen.no_timestamps_token_id - 1 : -1;
    if (no_speech && (ns_tok < 0 || ns_tok >= c->d.vocab_size)) return fail(c, CW_ERR_INVALID, "detect_language: no-speech token out of range");
    CWCHK(c, forward_sot(c, nb, sot_token, true, "detect_language"));
    return language_probs(c, nb, lang_ids, n_lang, ns_tok, best, prob, no_speech);
}

int32_t cw_get_transcribe_languages(cw_ctx* c, int32_t* lang_token, float* prob, int32_t B) {
    if (!lang_token || B < 1 || (size_t)B != c->tr_lang.size())
        return fail(c, CW_ERR_STATE, "get_transcribe_languages: B=%d but the last cw_transcribe had %d items", B, (int)c->tr_lang.size());
    for (int i = 0; i < B; ++i) {
        lang_token[i] = c->tr_lang[i];
        if (prob) prob[i] = c->tr_lang_prob[i];
    }
    return CW_OK;
}

int32_t cw_get_logits(cw_ctx* c, float* out, int32_t nb) {
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy2D(out, (size_t)c->d.vocab_size * 4, c->dlogits, (size_t)c->Vpad * 4, (size_t)c->d.vocab_size * 4, nb, hipMemcpyDeviceToHost));
    return CW_OK;
}

int32_t cw_set_logits_capture(cw_ctx* c, float* host_buf, int32_t max_steps) {
    c->logits_capture = host_buf;
    c->logits_capture_steps = host_buf ? max_steps : 0;
    return CW_OK;
}

static int normalize_alignment(cw_ctx* c) {
    if (!c->align_unnormalized) return CW_OK;
    CWCHK(c, KD(c, cw_launch_align_normalize, c->d_align, c->d_align_ml, c->last_nb, c->d.n_align, c->align_rows,
                                       c->last_L, CW_N_CTX, c->st));
    c->align_unnormalized = false;
    return CW_OK;
}

int32_t cw_get_alignment(cw_ctx* c, float* out, int32_t nb, int32_t L) {
    const int Ha = c->d.n_align, TGT = c->d.max_target_positions;
    if (Ha <= 0) return fail(c, CW_ERR_STATE, "no alignment heads configured");
    if (nb > c->last_nb || L > c->last_L) return fail(c, CW_ERR_STATE, "only %d x %d rows retained", c->last_nb, c->last_L);
    CWCHK(c, normalize_alignment(c));
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (int b = 0; b < nb; ++b)
        for (int a = 0; a < Ha; ++a)
            HIPCHK(c, hipMemcpy(out + (((size_t)b * Ha + a) * L) * CW_N_CTX,
                                c->align_cur + (((size_t)b * Ha + a) * TGT) * CW_N_CTX, (size_t)L * CW_N_CTX * 4,
                                hipMemcpyDeviceToHost));
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// beam search: device half of GenerationMixin._beam_search (TF/generation/utils.py:3208-3520).  The host side of the
// ABI (crisperwhisper_amd/generation.py) keeps the hypothesis bookkeeping -- running / finished beams, length penalty,
// early-stopping heuristic -- exactly as HF does; the device runs the decoder on items x beams rows, reduces every row
// to its best candidates and re-orders the per-row state by rewriting an ancestry table instead of copying KV caches.
// ------------------------------------------------------------------------------------------------
int beam_alloc(cw_ctx* c) {
    if (c->d_anc) return CW_OK;
    const int TGT = c->d.max_target_positions, Bm = c->Bm;
    CWCHK(c, dmalloc(c, &c->d_anc, (size_t)Bm * TGT * 4)); CWCHK(c, dmalloc(c, &c->d_anc_tmp, (size_t)Bm * TGT * 4));
    CWCHK(c, dmalloc(c, &c->d_ids_tmp, (size_t)Bm * TGT * 4));
    CWCHK(c, dmalloc(c, &c->d_parent, Bm * 4)); CWCHK(c, dmalloc(c, &c->d_tok, Bm * 4));
    CWCHK(c, dmalloc(c, &c->d_cand_val, (size_t)Bm * 64 * 4)); CWCHK(c, dmalloc(c, &c->d_cand_id, (size_t)Bm * 64 * 4));
    CWCHK(c, dmalloc(c, &c->d_rowmap, (size_t)Bm * TGT * 4));
    CWCHK(c, dmalloc(c, &c->d_topk_scratch, KD(c, cw_beam_topk_scratch_floats, Bm) * 4));
    return CW_OK;
}

int32_t cw_beam_begin(cw_ctx* c, int32_t n_items, int32_t num_beams, const int32_t* prompt, int32_t n_prompt,
                      int32_t max_length, int32_t min_new_tokens) {
    const int D = c->d.d_model, V = c->d.vocab_size, TGT = c->d.max_target_positions;
    if (c->sb_n > 0) return fail(c, CW_ERR_STATE, "beam search does not carry sequence_bias (it would be added to log_softmax(raw)): clear the table (cw_set_sequence_bias with n_seq = 0) first");
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (num_beams < 1 || n_items < 1 || n_items > c->nb_encoded) return fail(c, CW_ERR_STATE, "beam_begin: %d items but %d windows encoded", n_items, c->nb_encoded);
    const int rows = n_items * num_beams;
    if (rows > c->Bm) return fail(c, CW_ERR_INVALID, "beam search needs max_batch >= items x beams = %d (context has %d)", rows, c->Bm);
    if (n_prompt < 1 || n_prompt >= TGT || max_length <= n_prompt || max_length > TGT) return fail(c, CW_ERR_INVALID, "beam_begin: n_prompt=%d max_length=%d out of range", n_prompt, max_length);
    CWCHK(c, beam_alloc(c));
    CWCHK(c, epoch_hygiene(c, 2 * (long long)max_length + 4));
    std::vector<int> ids((size_t)rows * TGT, c->gen.pad_token_id), anc((size_t)rows * TGT);
    for (int r = 0; r < rows; ++r) {
        for (int t = 0; t < n_prompt; ++t) {
            const int tok = prompt[(size_t)(r / num_beams) * n_prompt + t];
            if (tok < 0 || tok >= V) return fail(c, CW_ERR_INVALID, "prompt token %d out of range", tok);
            ids[(size_t)r * TGT + t] = tok;
        }
        for (int t = 0; t < TGT; ++t) anc[(size_t)r * TGT + t] = r;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->d_anc, anc.data(), anc.size() * 4, hipMemcpyHostToDevice, c->st));
    const int cfg[4] = {n_prompt, min_new_tokens, max_length, 0};
    HIPCHK(c, hipMemcpyAsync(c->d_cfg, cfg, sizeof(cfg), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    c->beam_K = num_beams; c->beam_items = n_items; c->beam_n_prompt = n_prompt;
    c->beam_pos = n_prompt - 1; c->beam_max_len = max_length;
    c->align_cur = c->d_align;
    if (prefill_engages(c, n_prompt)) CWCHK(c, run_prefill(c, rows, n_prompt, num_beams));
    else for (int pos = 0; pos + 1 < n_prompt; ++pos) {     // prompt positions: forward only
        CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, pos, rows, c->st));
        CWCHK(c, KD(c, cw_launch_embed, c->d_ids, TGT, pos, c->embed, c->bf16 ? 1 : 0, c->dec_pos, c->dx, rows, D, c->st));
        c->hist_short = pos + 1 <= 64;
        CWCHK(c, decode_step(c, rows, false));
    }
    CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, n_prompt - 1, rows, c->st));
    CWCHK(c, KD(c, cw_launch_embed, c->d_ids, TGT, n_prompt - 1, c->embed, c->bf16 ? 1 : 0, c->dec_pos, c->dx, rows, D, c->st));
    KCHK(c);
    c->last_nb = rows; c->last_L = n_prompt - 1;
    return CW_OK;
}

// The candidate selection of one beam step on the first `rows` rows of the logits buffer (cw_beam_step, and cw_test_beam_topk on
// caller-supplied rows): [rows][n_cand] best (log-probability, token) pairs into d_cand_val / d_cand_id.
int launch_beam_topk(cw_ctx* c, int rows, int n_cand) {
    SampleParams sp = zeroed<SampleParams>();
    sp.logits = c->dlogits; sp.V = c->d.vocab_size; sp.ldv = c->Vpad; sp.B = rows; sp.mask = c->d_mask;
    sp.eos = c->gen.eos_token_id; sp.pad = c->gen.pad_token_id;
    sp.timestamp_begin = c->gen.no_timestamps_token_id + 1;
    sp.max_initial_timestamp_index = c->gen.max_initial_timestamp_index;
    sp.cfg = c->d_cfg; sp.pos = c->d_pos; sp.ids_stride = c->d.max_target_positions; sp.ids = c->d_ids;
    sp.embed_bf16 = c->bf16 ? 1 : 0;
    return KD(c, cw_launch_beam_topk, sp, n_cand, c->d_cand_val, c->d_cand_id, c->d_topk_scratch, c->st);
}

int32_t cw_beam_step(cw_ctx* c, int32_t n_cand, float* cand_logprob, int32_t* cand_token) {
    if (c->beam_K <= 0) return fail(c, CW_ERR_STATE, "cw_beam_begin not called");
    if (n_cand < 1 || n_cand > 64) return fail(c, CW_ERR_INVALID, "n_cand=%d out of range", n_cand);
    // the token chosen from this step sits at index beam_pos + 1: one step too many would write cache and alignment rows
    // beyond the limit the context was sized for
    if (c->beam_pos + 1 >= c->beam_max_len) return fail(c, CW_ERR_STATE, "beam_step: sequence already has max_length=%d tokens", c->beam_max_len);
    const int rows = c->beam_items * c->beam_K;
    StageTimer tm(c, CW_STAGE_DECODE);
    c->hist_short = c->beam_pos + 1 <= 64;   // keys 0 .. beam_pos
    CWCHK(c, decode_step(c, rows, true));
    CWCHK(c, launch_beam_topk(c, rows, n_cand));
    KCHK(c);
    tm.stop();
    HIPCHK(c, hipMemcpy(cand_logprob, c->d_cand_val, (size_t)rows * n_cand * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(cand_token, c->d_cand_id, (size_t)rows * n_cand * 4, hipMemcpyDeviceToHost));
    c->last_L += 1;                       // one more decoder input position has its alignment rows
    c->align_unnormalized = c->bf16 && c->d.n_align > 0;
    return CW_OK;
}

int32_t cw_beam_advance(cw_ctx* c, const int32_t* parent, const int32_t* token) {
    if (c->beam_K <= 0) return fail(c, CW_ERR_STATE, "cw_beam_begin not called");
    const int rows = c->beam_items * c->beam_K, V = c->d.vocab_size;
    for (int r = 0; r < rows; ++r) {
        if (parent[r] < 0 || parent[r] >= rows || parent[r] / c->beam_K != r / c->beam_K) return fail(c, CW_ERR_INVALID, "beam_advance: row %d cannot descend from row %d", r, parent[r]);
        if (token[r] < 0 || token[r] >= V) return fail(c, CW_ERR_INVALID, "beam_advance: token %d out of range", token[r]);
    }
    HIPCHK(c, hipMemcpyAsync(c->d_parent, parent, rows * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->d_tok, token, rows * 4, hipMemcpyHostToDevice, c->st));
    BeamAdvanceParams p;
    memset(&p, 0, sizeof(p));
    p.ids = c->d_ids; p.ids_tmp = c->d_ids_tmp; p.ids_stride = c->d.max_target_positions;
    p.anc = c->d_anc; p.anc_tmp = c->d_anc_tmp; p.cap = c->d.max_target_positions;
    p.parent = c->d_parent; p.token = c->d_tok; p.pos = c->d_pos;
    p.embed = c->embed; p.pos_embed = c->dec_pos; p.x_out = c->dx; p.d = c->d.d_model; p.embed_bf16 = c->bf16 ? 1 : 0;
    p.rows = rows;
    CWCHK(c, KD(c, cw_launch_beam_advance, p, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));                   // parent / token are caller-owned host buffers
    c->beam_pos += 1;
    return CW_OK;
}

int32_t cw_beam_finish(cw_ctx* c, int32_t n_items, int32_t L, const int32_t* row_of_pos) {
    if (c->beam_K <= 0) return fail(c, CW_ERR_STATE, "cw_beam_begin not called");
    const int rows = c->beam_items * c->beam_K, TGT = c->d.max_target_positions, Ha = c->d.n_align;
    if (n_items != c->beam_items || L < 0 || L > c->last_L) return fail(c, CW_ERR_INVALID, "beam_finish: %d items x %d rows requested, %d x %d decoded", n_items, L, c->beam_items, c->last_L);
    for (size_t i = 0; i < (size_t)n_items * L; ++i)
        if (row_of_pos[i] < 0 || row_of_pos[i] >= rows) return fail(c, CW_ERR_INVALID, "beam_finish: row %d out of range", row_of_pos[i]);
    if (Ha > 0 && L > 0) {
        if (!c->d_align_g) CWCHK(c, dmalloc(c, &c->d_align_g, (size_t)c->Bm * Ha * TGT * CW_N_CTX * 4, false));
        c->last_nb = rows;
        CWCHK(c, normalize_alignment(c));
        HIPCHK(c, hipMemcpyAsync(c->d_rowmap, row_of_pos, (size_t)n_items * L * 4, hipMemcpyHostToDevice, c->st));
        CWCHK(c, KD(c, cw_launch_align_gather, c->d_align, c->d_rowmap, n_items, Ha, TGT, L, CW_N_CTX, c->d_align_g, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        c->align_cur = c->d_align_g;
    }
    c->last_nb = n_items; c->last_L = L;
    c->beam_K = 0;                                            // back to one row per item
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// token timestamps
// ------------------------------------------------------------------------------------------------
static int run_alignment(cw_ctx* c, const float* w, int B, int Ha, int rows_cap, int S, int row0, int N,
                         const int* d_ncols, int width, float* mean, float* stdv, float* mat) {
    CWCHK(c, cw_launch_align_stats(w, B, Ha, rows_cap, S, row0, N, d_ncols, mean, stdv, c->st));
    CWCHK(c, cw_launch_align_filter(w, B, Ha, rows_cap, S, row0, N, d_ncols, mean, stdv, width, mat, c->st));
    return CW_OK;
}

static int token_timestamps(cw_ctx* c, const float* w, int32_t nb, int32_t L, int32_t n_prompt, const int32_t* num_frames, float* ts_out);

int32_t cw_token_timestamps(cw_ctx* c, int32_t nb, int32_t L, int32_t n_prompt, const int32_t* num_frames, float* ts_out) {
    if (c->d.n_align <= 0) return fail(c, CW_ERR_STATE, "no alignment heads configured");
    if (nb < 1 || nb > c->last_nb || L != c->last_L) return fail(c, CW_ERR_STATE, "rows retained: %d x %d, asked %d x %d", c->last_nb, c->last_L, nb, L);
    c->as_mass.clear(); c->as_spread.clear();
    return token_timestamps(c, nullptr, nb, L, n_prompt, num_frames, ts_out);
}

// Columns reaching the DTW, with HF's exact slicing semantics (:318-323 + :354): python-style
// `[..., : nf // 2]`, applied twice when every item has the same num_frames, once otherwise.
// nf <= 0 happens when the seek loop ran past the valid audio; it may leave zero columns.
static void timestamp_ncols(int nb, const int32_t* num_frames, std::vector<int>& ncols) {
    const int S = CW_N_CTX;
    ncols.resize(nb);
    bool uniform = true;
    for (int b = 1; b < nb; ++b) uniform = uniform && (num_frames[b] == num_frames[0]);
    auto floordiv2 = [](int v) { return (v >= 0) ? v / 2 : -((-v + 1) / 2); };
    auto slice_len = [](int n, int h) { return h >= 0 ? (h < n ? h : n) : (n + h > 0 ? n + h : 0); };
    for (int b = 0; b < nb; ++b) {
        int h = floordiv2(num_frames[b]);
        int n1 = slice_len(S, h);
        ncols[b] = uniform ? slice_len(n1, h) : n1;
    }
}

// stats -> filter -> DTW of nseq sequences (nseq <= max_batch) of N token rows each: w [nseq][Ha][rows_cap][S], token rows
// row0 .. row0 + N - 1, ncols[q] frames.  w null: the retained rows.  fc [nseq][N]: first frame of every token's run.
// sc non-null with cw_set_alignment_scores on: the path-score kernel runs behind the DTW on the rows and first columns it just
// produced (both stay on the device), and sc receives mass [nseq][N] followed by spread [nseq][N].
static int timestamp_first_cols(cw_ctx* c, const float* w, int nseq, int Ha, int rows_cap, int row0, int N, const int* ncols,
                                std::vector<int>& fc, std::vector<float>* sc = nullptr) {
    const int S = CW_N_CTX;
    HIPCHK(c, hipMemcpyAsync(c->d_ncols, ncols, nseq * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    StageTimer tm(c, CW_STAGE_TIMESTAMPS);
    CWCHK(c, normalize_alignment(c));
    if (!w) w = c->align_cur ? c->align_cur : c->d_align;
    CWCHK(c, run_alignment(c, w, nseq, Ha, rows_cap, S, row0, N, c->d_ncols, c->d.median_filter_width, c->d_mean, c->d_std, c->d_mat));
    {   // workspace of the wave-local DTW, grown on demand (diagonal-major copy of the cost matrices)
        const size_t need = cw_dtw_skew_floats(nseq, N, S);
        if (need > c->skew_cap) {
            // grown at most a few times: sized for the worst case of this batch size (N = max_target_positions) and the
            // previous buffer is released, so a token count that creeps upwards cannot pile up dead workspaces
            const size_t want = cw_dtw_skew_floats(nseq, c->d.max_target_positions, S) > need ? cw_dtw_skew_floats(nseq, c->d.max_target_positions, S) : need;
            if (c->d_skew) {
                HIPCHK(c, hipStreamSynchronize(c->st));
                for (auto it = c->allocs.begin(); it != c->allocs.end(); ++it)
                    if (*it == (void*)c->d_skew) { c->allocs.erase(it); break; }
                hipFree(c->d_skew);
                c->d_skew = nullptr; c->skew_cap = 0;
            }
            CWCHK(c, dmalloc(c, &c->d_skew, want * 4, false));
            c->skew_cap = want;
        }
    }
    CWCHK(c, cw_launch_dtw(c->d_mat, nseq, N, S, c->d_ncols, c->d_trace, c->d_first_col, c->sw.dtw_block ? c->d_path_text : nullptr, c->sw.dtw_block ? c->d_path_time : nullptr, c->d_path_len, c->st, c->sw.dtw_block ? nullptr : c->d_skew));
    const bool scores = sc && c->as_on;
    if (scores)
        CWCHK(c, cw_launch_align_path_score(w, nseq, Ha, rows_cap, S, row0, N, c->d_ncols, c->d_first_col, c->as_collar, c->d_as_mass,
                                            c->d_as_spread, c->st));
    KCHK(c);
    tm.stop();
    fc.resize((size_t)nseq * N);
    HIPCHK(c, hipMemcpy(fc.data(), c->d_first_col, fc.size() * 4, hipMemcpyDeviceToHost));
    if (scores) {
        sc->resize((size_t)2 * nseq * N);
        HIPCHK(c, hipMemcpy(sc->data(), c->d_as_mass, (size_t)nseq * N * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(sc->data() + (size_t)nseq * N, c->d_as_spread, (size_t)nseq * N * 4, hipMemcpyDeviceToHost));
    }
    return CW_OK;
}

// w: alignment rows of item 0 of the nb items in the [B][n_align][TGT][S] layout (null: the retained rows)
static int token_timestamps(cw_ctx* c, const float* w, int32_t nb, int32_t L, int32_t n_prompt, const int32_t* num_frames, float* ts_out) {
    const int Ha = c->d.n_align, TGT = c->d.max_target_positions;
    for (size_t i = 0; i < (size_t)nb * (L + 1); ++i) ts_out[i] = 0.f;
    const int N = L - n_prompt;
    // alignment scores: one row of L + 1 per sequence, appended to the rows of this timestamp stage (its caller cleared them);
    // NaN wherever no token row was scored (prompt positions, the eos slot, N <= 0)
    const size_t as0 = c->as_mass.size();
    if (c->as_on) {
        c->as_mass.resize(as0 + nb, std::vector<float>((size_t)L + 1, NAN));
        c->as_spread.resize(as0 + nb, std::vector<float>((size_t)L + 1, NAN));
    }
    if (N <= 0) return CW_OK;                     // generation_whisper.py:336-338
    std::vector<int> ncols, fc;
    std::vector<float> sc;
    timestamp_ncols(nb, num_frames, ncols);
    CWCHK(c, timestamp_first_cols(c, w, nb, Ha, TGT, n_prompt, N, ncols.data(), fc, &sc));
    if (c->as_on)
        for (int b = 0; b < nb; ++b) {
            memcpy(c->as_mass[as0 + b].data() + n_prompt, sc.data() + (size_t)b * N, (size_t)N * 4);
            memcpy(c->as_spread[as0 + b].data() + n_prompt, sc.data() + ((size_t)nb + b) * N, (size_t)N * 4);
        }
    for (int b = 0; b < nb; ++b) {
        float* ts = ts_out + (size_t)b * (L + 1);
        for (int i = 0; i < N; ++i) {
            // zero columns: the reference's backtrace walks up column 0 -> time index -1 for every token
            int col = ncols[b] > 0 ? fc[(size_t)b * N + i] : -1;
            ts[n_prompt + i] = (float)((double)col * 0.02);                                          // :369
        }
        ts[L] = ts[L - 1];                                                                          // :377-379
    }
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// native seek loop
// ------------------------------------------------------------------------------------------------
int32_t cw_transcribe(cw_ctx* c, int32_t B, const int32_t* num_frames, const cw_transcribe_cfg* cfg, int32_t* tokens,
                      float* token_ts, int32_t* lens, int32_t cap, int32_t* n_passes) {
    return cw_transcribe_prompted(c, B, num_frames, cfg, nullptr, 0, tokens, token_ts, lens, cap, n_passes);
}

int32_t cw_transcribe_prompted(cw_ctx* c, int32_t B, const int32_t* num_frames, const cw_transcribe_cfg* cfg,
                               const int32_t* prefix, int32_t n_prefix, int32_t* tokens, float* token_ts, int32_t* lens,
                               int32_t cap, int32_t* n_passes) {
    struct PrefixScope {                     // the decode calls of this seek loop carry n_prefix prompt_ids
        cw_ctx* c; int saved;
        ~PrefixScope() { c->pf_prefix = saved; }
    } scope{c, c->pf_prefix};
    c->pf_prefix = n_prefix > 0 ? n_prefix : 0;
    const int TGT = c->d.max_target_positions, V = c->d.vocab_size;
    if (B < 1 || B > c->Bm) return fail(c, CW_ERR_INVALID, "B=%d out of range (max_batch %d)", B, c->Bm);
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (n_prefix < 0 || (n_prefix > 0 && !prefix)) return fail(c, CW_ERR_INVALID, "prefix: n_prefix=%d", n_prefix);
    for (int k = 0; k < n_prefix; ++k)
        if (prefix[k] < 0 || prefix[k] >= V) return fail(c, CW_ERR_INVALID, "prefix token %d out of range", prefix[k]);
    if (n_prefix > 0 && (!isnan(c->logprob_thr) || !isnan(c->no_speech_thr)))
        return fail(c, CW_ERR_INVALID, "a decoder prompt prefix together with logprob / no-speech thresholds is not implemented");
    const int tb = c->gen.no_timestamps_token_id + 1;
    const int eos = c->gen.eos_token_id, pad = c->gen.pad_token_id;
    std::vector<std::vector<int>> prompts(B);
    std::vector<int> all(B), zeros(B, 0), full(B, CW_N_FRAMES);
    for (int i = 0; i < B; ++i) all[i] = i;
    bool pre_encoded = false;
    std::vector<float> lang_prob(B, NAN);            // NaN: the language was forced
    if (cfg->language_token >= 0) {
        for (int i = 0; i < B; ++i) {
            prompts[i] = {cfg->sot_token, cfg->language_token};
            if (cfg->task_token >= 0) prompts[i].push_back(cfg->task_token);
        }
    } else {   // detect_language (:1610-1673): one decoder step on <|startoftranscript|>, argmax over the language ids
        if (!cfg->lang_ids || cfg->n_lang_ids <= 0) return fail(c, CW_ERR_INVALID, "language detection needs lang_ids");
        CWCHK(c, cw_encode(c, B, all.data(), zeros.data(), full.data()));
        // (the logits stay on the device: langid.hip picks the arg-max, lowest id on a tie, and the candidates' softmax)
        std::vector<int> cand;                        // an id listed twice counts once, as in the host loop this replaces
        for (int k = 0; k < cfg->n_lang_ids; ++k)
            if (std::find(cand.begin(), cand.end(), cfg->lang_ids[k]) == cand.end()) cand.push_back(cfg->lang_ids[k]);
        const int n_cand = (int)cand.size();
        std::vector<int> best(B);
        std::vector<float> pr((size_t)B * n_cand);
        CWCHK(c, cw_detect_language(c, B, cfg->sot_token, cand.data(), n_cand, best.data(), pr.data(), nullptr));
        for (int i = 0; i < B; ++i) {
            prompts[i] = {cfg->sot_token, best[i]};
            if (cfg->task_token >= 0) prompts[i].push_back(cfg->task_token);
            for (int k = 0; k < n_cand; ++k)
                if (cand[k] == best[i]) lang_prob[i] = pr[(size_t)i * n_cand + k];
        }
        pre_encoded = true;
    }
    // what cw_get_transcribe_languages reports: slot 1 of the prompt where it is a language (one of cfg->lang_ids when given)
    c->tr_lang.assign(B, -1); c->tr_lang_prob = lang_prob;
    for (int i = 0; i < B; ++i) {
        const int tok = prompts[i][1];
        bool is_lang = !cfg->lang_ids || cfg->n_lang_ids <= 0;
        for (int k = 0; k < cfg->n_lang_ids && !is_lang; ++k) is_lang = cfg->lang_ids[k] == tok;
        if (is_lang) c->tr_lang[i] = tok;
    }
    // prompt_ids (generation_whisper.py:1909-1913): the prefix goes in front of every window's init tokens, after detection
    if (n_prefix > 0)
        for (int i = 0; i < B; ++i) prompts[i].insert(prompts[i].begin(), prefix, prefix + n_prefix);
    const int n_prompt = (int)prompts[0].size();
    int max_new = cfg->max_new_tokens;
    int max_length;
    if (n_prefix > 0) {                                                                // _set_max_new_tokens_and_length
        if ((max_new > 0 ? max_new : 0) + n_prompt > TGT)                              // :1920-1930
            return fail(c, CW_ERR_INVALID, "decoder input of %d tokens + max_new_tokens %d exceeds max_target_positions %d",
                        n_prompt, max_new, TGT);
        const int n_init = n_prompt < TGT / 2 - 1 ? n_prompt : TGT / 2 - 1;             // :1932-1946
        max_length = max_new >= 0 ? n_prompt + max_new : (cfg->max_length + n_init < TGT ? cfg->max_length + n_init : TGT);
    } else {
        if (max_new >= 0 && max_new + n_prompt > TGT) max_new = TGT - n_prompt;        // :1937-1942
        max_length = max_new >= 0 ? n_prompt + max_new : (cfg->max_length < TGT ? cfg->max_length : TGT);
    }
    if (max_length <= n_prompt) return fail(c, CW_ERR_INVALID, "max_length %d leaves no room after %d decoder input tokens", max_length, n_prompt);
    std::vector<long> seek(B, 0);
    std::vector<std::vector<int>> out_tok(B);
    std::vector<std::vector<float>> out_ts(B), out_lp(B), out_tl(B), out_am(B), out_as(B), out_en(B);
    std::vector<std::vector<int>> out_ti(B);
    c->tr_lp.clear();
    c->tr_ent.clear();
    c->tr_top_id.clear(); c->tr_top_lp.clear();
    c->tr_as_mass.clear(); c->tr_as_spread.clear();
    const int top_k = c->tok_lp_on ? c->top_k : 0;
    int passes = 0;
    for (;;) {
        std::vector<int> active, a_seek, a_n, a_nf;
        for (int i = 0; i < B; ++i)
            if (seek[i] < CW_N_FRAMES) {                                               // _maybe_reduce_batch
                active.push_back(i); a_seek.push_back((int)seek[i]);
                a_n.push_back((int)(CW_N_FRAMES - seek[i]));
                a_nf.push_back((int)(num_frames[i] - seek[i]));
            }
        if (active.empty()) break;
        const int nb = (int)active.size();
        if (!(pre_encoded && passes == 0)) CWCHK(c, cw_encode(c, nb, active.data(), a_seek.data(), a_n.data()));
        std::vector<int> prm((size_t)nb * n_prompt), seq((size_t)nb * TGT), ln(nb);
        for (int r = 0; r < nb; ++r) for (int k = 0; k < n_prompt; ++k) prm[(size_t)r * n_prompt + k] = prompts[active[r]][k];
        // deterministic half of generate_with_fallback: a window with a low average log-probability AND a high no-speech
        // probability is skipped (seek moves on by the whole window, no segment; :879-881, :1275-1285)
        const bool thr = !isnan(c->logprob_thr) && !isnan(c->no_speech_thr);
        std::vector<float> nsp(nb, 0.f), alp(nb, 0.f);
        if (thr) CWCHK(c, cw_no_speech_probs(c, nb, cfg->sot_token, nsp.data()));
        CWCHK(c, cw_decode(c, nb, prm.data(), n_prompt, max_length, cfg->min_new_tokens, nullptr, seq.data(), ln.data(), nullptr));
        if (thr) CWCHK(c, cw_get_avg_logprobs(c, alp.data(), nb));
        std::vector<float> tlp;
        if (c->tok_lp_on) { tlp.resize((size_t)nb * TGT); CWCHK(c, cw_get_token_logprobs(c, tlp.data(), nb)); }
        std::vector<float> ten;
        if (c->tok_ent_on) { ten.resize((size_t)nb * TGT); CWCHK(c, cw_get_token_entropy(c, ten.data(), nb)); }
        std::vector<int> tti; std::vector<float> ttl;
        if (top_k > 0) {
            tti.resize((size_t)nb * TGT * top_k); ttl.resize(tti.size());
            CWCHK(c, cw_get_top_logprobs(c, tti.data(), ttl.data(), nb));
        }
        int total = 0;
        for (int r = 0; r < nb; ++r) total = ln[r] > total ? ln[r] : total;
        const int L = total - 1;
        std::vector<float> ts((size_t)nb * (L + 1));
        CWCHK(c, cw_token_timestamps(c, nb, L, n_prompt, a_nf.data(), ts.data()));
        ++passes;
        for (int r = 0; r < nb; ++r) {
            const int i = active[r];
            if (thr && alp[r] < c->logprob_thr && nsp[r] > c->no_speech_thr) { seek[i] += a_n[r]; continue; }
            const int* s = seq.data() + (size_t)r * TGT + n_prompt;
            int n = total - n_prompt;
            if (n > 0 && s[n - 1] == pad) {                                            // strip right padding (:1060-1067)
                int npad = 0;
                for (int k = 0; k < n; ++k) npad += (s[k] == pad);
                if (pad == eos) npad -= 1;
                n -= npad;
            }
            if (n > 0 && s[n - 1] == eos) n -= 1;                                      // :1081-1082
            // _retrieve_segment: keep everything up to the last *pair* of timestamp tokens, or the whole window
            const double time_offset = (double)seek[i] * 0.02 / 2.0;
            const float off32 = (float)time_offset;
            const bool single_ending = n >= 2 && s[n - 2] < tb && s[n - 1] >= tb;
            int last_pair_end = -1;                                                    // index after the pair's 1st token
            for (int k = 0; k + 1 < n; ++k) if (s[k] >= tb && s[k + 1] >= tb) last_pair_end = k + 1;
            int keep, advance;
            if (last_pair_end >= 0) {
                if (single_ending) { keep = n; advance = a_n[r]; }
                else { keep = last_pair_end + 1; advance = (s[last_pair_end - 1] - tb) * 2; }
            } else { keep = n; advance = a_n[r]; }
            for (int k = 0; k < keep; ++k) {
                out_tok[i].push_back(s[k]);
                out_ts[i].push_back(ts[(size_t)r * (L + 1) + n_prompt + k] + off32);
                if (c->tok_lp_on) out_lp[i].push_back(tlp[(size_t)r * TGT + n_prompt + k]);
                if (c->tok_ent_on) out_en[i].push_back(ten[(size_t)r * TGT + n_prompt + k]);
                if (c->as_on) {                                                        // (rows of the cw_token_timestamps above)
                    out_am[i].push_back(c->as_mass[r][n_prompt + k]);
                    out_as[i].push_back(c->as_spread[r][n_prompt + k]);
                }
                if (top_k > 0) {
                    const size_t o = ((size_t)r * TGT + n_prompt + k) * top_k;
                    out_ti[i].insert(out_ti[i].end(), tti.begin() + o, tti.begin() + o + top_k);
                    out_tl[i].insert(out_tl[i].end(), ttl.begin() + o, ttl.begin() + o + top_k);
                }
            }
            seek[i] += advance;
        }
    }
    for (int i = 0; i < B; ++i) {
        const int n = (int)out_tok[i].size();
        if (n > cap) return fail(c, CW_ERR_INVALID, "item %d produced %d tokens, capacity %d", i, n, cap);
        lens[i] = n;
        memcpy(tokens + (size_t)i * cap, out_tok[i].data(), (size_t)n * 4);
        memcpy(token_ts + (size_t)i * cap, out_ts[i].data(), (size_t)n * 4);
    }
    if (c->tok_lp_on) c->tr_lp = std::move(out_lp);
    if (c->tok_ent_on) c->tr_ent = std::move(out_en);
    if (top_k > 0) { c->tr_top_id = std::move(out_ti); c->tr_top_lp = std::move(out_tl); }
    if (c->as_on) { c->tr_as_mass = std::move(out_am); c->tr_as_spread = std::move(out_as); }
    if (n_passes) *n_passes = passes;
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// forced alignment of known token sequences (include/crisperwhisper.h: cw_align_tokens)
// ------------------------------------------------------------------------------------------------
// whole decoder inputs (init tokens + text + eos) of cw_align_tokens / cw_score_tokens: every argument is checked before anything
// is launched.  num_frames null: not needed by the caller (scoring alone).  n_max: the longest row.
static int check_token_rows(cw_ctx* c, const char* who, int nb, const int32_t* num_frames, const int32_t* ids, int ids_stride,
                            const int32_t* n_ids, int n_init, int* n_max_out) {
    const int TGT = c->d.max_target_positions, V = c->d.vocab_size;
    if (n_init < 1 || n_init >= TGT) return fail(c, CW_ERR_INVALID, "%s: n_init=%d out of range", who, n_init);
    if (ids_stride < n_init + 1) return fail(c, CW_ERR_INVALID, "%s: ids_stride=%d below n_init + 1", who, ids_stride);
    int n_max = 0;
    for (int b = 0; b < nb; ++b) {
        const int n = n_ids[b];
        if (n < n_init + 1 || n > TGT || n > ids_stride)
            return fail(c, CW_ERR_INVALID, "%s: row %d has %d ids; needs %d .. %d (init tokens + eos .. max_target_positions)",
                        who, b, n, n_init + 1, TGT < ids_stride ? TGT : ids_stride);
        if (num_frames && (num_frames[b] < 0 || num_frames[b] > CW_N_FRAMES))
            return fail(c, CW_ERR_INVALID, "%s: num_frames[%d]=%d out of range 0 .. %d", who, b, num_frames[b], CW_N_FRAMES);
        for (int k = 0; k < n; ++k) {
            const int tok = ids[(size_t)b * ids_stride + k];
            if (tok < 0 || tok >= V) return fail(c, CW_ERR_INVALID, "%s: row %d id %d at %d is outside the vocabulary (%d)", who, b, tok, k, V);
            if (k >= n_init && k + 1 < n && tok == c->gen.eos_token_id)
                return fail(c, CW_ERR_INVALID, "%s: row %d has eos at %d before its last id", who, b, k);
        }
        n_max = n > n_max ? n : n_max;
    }
    *n_max_out = n_max;
    return CW_OK;
}

// timestamps over each row's own token count: a row's z-score statistics, filter and DTW see its own rows only, so its
// timestamps do not depend on the other rows of the batch.  Consecutive rows of one length share one pass of the stages
// (per-item work in every one of them; num_frames >= 0 makes the one- and two-fold slicing of the columns agree).
static int forced_rows_timestamps(cw_ctx* c, int nb, const int32_t* num_frames, int ids_stride, const int32_t* n_ids, int n_init,
                                  float* token_ts) {
    const int TGT = c->d.max_target_positions, Ha = c->d.n_align;
    CWCHK(c, normalize_alignment(c));
    const float* w0 = c->align_cur ? c->align_cur : c->d_align;
    std::vector<float> ts;
    c->as_mass.clear(); c->as_spread.clear();     // (every group below appends its rows: row b ends up at index b)
    for (int b0 = 0, b1; b0 < nb; b0 = b1) {
        for (b1 = b0 + 1; b1 < nb && n_ids[b1] == n_ids[b0]; ++b1) {}
        const int L = n_ids[b0] - 1, n = b1 - b0;
        ts.resize((size_t)n * (L + 1));
        CWCHK(c, token_timestamps(c, w0 + (size_t)b0 * Ha * TGT * CW_N_CTX, n, L, n_init, num_frames + b0, ts.data()));
        for (int r = 0; r < n; ++r) memcpy(token_ts + (size_t)(b0 + r) * ids_stride, ts.data() + (size_t)r * (L + 1), (size_t)(L + 1) * 4);
    }
    return CW_OK;
}

struct PrefixScope {                         // no prompt_ids here: the prompt prefill must not engage in the loop's decode
    cw_ctx* c; int saved;
    ~PrefixScope() { c->pf_prefix = saved; }
};

int32_t cw_align_tokens(cw_ctx* c, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                        const int32_t* n_ids, int32_t n_init, float* token_ts) {
    const int TGT = c->d.max_target_positions, Ha = c->d.n_align;
    if (Ha <= 0) return fail(c, CW_ERR_STATE, "align_tokens: no alignment heads configured");
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "align_tokens: nb=%d out of range (the context has %d rows)", nb, c->Bm);
    if (!num_frames || !ids || !n_ids || !token_ts) return fail(c, CW_ERR_INVALID, "align_tokens: null argument");
    int n_max = 0;
    CWCHK(c, check_token_rows(c, "align_tokens", nb, num_frames, ids, ids_stride, n_ids, n_init, &n_max));
    PrefixScope scope{c, c->pf_prefix};
    c->pf_prefix = 0;
    std::vector<int> all(nb), zeros(nb, 0), full(nb, CW_N_FRAMES);
    for (int i = 0; i < nb; ++i) all[i] = i;
    CWCHK(c, cw_encode(c, nb, all.data(), zeros.data(), full.data()));
    const int Lmax = n_max - 1;                  // decoder input positions 0 .. Lmax-1 (the last id of a row is only predicted)
    if (c->align_prefill && prefill_capable(c)) {
        // one teacher-forced forward of every row over positions 0 .. Lmax-1 (prefill.hip); positions beyond a row's own
        // length run on pad ids and are never read: causal self-attention keeps them out of the row's earlier positions
        std::vector<int> dev((size_t)nb * TGT, c->gen.pad_token_id);
        for (int b = 0; b < nb; ++b) memcpy(dev.data() + (size_t)b * TGT, ids + (size_t)b * ids_stride, (size_t)n_ids[b] * 4);
        c->beam_K = 0;
        c->align_cur = c->d_align;
        HIPCHK(c, hipMemcpyAsync(c->d_ids, dev.data(), dev.size() * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        StageTimer tm(c, CW_STAGE_DECODE);
        CWCHK(c, run_prefill(c, nb, Lmax + 1, 1, true));
        KCHK(c);
        tm.stop();
        ++c->align_prefill_runs;
        c->last_L = Lmax;
        c->last_nb = nb;
        c->align_unnormalized = true;
    } else {
        // the per-position decoder step: a greedy decode whose every generated token is forced (cw_decode's `forced`)
        std::vector<int> prompt((size_t)nb * n_init), forced((size_t)nb * TGT, -1), seq((size_t)nb * TGT), lens(nb);
        for (int b = 0; b < nb; ++b) {
            memcpy(prompt.data() + (size_t)b * n_init, ids + (size_t)b * ids_stride, (size_t)n_init * 4);
            for (int k = n_init; k < n_ids[b]; ++k) forced[(size_t)b * TGT + k] = ids[(size_t)b * ids_stride + k];
        }
        CWCHK(c, cw_decode(c, nb, prompt.data(), n_init, n_max, 0, forced.data(), seq.data(), lens.data(), nullptr));
        if (c->last_L < Lmax) return fail(c, CW_ERR_STATE, "align_tokens: the forced decode stopped at %d of %d positions", c->last_L, Lmax);
    }
    return forced_rows_timestamps(c, nb, num_frames, ids_stride, n_ids, n_init, token_ts);
}

// ------------------------------------------------------------------------------------------------
// per-head forced alignment (include/crisperwhisper.h: cw_align_heads)
// ------------------------------------------------------------------------------------------------
namespace {
// For the duration of cw_align_heads the context's alignment outputs are the call's capture buffer, its statistics and a slot
// table built from the requested heads.  Restores the context's own on every exit and leaves no retained rows behind, so a
// cw_token_timestamps / cw_get_alignment after the call is refused instead of answered from a buffer that no longer exists.
struct AlignSwapScope {
    cw_ctx* c;
    float *align, *ml; int* slot; int n_align, rows; std::vector<int> layers, heads;
    bool graphs;                             // the decode loop ran: its captured steps hold the call's pointers
    AlignSwapScope(cw_ctx* c_, float* cap, float* cap_ml, int* cap_slot, int n, int rows_, std::vector<int> l, std::vector<int> h)
        : c(c_), align(c_->d_align), ml(c_->d_align_ml), slot(c_->d_align_slot), n_align(c_->d.n_align), rows(c_->align_rows),
          layers(std::move(l)), heads(std::move(h)), graphs(false) {
        c->d_align = cap; c->d_align_ml = cap_ml; c->d_align_slot = cap_slot; c->d.n_align = n; c->align_rows = rows_;
        c->align_layers.swap(layers); c->align_heads.swap(heads);
        c->align_cur = cap;
    }
    void loop() { drop_step_graphs(c); graphs = true; }
    ~AlignSwapScope() {
        hipStreamSynchronize(c->st);
        if (graphs) drop_step_graphs(c);
        c->d_align = align; c->d_align_ml = ml; c->d_align_slot = slot; c->d.n_align = n_align; c->align_rows = rows;
        c->align_layers.swap(layers); c->align_heads.swap(heads);
        c->align_cur = c->d_align;
        c->last_nb = 0; c->last_L = 0; c->align_unnormalized = false;
    }
};
}  // namespace

static size_t cw_align_heads_bytes(int32_t nb, int32_t n_heads, int32_t rows) {
    return (size_t)nb * (size_t)n_heads * (size_t)rows * CW_N_CTX * 4;
}

int32_t cw_align_heads(cw_ctx* c, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                       const int32_t* n_ids, int32_t n_init, int32_t n_heads, const int32_t* layers, const int32_t* heads,
                       float* token_ts, const float* ref_begin, const float* ref_end, int32_t clip_frames, float* similarity) {
    const int TGT = c->d.max_target_positions, H = c->d.n_heads, NL = c->d.dec_layers, S = CW_N_CTX;
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "align_heads: nb=%d out of range (the context has %d rows)", nb, c->Bm);
    if (!num_frames || !ids || !n_ids || !token_ts || !layers || !heads) return fail(c, CW_ERR_INVALID, "align_heads: null argument");
    if (n_heads < 1 || n_heads > NL * H) return fail(c, CW_ERR_INVALID, "align_heads: n_heads=%d outside 1 .. %d", n_heads, NL * H);
    std::vector<int> slot((size_t)NL * H, -1);
    for (int k = 0; k < n_heads; ++k) {
        const int l = layers[k], h = heads[k];
        if (l < 0 || l >= NL || h < 0 || h >= H) return fail(c, CW_ERR_INVALID, "align_heads: head %d is (%d, %d), outside %d layers x %d heads", k, l, h, NL, H);
        if (slot[(size_t)l * H + h] >= 0) return fail(c, CW_ERR_INVALID, "align_heads: head (%d, %d) requested twice", l, h);
        slot[(size_t)l * H + h] = k;
    }
    if ((ref_begin == nullptr) != (ref_end == nullptr)) return fail(c, CW_ERR_INVALID, "align_heads: ref_begin and ref_end go together");
    const bool sim = ref_begin && similarity;
    int n_max = 0;
    CWCHK(c, check_token_rows(c, "align_heads", nb, num_frames, ids, ids_stride, n_ids, n_init, &n_max));
    const int Lmax = n_max - 1;                  // decoder input positions 0 .. Lmax-1 = capture rows per (item, head)
    const size_t cap_bytes = cw_align_heads_bytes(nb, n_heads, Lmax);
    if (cap_bytes > (size_t)CW_ALIGN_HEADS_MAX_BYTES)
        return fail(c, CW_ERR_INVALID, "align_heads: %d items x %d heads x %d positions need %zu bytes of attention rows, above the cap of %llu; pass fewer items or heads per call",
                    nb, n_heads, Lmax, cap_bytes, (unsigned long long)CW_ALIGN_HEADS_MAX_BYTES);

    float *cap = nullptr, *cap_ml = nullptr, *d_rb = nullptr, *d_re = nullptr, *d_sim = nullptr;
    int* cap_slot = nullptr;
    DevScope mem;                                // call-local device memory, released on every exit
    const size_t n_rows = (size_t)nb * n_heads * Lmax;
    if (mem.get(&cap, cap_bytes + (size_t)S * 4) != hipSuccess || mem.get(&cap_ml, n_rows * ATT_NS * 2 * 4) != hipSuccess ||
        mem.get(&cap_slot, slot.size() * 4) != hipSuccess)
        return fail(c, CW_ERR_NOMEM, "align_heads: hipMalloc of the %zu-byte capture failed", cap_bytes);
    HIPCHK(c, hipMemcpy(cap_slot, slot.data(), slot.size() * 4, hipMemcpyHostToDevice));
    // rows a shorter item never writes are read by nothing, but the similarity launch covers them: keep them defined
    HIPCHK(c, hipMemsetAsync(cap, 0, cap_bytes + (size_t)S * 4, c->st));
    HIPCHK(c, hipMemsetAsync(cap_ml, 0, n_rows * ATT_NS * 2 * 4, c->st));

    PrefixScope scope{c, c->pf_prefix};
    c->pf_prefix = 0;
    AlignSwapScope swap(c, cap, cap_ml, cap_slot, n_heads, Lmax,
                        std::vector<int>(layers, layers + n_heads), std::vector<int>(heads, heads + n_heads));
    std::vector<int> all(nb), zeros(nb, 0), full(nb, CW_N_FRAMES);
    for (int i = 0; i < nb; ++i) all[i] = i;
    CWCHK(c, cw_encode(c, nb, all.data(), zeros.data(), full.data()));
    // wall time of the call's four parts with the stream drained between them (cw_align_heads_times)
    auto lap = [c](std::chrono::steady_clock::time_point& t0) {
        hipStreamSynchronize(c->st);
        const auto t1 = std::chrono::steady_clock::now();
        const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    };
    auto t0 = std::chrono::steady_clock::now();
    lap(t0);
    if (c->align_prefill && prefill_capable(c)) {
        std::vector<int> dev((size_t)nb * TGT, c->gen.pad_token_id);
        for (int b = 0; b < nb; ++b) memcpy(dev.data() + (size_t)b * TGT, ids + (size_t)b * ids_stride, (size_t)n_ids[b] * 4);
        c->beam_K = 0;
        HIPCHK(c, hipMemcpyAsync(c->d_ids, dev.data(), dev.size() * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        StageTimer tm(c, CW_STAGE_DECODE);
        CWCHK(c, run_prefill(c, nb, Lmax + 1, 1, true));
        KCHK(c);
        tm.stop();
        ++c->align_prefill_runs;
        c->last_L = Lmax;
        c->last_nb = nb;
        c->align_unnormalized = true;
    } else {
        swap.loop();
        std::vector<int> prompt((size_t)nb * n_init), forced((size_t)nb * TGT, -1), seq((size_t)nb * TGT), lens(nb);
        for (int b = 0; b < nb; ++b) {
            memcpy(prompt.data() + (size_t)b * n_init, ids + (size_t)b * ids_stride, (size_t)n_init * 4);
            for (int k = n_init; k < n_ids[b]; ++k) forced[(size_t)b * TGT + k] = ids[(size_t)b * ids_stride + k];
        }
        CWCHK(c, cw_decode(c, nb, prompt.data(), n_init, n_max, 0, forced.data(), seq.data(), lens.data(), nullptr));
        c->align_cur = cap;            // (cw_decode points it at the context's d_align, which is the capture here)
        if (c->last_L < Lmax) return fail(c, CW_ERR_STATE, "align_heads: the forced decode stopped at %d of %d positions", c->last_L, Lmax);
        c->last_L = Lmax;                        // rows beyond Lmax - 1 do not exist in the capture
    }
    c->align_heads_ms[0] = lap(t0);
    CWCHK(c, normalize_alignment(c));
    c->align_heads_ms[1] = lap(t0);

    std::vector<int> ncols;
    timestamp_ncols(nb, num_frames, ncols);
    c->align_heads_ms[2] = c->align_heads_ms[4] = 0.f;
    if (sim) {   // the rows as normalised, before the timestamp stage reads them
        std::vector<float> rb((size_t)nb * Lmax, NAN), re((size_t)nb * Lmax, NAN), out((size_t)n_heads * nb * Lmax);
        for (int b = 0; b < nb; ++b)
            for (int k = n_init; k < n_ids[b] - 1; ++k) {
                rb[(size_t)b * Lmax + k] = ref_begin[(size_t)b * ids_stride + k];
                re[(size_t)b * Lmax + k] = ref_end[(size_t)b * ids_stride + k];
            }
        if (mem.get(&d_rb, rb.size() * 4) != hipSuccess || mem.get(&d_re, re.size() * 4) != hipSuccess || mem.get(&d_sim, out.size() * 4) != hipSuccess)
            return fail(c, CW_ERR_NOMEM, "align_heads: hipMalloc of the similarity buffers failed");
        HIPCHK(c, hipMemcpyAsync(c->d_ncols, ncols.data(), nb * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(d_rb, rb.data(), rb.size() * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(d_re, re.data(), re.size() * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        StageTimer tm(c, CW_STAGE_TIMESTAMPS);
        CWCHK(c, cw_launch_align_similarity(cap, nb, n_heads, Lmax, S, 0, Lmax, c->d_ncols, d_rb, d_re, clip_frames, d_sim, c->st));
        KCHK(c);
        tm.stop();
        hipEventElapsedTime(&c->align_heads_ms[4], c->ev0, c->ev1);     // the events tm just recorded around the launch
        HIPCHK(c, hipMemcpy(out.data(), d_sim, out.size() * 4, hipMemcpyDeviceToHost));
        for (int k = 0; k < n_heads; ++k)
            for (int b = 0; b < nb; ++b) {
                float* dst = similarity + ((size_t)k * nb + b) * ids_stride;
                for (int t = 0; t < ids_stride; ++t) dst[t] = t < Lmax ? out[((size_t)k * nb + b) * Lmax + t] : NAN;
            }
        c->align_heads_ms[2] = lap(t0);
    } else if (similarity) {
        for (size_t i = 0; i < (size_t)n_heads * nb * ids_stride; ++i) similarity[i] = NAN;
    }

    // timestamps: the (item, head) sequences are [nb * n_heads][1][Lmax][S]; consecutive sequences of one token count share
    // a pass of the stages, at most max_batch of them (the workspaces' size)
    for (size_t i = 0; i < (size_t)n_heads * nb * ids_stride; ++i) token_ts[i] = 0.f;
    const int n_seq = nb * n_heads;
    std::vector<int> nc, fc;
    for (int q0 = 0, q1; q0 < n_seq; q0 = q1) {
        const int L = n_ids[q0 / n_heads] - 1, N = L - n_init;
        for (q1 = q0 + 1; q1 < n_seq && q1 - q0 < c->Bm && n_ids[q1 / n_heads] - 1 == L; ++q1) {}
        if (N <= 0) continue;
        nc.resize(q1 - q0);
        for (int q = q0; q < q1; ++q) nc[q - q0] = ncols[q / n_heads];
        CWCHK(c, timestamp_first_cols(c, cap + (size_t)q0 * Lmax * S, q1 - q0, 1, Lmax, n_init, N, nc.data(), fc));
        for (int q = q0; q < q1; ++q) {
            const int b = q / n_heads, k = q % n_heads;
            float* ts = token_ts + ((size_t)k * nb + b) * ids_stride;
            for (int i = 0; i < N; ++i) {
                const int col = ncols[b] > 0 ? fc[(size_t)(q - q0) * N + i] : -1;
                ts[n_init + i] = (float)((double)col * 0.02);
            }
            ts[L] = ts[L - 1];
        }
    }
    c->align_heads_ms[3] = lap(t0);
    return CW_OK;
}

int32_t cw_align_heads_times(cw_ctx* c, float* ms) {
    memcpy(ms, c->align_heads_ms, sizeof(c->align_heads_ms));
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// scoring of known token sequences (include/crisperwhisper.h: cw_score_tokens, cw_align_score_tokens)
// ------------------------------------------------------------------------------------------------
static int score_reserve(cw_ctx* c, size_t M, size_t parts) {
    const size_t D = c->d.d_model;
    CWCHK(c, regrow(c, "score", c->sc_rows, M, {{(void**)&c->sc_src, M * 4}, {(void**)&c->sc_tgt, M * 4}, {(void**)&c->sc_ti, M * 4},
                                                {&c->sc_a, M * D * 2}, {(void**)&c->sc_lp, M * 4}, {(void**)&c->sc_tl, M * 4}}));
    return regrow(c, "score", c->sc_parts, parts, {{(void**)&c->sc_part, parts * sizeof(ScorePart)}});
}

// what cw_align_cut_tokens needs on top: stop_logprob [M] and the stop records of the head, the cut kernel's [Bm] arrays
static int cut_reserve(cw_ctx* c, size_t M, size_t parts) {
    CWCHK(c, regrow(c, "align_cut", c->sc_stop_rows, M, {{(void**)&c->sc_stop, M * 4}}));
    CWCHK(c, regrow(c, "align_cut", c->sc_sparts, parts, {{(void**)&c->sc_spart, parts * sizeof(ScoreStopPart)}}));
    if (!c->cut_ok) {
        const size_t Bm = (size_t)c->Bm;
        CWCHK(c, dmalloc(c, &c->cut_base, Bm * 4)); CWCHK(c, dmalloc(c, &c->cut_ntok, Bm * 4)); CWCHK(c, dmalloc(c, &c->cut_out, Bm * 4));
        CWCHK(c, dmalloc(c, &c->cut_score, Bm * 4)); CWCHK(c, dmalloc(c, &c->cut_force, Bm));
        CWCHK(c, dmalloc(c, &c->cut_ok, Bm * c->d.max_target_positions));
    }
    return CW_OK;
}

// what cw_set_score_top_logprobs needs on top: the head's per-split lists and its [M][CW_TOP_LOGPROBS_MAX] results
static int top_reserve(cw_ctx* c, size_t M, size_t parts) {
    CWCHK(c, regrow(c, "score", c->sc_alt_rows, M, {{(void**)&c->sc_alt_id, M * CW_TOP_LOGPROBS_MAX * 4}, {(void**)&c->sc_alt_lp, M * CW_TOP_LOGPROBS_MAX * 4}}));
    return regrow(c, "score", c->sc_tparts, parts, {{(void**)&c->sc_tpart, parts * CW_TOP_LOGPROBS_MAX * sizeof(ScoreTopPart)}});
}

// what cw_set_score_entropy needs on top: the head's per-split centred sums and its [M] results
static int ent_reserve(cw_ctx* c, size_t M, size_t parts) {
    CWCHK(c, regrow(c, "score", c->sc_ent_rows, M, {{(void**)&c->sc_ent, M * 4}}));
    return regrow(c, "score", c->sc_eparts, parts, {{(void**)&c->sc_epart, parts * 4}});
}

// the host copy cw_get_score_top_logprobs answers from: [rows][ids_stride][CW_TOP_LOGPROBS_MAX], -1 / NaN until a position is filled
static void top_results_begin(cw_ctx* c, int rows, int ids_stride) {
    const size_t n = (size_t)rows * ids_stride * CW_TOP_LOGPROBS_MAX;
    c->sc_top_ids.assign(n, -1);
    c->sc_top_lps.assign(n, std::numeric_limits<float>::quiet_NaN());
}

// cw_align_cut_tokens' extra arguments; null through score_rows: the plain scoring calls
struct CutArgs {
    const uint8_t* cut_ok;       // [rows][ids_stride]
    const uint8_t* force_all;    // [rows]
    int32_t* cut;                // [rows] out
    float* cut_score;            // [rows] out
    float* stop_logprob;         // [rows][ids_stride] out
};

// the cut kernel's arguments, uploaded before the forward: row r's scores start at base[r] in the arrays the head fills
static int cut_upload(cw_ctx* c, int rows, int ids_stride, const int32_t* n_ids, int n_init, const CutArgs& ca,
                      const std::vector<int>& base) {
    const int TGT = c->d.max_target_positions;
    std::vector<int> ntok(rows);
    std::vector<uint8_t> ok((size_t)rows * TGT, 0), force(rows);
    for (int r = 0; r < rows; ++r) {
        ntok[r] = n_ids[r] - n_init - 1;
        force[r] = ca.force_all[r] ? 1 : 0;
        memcpy(ok.data() + (size_t)r * TGT, ca.cut_ok + (size_t)r * ids_stride, (size_t)ntok[r] + 1);
    }
    HIPCHK(c, hipMemcpyAsync(c->cut_base, base.data(), (size_t)rows * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->cut_ntok, ntok.data(), (size_t)rows * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->cut_force, force.data(), (size_t)rows, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->cut_ok, ok.data(), ok.size(), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));      // host vectors go out of scope
    return CW_OK;
}

// The scoring head over the residual stream run_prefill (full) leaves in pf_x [rows][n_pos][D]: position p of a row predicts id
// p + 1, and only positions n_init-1 .. n_ids[row]-2 are projected.  score_head_prepare uploads their list and targets (they
// depend on the arguments alone, so before the forward), score_head_launch queues the kernels behind the forward,
// score_head_fetch reads the results.
static int score_head_prepare(cw_ctx* c, int rows, int n_pos, const int32_t* ids, int ids_stride, const int32_t* n_ids, int n_init,
                              int* M_out) {
    std::vector<int> src, tgt;
    for (int r = 0; r < rows; ++r)
        for (int k = n_init; k < n_ids[r]; ++k) { src.push_back(r * n_pos + k - 1); tgt.push_back(ids[(size_t)r * ids_stride + k]); }
    const int M = (int)src.size(), V = c->d.vocab_size, D = c->d.d_model;
    const int ns = KD(c, cw_score_head_splits, M, V, nullptr);
    CWCHK(c, score_reserve(c, (size_t)M, (size_t)M * ns));
    HIPCHK(c, hipMemcpyAsync(c->sc_src, src.data(), (size_t)M * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->sc_tgt, tgt.data(), (size_t)M * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));      // host vectors go out of scope
    *M_out = M;
    return CW_OK;
}

static int score_head_launch(cw_ctx* c, int M, int cut_rows = 0) {
    const int V = c->d.vocab_size, D = c->d.d_model;
    CWCHK(c, KD(c, cw_launch_score_ln, c->pf_x, c->sc_src, c->dec_ln_g, c->dec_ln_b, c->sc_a, M, D, c->st));
    CWCHK(c, KD(c, cw_launch_score_head, c->sc_a, c->embed_pk, c->sc_tgt, M, V, D, score_out(c, cut_rows > 0, false), c->st));
    if (cut_rows > 0)                            // cw_align_cut_tokens: the STOP head, then the cut on the arrays it leaves
        CWCHK(c, cw_launch_align_cut(c->sc_lp, c->sc_stop, c->cut_base, c->cut_ntok, c->cut_ok, c->d.max_target_positions, c->cut_force,
                                     cut_rows, c->cut_out, c->cut_score, c->st));
    return CW_OK;
}

static int score_head_fetch(cw_ctx* c, int rows, int M, int ids_stride, const int32_t* n_ids, int n_init, float* token_logprob,
                            int32_t* top_id, float* top_logprob, const CutArgs* ca = nullptr) {
    std::vector<float> lp(M), tl(M), sl(ca ? M : 0);
    std::vector<int> ti(M);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(lp.data(), c->sc_lp, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ti.data(), c->sc_ti, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(tl.data(), c->sc_tl, (size_t)M * 4, hipMemcpyDeviceToHost));
    if (ca) {
        HIPCHK(c, hipMemcpy(sl.data(), c->sc_stop, (size_t)M * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ca->cut, c->cut_out, (size_t)rows * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ca->cut_score, c->cut_score, (size_t)rows * 4, hipMemcpyDeviceToHost));
    }
    int m = 0;
    for (int r = 0; r < rows; ++r)
        for (int k = n_init; k < n_ids[r]; ++k, ++m) {
            token_logprob[(size_t)r * ids_stride + k] = lp[m];
            if (top_id) top_id[(size_t)r * ids_stride + k] = ti[m];
            if (top_logprob) top_logprob[(size_t)r * ids_stride + k] = tl[m];
            if (ca) ca->stop_logprob[(size_t)r * ids_stride + k] = sl[m];
        }
    if (c->sc_top_k > 0) {                       // the alternatives stay with the context (cw_get_score_top_logprobs)
        const size_t W = CW_TOP_LOGPROBS_MAX;
        std::vector<int> ai((size_t)M * W);
        std::vector<float> al((size_t)M * W);
        HIPCHK(c, hipMemcpy(ai.data(), c->sc_alt_id, ai.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(al.data(), c->sc_alt_lp, al.size() * 4, hipMemcpyDeviceToHost));
        top_results_begin(c, rows, ids_stride);
        m = 0;
        for (int r = 0; r < rows; ++r)
            for (int k = n_init; k < n_ids[r]; ++k, ++m) {
                memcpy(&c->sc_top_ids[((size_t)r * ids_stride + k) * W], &ai[(size_t)m * W], W * 4);
                memcpy(&c->sc_top_lps[((size_t)r * ids_stride + k) * W], &al[(size_t)m * W], W * 4);
            }
    }
    if (c->sc_ent_on) {                          // the entropies stay with the context too (cw_get_score_entropy)
        std::vector<float> en((size_t)M);
        HIPCHK(c, hipMemcpy(en.data(), c->sc_ent, en.size() * 4, hipMemcpyDeviceToHost));
        c->sc_ents.assign((size_t)rows * ids_stride, std::numeric_limits<float>::quiet_NaN());
        m = 0;
        for (int r = 0; r < rows; ++r)
            for (int k = n_init; k < n_ids[r]; ++k, ++m) c->sc_ents[(size_t)r * ids_stride + k] = en[m];
    }
    return CW_OK;
}

// num_frames / token_ts null: scores only (any rows_per_item); else rows_per_item == 1 and the timestamps of cw_align_tokens too.
// ca non-null (cw_align_cut_tokens, with token_ts): the STOP head and the cut kernel behind the same forward, and the timestamp
// stage over row b's first n_init + cut[b] + 1 ids -- the forward is causal, so those rows are what the prefix alone would give.
static int score_rows(cw_ctx* c, const char* who, int n_items, int rpi, const int32_t* num_frames, const int32_t* ids, int ids_stride,
                      const int32_t* n_ids, int n_init, float* token_ts, float* token_logprob, int32_t* top_id, float* top_logprob,
                      const CutArgs* ca = nullptr) {
    const int TGT = c->d.max_target_positions;
    const bool align = token_ts != nullptr;
    if (align && c->d.n_align <= 0) return fail(c, CW_ERR_STATE, "%s: no alignment heads configured", who);
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (rpi < 1) return fail(c, CW_ERR_INVALID, "%s: rows_per_item=%d below 1", who, rpi);
    if (n_items < 1 || n_items > c->Bm || (long long)n_items * rpi > c->Bm)
        return fail(c, CW_ERR_INVALID, "%s: %d items x %d rows out of range (the context has %d rows)", who, n_items, rpi, c->Bm);
    if (!ids || !n_ids || !token_logprob || (align && !num_frames)) return fail(c, CW_ERR_INVALID, "%s: null argument", who);
    const int rows = n_items * rpi;
    int n_max = 0;
    CWCHK(c, check_token_rows(c, who, rows, num_frames, ids, ids_stride, n_ids, n_init, &n_max));
    if (ca)
        for (int b = 0; b < rows; ++b) {
            bool any = ca->force_all[b] != 0;
            for (int n = 0; !any && n <= n_ids[b] - n_init - 1; ++n) any = ca->cut_ok[(size_t)b * ids_stride + n] != 0;
            if (!any) return fail(c, CW_ERR_INVALID, "%s: row %d is not forced and its cut_ok allows no cut", who, b);
        }
    PrefixScope scope{c, c->pf_prefix};
    c->pf_prefix = 0;
    const int Lmax = n_max - 1;
    c->sc_top_rows = 0;                          // cw_get_score_top_logprobs answers for a call that came to its end only
    c->sc_ent_nrows = 0;                         // ... and so does cw_get_score_entropy
    if (c->score_prefill && prefill_capable(c)) {
        // one encoder pass per item; decoder row r reads the cross K/V cache of item r / rows_per_item
        std::vector<int> all(n_items), zeros(n_items, 0), full(n_items, CW_N_FRAMES);
        for (int i = 0; i < n_items; ++i) all[i] = i;
        CWCHK(c, cw_encode(c, n_items, all.data(), zeros.data(), full.data()));
        std::vector<int> dev((size_t)rows * TGT, c->gen.pad_token_id);
        for (int b = 0; b < rows; ++b) memcpy(dev.data() + (size_t)b * TGT, ids + (size_t)b * ids_stride, (size_t)n_ids[b] * 4);
        c->beam_K = 0;
        c->align_cur = c->d_align;
        HIPCHK(c, hipMemcpyAsync(c->d_ids, dev.data(), dev.size() * 4, hipMemcpyHostToDevice, c->st));
        int M = 0;
        CWCHK(c, score_head_prepare(c, rows, Lmax, ids, ids_stride, n_ids, n_init, &M));     // (synchronises the stream)
        if (c->sc_top_k > 0) CWCHK(c, top_reserve(c, (size_t)M, (size_t)M * KD(c, cw_score_head_splits, M, c->d.vocab_size, nullptr)));
        if (c->sc_ent_on) CWCHK(c, ent_reserve(c, (size_t)M, (size_t)M * KD(c, cw_score_head_splits, M, c->d.vocab_size, nullptr)));
        if (ca) {
            CWCHK(c, cut_reserve(c, (size_t)M, (size_t)M * KD(c, cw_score_head_splits, M, c->d.vocab_size, nullptr)));
            std::vector<int> first(rows, 0);     // the head's arrays hold row after row, n_ids - n_init entries each
            for (int r = 1; r < rows; ++r) first[r] = first[r - 1] + n_ids[r - 1] - n_init;
            CWCHK(c, cut_upload(c, rows, ids_stride, n_ids, n_init, *ca, first));
        }
        StageTimer tm(c, CW_STAGE_DECODE);
        CWCHK(c, run_prefill(c, rows, Lmax + 1, rpi, align, true));
        CWCHK(c, score_head_launch(c, M, ca ? rows : 0));
        KCHK(c);
        tm.stop();
        ++c->score_prefill_runs;
        c->last_L = align ? Lmax : 0;            // without align no alignment rows were recorded: nothing is retained
        c->last_nb = align ? rows : 0;
        c->align_unnormalized = align;
        CWCHK(c, score_head_fetch(c, rows, M, ids_stride, n_ids, n_init, token_logprob, top_id, top_logprob, ca));
    } else {
        // the per-position decoder step with every token forced; the item is encoded into each of its rows, and the raw logits
        // of every step are reduced on the device (score_rows_kernel) before the next step overwrites them
        std::vector<int> item(rows), zeros(rows, 0), full(rows, CW_N_FRAMES);
        for (int r = 0; r < rows; ++r) item[r] = r / rpi;
        CWCHK(c, cw_encode(c, rows, item.data(), zeros.data(), full.data()));
        if (!c->sc_step_lp) {
            const size_t n = (size_t)c->Bm * TGT * 4;
            CWCHK(c, dmalloc(c, &c->sc_step_lp, n)); CWCHK(c, dmalloc(c, &c->sc_step_tl, n)); CWCHK(c, dmalloc(c, &c->sc_step_ti, n));
        }
        if (c->sc_top_k > 0 && !c->sc_step_alt_id) {
            const size_t n = (size_t)c->Bm * TGT * CW_TOP_LOGPROBS_MAX * 4;
            CWCHK(c, dmalloc(c, &c->sc_step_alt_id, n)); CWCHK(c, dmalloc(c, &c->sc_step_alt_lp, n));
        }
        if (c->sc_ent_on && !c->sc_step_ent) CWCHK(c, dmalloc(c, &c->sc_step_ent, (size_t)c->Bm * TGT * 4));
        if (ca) {
            if (!c->sc_step_stop) CWCHK(c, dmalloc(c, &c->sc_step_stop, (size_t)c->Bm * TGT * 4));
            CWCHK(c, cut_reserve(c, 0, 0));
            std::vector<int> first(rows);        // the loop's arrays are [rows][TGT], indexed by position
            for (int r = 0; r < rows; ++r) first[r] = r * TGT + n_init;
            CWCHK(c, cut_upload(c, rows, ids_stride, n_ids, n_init, *ca, first));
        }
        std::vector<int> prompt((size_t)rows * n_init), forced((size_t)rows * TGT, -1), seq((size_t)rows * TGT), lens(rows);
        for (int b = 0; b < rows; ++b) {
            memcpy(prompt.data() + (size_t)b * n_init, ids + (size_t)b * ids_stride, (size_t)n_init * 4);
            for (int k = n_init; k < n_ids[b]; ++k) forced[(size_t)b * TGT + k] = ids[(size_t)b * ids_stride + k];
        }
        struct HookScope { cw_ctx* c; ~HookScope() { c->score_hook = false; c->score_stop = false; } } hook{c};
        c->score_hook = true;
        c->score_stop = ca != nullptr;
        CWCHK(c, cw_decode(c, rows, prompt.data(), n_init, n_max, 0, forced.data(), seq.data(), lens.data(), nullptr));
        c->score_hook = false;
        c->score_stop = false;
        if (c->last_L < Lmax) return fail(c, CW_ERR_STATE, "%s: the forced decode stopped at %d of %d positions", who, c->last_L, Lmax);
        std::vector<float> lp((size_t)rows * TGT), tl((size_t)rows * TGT), sl(ca ? (size_t)rows * TGT : 0);
        std::vector<int> ti((size_t)rows * TGT);
        if (ca) {                                // the cut over the loop's [rows][TGT] arrays; the copies below wait for it
            CWCHK(c, cw_launch_align_cut(c->sc_step_lp, c->sc_step_stop, c->cut_base, c->cut_ntok, c->cut_ok, TGT, c->cut_force, rows,
                                         c->cut_out, c->cut_score, c->st));
            KCHK(c);
            HIPCHK(c, hipStreamSynchronize(c->st));
            HIPCHK(c, hipMemcpy(sl.data(), c->sc_step_stop, sl.size() * 4, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(ca->cut, c->cut_out, (size_t)rows * 4, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(ca->cut_score, c->cut_score, (size_t)rows * 4, hipMemcpyDeviceToHost));
        }
        HIPCHK(c, hipMemcpy(lp.data(), c->sc_step_lp, lp.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ti.data(), c->sc_step_ti, ti.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(tl.data(), c->sc_step_tl, tl.size() * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; ++r)
            for (int k = n_init; k < n_ids[r]; ++k) {
                token_logprob[(size_t)r * ids_stride + k] = lp[(size_t)r * TGT + k];
                if (top_id) top_id[(size_t)r * ids_stride + k] = ti[(size_t)r * TGT + k];
                if (top_logprob) top_logprob[(size_t)r * ids_stride + k] = tl[(size_t)r * TGT + k];
                if (ca) ca->stop_logprob[(size_t)r * ids_stride + k] = sl[(size_t)r * TGT + k];
            }
        if (c->sc_top_k > 0) {                   // the loop's [rows][TGT][CW_TOP_LOGPROBS_MAX], indexed by position
            const size_t W = CW_TOP_LOGPROBS_MAX;
            std::vector<int> ai((size_t)rows * TGT * W);
            std::vector<float> al((size_t)rows * TGT * W);
            HIPCHK(c, hipMemcpy(ai.data(), c->sc_step_alt_id, ai.size() * 4, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(al.data(), c->sc_step_alt_lp, al.size() * 4, hipMemcpyDeviceToHost));
            top_results_begin(c, rows, ids_stride);
            for (int r = 0; r < rows; ++r)
                for (int k = n_init; k < n_ids[r]; ++k) {
                    memcpy(&c->sc_top_ids[((size_t)r * ids_stride + k) * W], &ai[((size_t)r * TGT + k) * W], W * 4);
                    memcpy(&c->sc_top_lps[((size_t)r * ids_stride + k) * W], &al[((size_t)r * TGT + k) * W], W * 4);
                }
        }
        if (c->sc_ent_on) {                      // the loop's [rows][TGT], indexed by position
            std::vector<float> en((size_t)rows * TGT);
            HIPCHK(c, hipMemcpy(en.data(), c->sc_step_ent, en.size() * 4, hipMemcpyDeviceToHost));
            c->sc_ents.assign((size_t)rows * ids_stride, std::numeric_limits<float>::quiet_NaN());
            for (int r = 0; r < rows; ++r)
                for (int k = n_init; k < n_ids[r]; ++k) c->sc_ents[(size_t)r * ids_stride + k] = en[(size_t)r * TGT + k];
        }
    }
    if (c->sc_top_k > 0) { c->sc_top_rows = rows; c->sc_top_stride = ids_stride; }
    if (c->sc_ent_on) { c->sc_ent_nrows = rows; c->sc_ent_stride = ids_stride; }
    if (ca) {
        std::vector<int32_t> kept(rows);         // init tokens + the kept text + the slot cw_align_tokens gives the eos
        for (int b = 0; b < rows; ++b) {
            if (ca->cut[b] < 0 || ca->cut[b] > n_ids[b] - n_init - 1) return fail(c, CW_ERR_STATE, "%s: row %d came back with cut %d", who, b, ca->cut[b]);
            kept[b] = n_init + ca->cut[b] + 1;
        }
        return forced_rows_timestamps(c, rows, num_frames, ids_stride, kept.data(), n_init, token_ts);
    }
    if (align) return forced_rows_timestamps(c, rows, num_frames, ids_stride, n_ids, n_init, token_ts);
    return CW_OK;
}

int32_t cw_score_tokens(cw_ctx* c, int32_t n_items, int32_t rows_per_item, const int32_t* ids, int32_t ids_stride,
                        const int32_t* n_ids, int32_t n_init, float* token_logprob, int32_t* top_id, float* top_logprob) {
    return score_rows(c, "score_tokens", n_items, rows_per_item, nullptr, ids, ids_stride, n_ids, n_init, nullptr, token_logprob,
                      top_id, top_logprob);
}

int32_t cw_align_score_tokens(cw_ctx* c, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                              const int32_t* n_ids, int32_t n_init, float* token_ts, float* token_logprob, int32_t* top_id,
                              float* top_logprob) {
    if (!token_ts) return fail(c, CW_ERR_INVALID, "align_score_tokens: null argument");
    return score_rows(c, "align_score_tokens", nb, 1, num_frames, ids, ids_stride, n_ids, n_init, token_ts, token_logprob, top_id,
                      top_logprob);
}

int32_t cw_align_cut_tokens(cw_ctx* c, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                            const int32_t* n_ids, int32_t n_init, const uint8_t* cut_ok, const uint8_t* force_all, int32_t* cut,
                            float* cut_score, float* token_ts, float* token_logprob, float* stop_logprob, int32_t* top_id,
                            float* top_logprob) {
    if (!cut_ok || !force_all || !cut || !cut_score || !token_ts || !token_logprob || !stop_logprob)
        return fail(c, CW_ERR_INVALID, "align_cut_tokens: null argument");
    const CutArgs ca{cut_ok, force_all, cut, cut_score, stop_logprob};
    return score_rows(c, "align_cut_tokens", nb, 1, num_frames, ids, ids_stride, n_ids, n_init, token_ts, token_logprob, top_id,
                      top_logprob, &ca);
}

// ---- alternatives of the teacher-forced positions (include/crisperwhisper.h) ----------------------------------------------------
int32_t cw_set_score_top_logprobs(cw_ctx* c, int32_t k) {
    if (k < 0 || k > CW_TOP_LOGPROBS_MAX) return fail(c, CW_ERR_INVALID, "set_score_top_logprobs: k=%d outside 0 .. %d", k, CW_TOP_LOGPROBS_MAX);
    c->sc_top_k = k;
    c->sc_top_rows = 0;                          // what an earlier call stored was stored for its own k
    if (k == 0) { c->sc_top_ids.clear(); c->sc_top_lps.clear(); }
    return CW_OK;
}

int32_t cw_get_score_top_logprobs(cw_ctx* c, int32_t* ids_out, float* lp_out, int32_t rows, int32_t ids_stride) {
    if (c->sc_top_k < 1) return fail(c, CW_ERR_STATE, "score top_logprobs is off (cw_set_score_top_logprobs)");
    if (!ids_out || !lp_out || rows < 1 || ids_stride < 1) return fail(c, CW_ERR_INVALID, "get_score_top_logprobs: bad arguments");
    if (rows > c->sc_top_rows || ids_stride != c->sc_top_stride)
        return fail(c, CW_ERR_STATE, "get_score_top_logprobs: asked %d rows of stride %d, the last scoring call stored %d of stride %d", rows,
                    ids_stride, c->sc_top_rows, c->sc_top_stride);
    const size_t n = (size_t)rows * ids_stride, k = (size_t)c->sc_top_k;
    for (size_t i = 0; i < n; ++i) {             // stored rows are CW_TOP_LOGPROBS_MAX wide, the caller's k
        memcpy(ids_out + i * k, &c->sc_top_ids[i * CW_TOP_LOGPROBS_MAX], k * 4);
        memcpy(lp_out + i * k, &c->sc_top_lps[i * CW_TOP_LOGPROBS_MAX], k * 4);
    }
    return CW_OK;
}

// ---- entropy of the teacher-forced positions (include/crisperwhisper.h) ----------------------------------------------------------
int32_t cw_set_score_entropy(cw_ctx* c, int32_t on) {
    c->sc_ent_on = on != 0;
    c->sc_ent_nrows = 0;                         // what an earlier call stored is not handed out under a new setting
    if (!c->sc_ent_on) c->sc_ents.clear();
    return CW_OK;
}

int32_t cw_get_score_entropy(cw_ctx* c, float* out, int32_t rows, int32_t ids_stride) {
    if (!c->sc_ent_on) return fail(c, CW_ERR_STATE, "score entropy is off (cw_set_score_entropy)");
    if (!out || rows < 1 || ids_stride < 1) return fail(c, CW_ERR_INVALID, "get_score_entropy: bad arguments");
    if (rows > c->sc_ent_nrows || ids_stride != c->sc_ent_stride)
        return fail(c, CW_ERR_STATE, "get_score_entropy: asked %d rows of stride %d, the last scoring call stored %d of stride %d", rows,
                    ids_stride, c->sc_ent_nrows, c->sc_ent_stride);
    memcpy(out, c->sc_ents.data(), (size_t)rows * ids_stride * 4);
    return CW_OK;
}

int32_t cw_align_matrix(cw_ctx* c, const float* attn, int32_t B, int32_t Ha, int32_t N, int32_t M, const int32_t* n_cols,
                        int32_t width, float* mat_out) {
    float *dw = nullptr, *dmean = nullptr, *dstd = nullptr, *dmat = nullptr; int* dn = nullptr;
    size_t nw = (size_t)B * Ha * N * M;
    HIPCHK(c, hipMalloc((void**)&dw, nw * 4)); HIPCHK(c, hipMalloc((void**)&dmean, (size_t)B * Ha * M * 4));
    HIPCHK(c, hipMalloc((void**)&dstd, (size_t)B * Ha * M * 4)); HIPCHK(c, hipMalloc((void**)&dmat, (size_t)B * N * M * 4));
    HIPCHK(c, hipMalloc((void**)&dn, B * 4));
    HIPCHK(c, hipMemcpy(dw, attn, nw * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dn, n_cols, B * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(dmat, 0, (size_t)B * N * M * 4));
    int r = run_alignment(c, dw, B, Ha, N, M, 0, N, dn, width, dmean, dstd, dmat);
    if (r == CW_OK) {
        hipError_t e = hipStreamSynchronize(c->st);
        if (e == hipSuccess) e = hipMemcpy(mat_out, dmat, (size_t)B * N * M * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = fail(c, CW_ERR_HIP, "align_matrix: %s", hipGetErrorString(e));
    }
    hipFree(dw); hipFree(dmean); hipFree(dstd); hipFree(dmat); hipFree(dn);
    return r;
}

int32_t cw_dtw(cw_ctx* c, const float* mat, int32_t N, int32_t M, int32_t* text_idx, int32_t* time_idx, int32_t* path_len) {
    if (N < 1 || N > 512 || M < 1) return fail(c, CW_ERR_INVALID, "dtw: N=%d M=%d unsupported", N, M);
    float* dmat = nullptr; unsigned char* dtr = nullptr; int *dfc = nullptr, *dpt = nullptr, *dpj = nullptr, *dpl = nullptr, *dn = nullptr;
    HIPCHK(c, hipMalloc((void**)&dmat, (size_t)N * M * 4)); HIPCHK(c, hipMalloc((void**)&dtr, (size_t)N * M));
    HIPCHK(c, hipMalloc((void**)&dfc, N * 4)); HIPCHK(c, hipMalloc((void**)&dpt, (size_t)(N + M + 2) * 4));
    HIPCHK(c, hipMalloc((void**)&dpj, (size_t)(N + M + 2) * 4)); HIPCHK(c, hipMalloc((void**)&dpl, 4)); HIPCHK(c, hipMalloc((void**)&dn, 4));
    HIPCHK(c, hipMemcpy(dmat, mat, (size_t)N * M * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dn, &M, 4, hipMemcpyHostToDevice));
    float* dskew = nullptr;
    HIPCHK(c, hipMalloc((void**)&dskew, cw_dtw_skew_floats(1, N, M) * 4));
    int r = cw_launch_dtw(dmat, 1, N, M, dn, dtr, dfc, dpt, dpj, dpl, c->st, c->sw.dtw_block ? nullptr : dskew);
    if (r == CW_OK) {
        std::vector<int> pt(N + M + 2), pj(N + M + 2);
        int n = 0;
        hipError_t e = hipStreamSynchronize(c->st);
        if (e == hipSuccess) e = hipMemcpy(&n, dpl, 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(pt.data(), dpt, pt.size() * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(pj.data(), dpj, pj.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = fail(c, CW_ERR_HIP, "dtw: %s", hipGetErrorString(e));
        else {
            for (int k = 0; k < n; ++k) { text_idx[k] = pt[n - 1 - k]; time_idx[k] = pj[n - 1 - k]; }
            *path_len = n;
        }
    } else {
        fail(c, r, "dtw launch rejected N=%d", N);
    }
    hipFree(dmat); hipFree(dtr); hipFree(dfc); hipFree(dpt); hipFree(dpj); hipFree(dpl); hipFree(dn); hipFree(dskew);
    return r;
}

int32_t cw_adjust_pauses(cw_ctx* c, double* start, double* end, int32_t W, double thr) {
    if (W <= 0) return CW_OK;
    if (W > c->pause_cap) {   // grow the persistent scratch (start/end in, start/end out)
        int cap = 1024;
        while (cap < W) cap *= 2;
        CWCHK(c, dmalloc(c, &c->d_pause, (size_t)4 * cap * 8, false));
        c->pause_cap = cap;
    }
    double* ds = c->d_pause;              // [in W | out W]
    double* de = c->d_pause + 2 * (size_t)c->pause_cap;
    HIPCHK(c, hipMemcpyAsync(ds, start, (size_t)W * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(de, end, (size_t)W * 8, hipMemcpyHostToDevice, c->st));
    CWCHK(c, cw_launch_pauses(ds, de, W, thr, c->st));
    HIPCHK(c, hipMemcpyAsync(start, ds + W, (size_t)W * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(end, de + W, (size_t)W * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// audio ingest
// ------------------------------------------------------------------------------------------------
static int igcd(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

int64_t cw_resampled_length(int64_t n, int32_t sr_in, int32_t sr_out) {
    if (n < 0 || sr_in <= 0 || sr_out <= 0) return -1;
    const int g = igcd(sr_in, sr_out);
    const int64_t o = sr_in / g, w = sr_out / g;
    return (n * w + o - 1) / o;
}

// torchaudio's _get_sinc_resample_kernel with dtype=None (f64 arithmetic, rounded to f32 at the end): K[p][j],
// p in 0..new-1, j in 0..2*width+orig-1
// false: the rate pair needs an unreasonably large polyphase table (coprime rates in the MHz range, corrupted headers)
static bool resample_taps(int sr_in, int sr_out, std::vector<float>& K, int& orig, int& nw, int& width) {
    const int g = igcd(sr_in, sr_out);
    orig = sr_in / g; nw = sr_out / g;
    const double lpw = 6.0, rolloff = 0.99;
    const double base_freq = (double)(orig < nw ? orig : nw) * rolloff;
    const double w = ceil(lpw * orig / base_freq);
    if (w > 1e6 || ((double)nw * (2.0 * w + orig)) > 536870912.0) return false;   // 512 M taps = 2 GB
    width = (int)w;
    const int n_taps = 2 * width + orig;
    K.assign((size_t)nw * n_taps, 0.f);
    const double scale = base_freq / orig;
    for (int p = 0; p < nw; ++p)
        for (int j = 0; j < n_taps; ++j) {
            double t = (double)(-p) / nw + (double)(j - width) / orig;
            t *= base_freq;
            t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
            const double c = cos(t * M_PI / lpw / 2.0);
            const double window = c * c;
            t *= M_PI;
            const double sinc = t == 0.0 ? 1.0 : sin(t) / t;
            K[(size_t)p * n_taps + j] = (float)(sinc * window * scale);
        }
    return true;
}

int32_t cw_resample_taps(int32_t sr_in, int32_t sr_out, float* taps, int32_t cap, int32_t* orig, int32_t* nw,
                         int32_t* width) {
    if (sr_in <= 0 || sr_out <= 0) return CW_ERR_INVALID;
    std::vector<float> K;
    int o = 0, w = 0, wd = 0;
    if (!resample_taps(sr_in, sr_out, K, o, w, wd)) return CW_ERR_INVALID;
    if (orig) *orig = o;
    if (nw) *nw = w;
    if (width) *width = wd;
    if (taps) {
        if ((size_t)cap < K.size()) return CW_ERR_INVALID;
        memcpy(taps, K.data(), K.size() * 4);
    }
    return CW_OK;
}

int32_t cw_ingest(cw_ctx* c, const void* raw, int32_t fmt, int32_t channels, int64_t n_frames, int32_t sr_in,
                  int32_t sr_out, int32_t normalise, float* out) {
    static const int bytes_of[] = {1, 2, 3, 4, 4, 8};
    if (fmt < 0 || fmt > CW_PCM_F64) return fail(c, CW_ERR_INVALID, "unknown sample format %d", fmt);
    if (channels < 1 || n_frames < 1 || sr_in <= 0 || sr_out <= 0)
        return fail(c, CW_ERR_INVALID, "bad audio geometry (channels=%d frames=%lld %d->%d Hz)", channels, (long long)n_frames, sr_in, sr_out);
    const size_t raw_bytes = (size_t)n_frames * channels * bytes_of[fmt];
    const int64_t n_out = cw_resampled_length(n_frames, sr_in, sr_out);
    void* d_raw = nullptr; float *d_mono = nullptr, *d_out = nullptr, *d_taps = nullptr; double* d_acc = nullptr;
    int rc = CW_OK;
    auto cleanup = [&]() { hipFree(d_raw); hipFree(d_mono); hipFree(d_out); hipFree(d_taps); hipFree(d_acc); };
#define ING(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { cleanup(); return fail(c, CW_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } } while (0)
    ING(hipMalloc(&d_raw, raw_bytes));
    ING(hipMalloc((void**)&d_mono, (size_t)n_frames * 4));
    ING(hipMemcpyAsync(d_raw, raw, raw_bytes, hipMemcpyHostToDevice, c->st));
    rc = cw_launch_pcm_to_mono(d_raw, fmt, channels, n_frames, d_mono, c->st);
    if (rc == CW_OK && normalise) {
        ING(hipMalloc((void**)&d_acc, 16));
        rc = cw_launch_normalise(d_mono, n_frames, d_acc, c->st);
    }
    const float* d_res = d_mono;
    if (rc == CW_OK && sr_in != sr_out) {                       // F.resample returns its input when the rates agree
        std::vector<float> K, Kt;
        int orig = 0, nw = 0, width = 0;
        if (!resample_taps(sr_in, sr_out, K, orig, nw, width)) {
            cleanup();
            return fail(c, CW_ERR_INVALID, "unsupported sampling-rate pair %d -> %d Hz (polyphase table too large)", sr_in, sr_out);
        }
        const int n_taps = 2 * width + orig;
        Kt.resize(K.size());
        for (int p = 0; p < nw; ++p) for (int j = 0; j < n_taps; ++j) Kt[(size_t)j * nw + p] = K[(size_t)p * n_taps + j];
        ING(hipMalloc((void**)&d_taps, Kt.size() * 4));
        ING(hipMalloc((void**)&d_out, (size_t)n_out * 4));
        ING(hipMemcpyAsync(d_taps, Kt.data(), Kt.size() * 4, hipMemcpyHostToDevice, c->st));
        ING(hipStreamSynchronize(c->st));                       // Kt is a local
        rc = cw_launch_resample(d_mono, n_frames, d_taps, orig, nw, width, n_out, d_out, c->st);
        d_res = d_out;
    }
    if (rc != CW_OK) { cleanup(); return fail(c, rc, "cw_ingest: launch rejected"); }
    ING(hipMemcpyAsync(out, d_res, (size_t)n_out * 4, hipMemcpyDeviceToHost, c->st));
    ING(hipStreamSynchronize(c->st));
#undef ING
    cleanup();
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// options
// ------------------------------------------------------------------------------------------------
// e4m3 copies of the encoder qkv / fc1 / fc2 and decoder cross-K/V weights from the resident 16-bit weights (row-wise scales)
static int enc8_quantise(cw_ctx* c) {
    const int D = c->d.d_model, F = c->d.ffn_dim;
    for (auto& L : c->enc) {
        CWCHK(c, KD(c, cw_launch_quant_rows_fp8, L.wqkv, 3 * D, D, L.wqkv8, L.sqkv, c->st));
        CWCHK(c, KD(c, cw_launch_quant_rows_fp8, L.w1, F, D, L.w18, L.s1, c->st));
        CWCHK(c, KD(c, cw_launch_quant_rows_fp8, L.w2, D, F, L.w28, L.s2, c->st));
    }
    for (auto& L : c->dec) CWCHK(c, KD(c, cw_launch_quant_rows_fp8, L.wkv_c, 2 * D, D, L.wkv_c8, L.skv_c, c->st));
    KCHK(c);
    c->enc8_stale = false;
    return CW_OK;
}

int32_t cw_set_option(cw_ctx* c, const char* name, int32_t value) {
    if (!name) return fail(c, CW_ERR_INVALID, "cw_set_option: null option name");
    if (!strcmp(name, "prompt_prefix")) {    // the coming decoder inputs start with this many prompt_ids (0: none)
        if (value < 0 || value >= c->d.max_target_positions) return fail(c, CW_ERR_INVALID, "prompt_prefix=%d out of range", value);
        c->pf_prefix = value;
        return CW_OK;
    }
    if (!strcmp(name, "prompt_prefill")) {   // 0: prompt positions through the per-position decoder step (A/B of the prefill)
        c->prompt_prefill = value != 0;
        return CW_OK;
    }
    if (!strcmp(name, "align_prefill")) {    // 0: cw_align_tokens runs its forward through the per-position decoder step (A/B)
        c->align_prefill = value != 0;
        return CW_OK;
    }
    if (!strcmp(name, "score_prefill")) {    // 0: cw_score_tokens runs its forward through the per-position decoder step (A/B)
        c->score_prefill = value != 0;
        return CW_OK;
    }
    if (!strcmp(name, "cross_kv_fp8")) {
        if (!value) { c->kv8 = false; return CW_OK; }
        if (!c->bf16) return fail(c, CW_ERR_INVALID, "cross_kv_fp8 needs the bf16 engine (the f32 engine is the parity mode)");
        if (!c->dec[0].ck8) {
            const size_t n = (size_t)c->Bm * c->d.n_heads * CW_N_CTX * 64;
            const size_t nv = (size_t)c->Bm * cw_bf16::cw_kv8_v_bytes(c->d.n_heads, CW_N_CTX);   // V: fragment-major for the fp8 matrix cores
            for (auto& L : c->dec) {
                CWCHK(c, dmalloc(c, &L.ck8, n, false)); CWCHK(c, dmalloc(c, &L.cv8, nv, false));
                CWCHK(c, dmalloc(c, &L.kvs, (size_t)c->Bm * c->d.n_heads * 2 * 4));
            }
        }
        c->kv8 = true;
        c->nb_encoded = 0;                                   // windows must be re-encoded to fill the fp8 cache
        drop_step_graphs(c);   // graphs hold the kernel choice
        return CW_OK;
    }
    if (!strcmp(name, "encoder_gemm_fp8")) {
        if (!value) { c->enc8 = false; c->enc8_mask = 0; c->nb_encoded = 0; return CW_OK; }
        if (!c->bf16) return fail(c, CW_ERR_INVALID, "encoder_gemm_fp8 needs a 16-bit engine (the f32 engine is the parity mode)");
        const int D = c->d.d_model, F = c->d.ffn_dim;
        if (D % 256 != 0 || F % 256 != 0 || D > 2048) return fail(c, CW_ERR_INVALID, "encoder_gemm_fp8: d_model / ffn_dim must be multiples of 256 (d_model <= 2048)");
        CWCHK(c, cw_check_weights(c));                       // the e4m3 copies are made from the resident 16-bit weights
        if (!c->h8) {
            const size_t MR = (size_t)c->Bm * CW_N_CTX;
            CWCHK(c, dmalloc(c, &c->h8, MR * D, false)); CWCHK(c, dmalloc(c, &c->mid8, MR * F, false));
            CWCHK(c, dmalloc(c, &c->sa8, MR * 4)); CWCHK(c, dmalloc(c, &c->smid8, MR * 4));
            for (auto& L : c->enc) {
                CWCHK(c, dmalloc(c, &L.wqkv8, (size_t)3 * D * D, false)); CWCHK(c, dmalloc(c, &L.sqkv, (size_t)3 * D * 4));
                CWCHK(c, dmalloc(c, &L.w18, (size_t)F * D, false)); CWCHK(c, dmalloc(c, &L.s1, (size_t)F * 4));
                CWCHK(c, dmalloc(c, &L.w28, (size_t)D * F, false)); CWCHK(c, dmalloc(c, &L.s2, (size_t)D * 4));
            }
            for (auto& L : c->dec) { CWCHK(c, dmalloc(c, &L.wkv_c8, (size_t)2 * D * D, false)); CWCHK(c, dmalloc(c, &L.skv_c, (size_t)2 * D * 4)); }
        }
        CWCHK(c, enc8_quantise(c));
        c->enc8 = true;
        c->enc8_mask = value >= 16 ? ((value - 16) & 15) : 15;   // 1 = every GEMM; 16 + mask = a subset (tools/fp8_sweep.py)
        c->nb_encoded = 0;                                   // windows must be re-encoded
        return CW_OK;
    }
    if (!strcmp(name, "test_epoch_forwards")) {   // test hook: pretend this many decoder forwards have run since the granule epoch last started (epoch_hygiene)
        c->forwards_since_reset = (long long)value;
        return CW_OK;
    }
    if (!strcmp(name, "handoff_fail_pos")) {   // test hook: the in-launch hand-off of qkv_self_kernel gives up at this decoder position (-1: never)
        c->fail_pos = value;
        drop_step_graphs(c);   // kernel arguments are baked into the graphs
        return CW_OK;
    }
    // the context's own switches under their names in switches.def (A/B, differential tests); a flag is set by value != 0
    for (const char* sw_name : {"no_wnt", "no_xq_in_qkv", "rows_ln", "skinny"}) {
        if (strcmp(name, sw_name)) continue;
        const cw_sw::Row* r = cw_sw::find(name);
#ifndef CW_EXPERIMENTS
        if (r->rejected && value != 0)
            return fail(c, CW_ERR_INVALID, "option %s selects a measured-and-rejected kernel variant that is not in this build (make EXTRA=-DCW_EXPERIMENTS)", name);
#endif
        r->set(c->sw, value);
        drop_step_graphs(c);   // graphs hold the kernel choice
        return CW_OK;
    }
    return fail(c, CW_ERR_INVALID, "unknown option %s", name);
}

// 1 when the library was built with -DCW_EXPERIMENTS (the measured-and-rejected kernel variants and their A/B switches:
// DESIGN.md "A/B switches"); the differential tests of those variants skip otherwise.
int32_t cw_has_experiments(void) {
#ifdef CW_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

}  // extern "C"
