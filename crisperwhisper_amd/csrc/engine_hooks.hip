// Test and bench hooks of the C ABI (include/crisperwhisper.h: cw_test_*, cw_time_* and the measurement calls): each drives kernels
// or engine helpers on caller-supplied operands.  The product paths are in engine.hip.
#include "engine_internal.h"

extern "C" {

// ------------------------------------------------------------------------------------------------
// kernel-level test hooks
// ------------------------------------------------------------------------------------------------
static int g_test_no_wnt = 0;      // cw_test_gemv_epi / cw_test_gemv_stack with default-policy weight loads (option "no_wnt"; a context's own: cw_set_option)
static int g_test_cross_fp8 = 0;   // cw_test_cross_attention through the e4m3 cache (option "cross_test_fp8")
static int g_test_attn_poison_qpad = 0;   // cw_test_attention: Q rows S .. S_pad-1 hold NaN instead of zeros (option "attn_poison_qpad")
int32_t cw_test_set_option(const char* name, int32_t value) {
    if (!strcmp(name, "no_wnt")) { g_test_no_wnt = value; return CW_OK; }
    if (!strcmp(name, "cross_test_fp8")) { g_test_cross_fp8 = value; return CW_OK; }
    if (!strcmp(name, "attn_poison_qpad")) { g_test_attn_poison_qpad = value; return CW_OK; }
    if (!strcmp(name, "gemm_gm")) {
#ifndef CW_EXPERIMENTS
        return CW_ERR_INVALID;
#endif
        cw_bf16::cw_gemm_set_gm(value); cw_f16::cw_gemm_set_gm(value); return CW_OK;
    }
    return cw_sw::set_test_option(name, value) ? CW_OK : CW_ERR_INVALID;   // the launcher switches: the process table
}

// cw_test_mel_stages: what the last cw_mel / cw_mel_resident left in d_logspec, d_gmax and d_feats_tm for items 0 .. B-1 (copies
// only).  The clip maximum is decoded here exactly as mel.hip: ordered_to_float decodes it.
int32_t cw_test_mel_stages(cw_ctx* c, int32_t B, float* logspec, float* gmax, float* feats_tm) {
    if (B < 1 || B > c->Bm) return fail(c, CW_ERR_INVALID, "test_mel_stages: B=%d out of range (max_batch %d)", B, c->Bm);
    const size_t n = (size_t)B * CW_N_FRAMES * c->d.n_mels;
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (logspec) HIPCHK(c, hipMemcpy(logspec, c->d_logspec, n * 4, hipMemcpyDeviceToHost));
    if (gmax) {
        std::vector<unsigned int> u(B);
        HIPCHK(c, hipMemcpy(u.data(), c->d_gmax, (size_t)B * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            const unsigned int bits = (u[b] & 0x80000000u) ? (u[b] & 0x7fffffffu) : ~u[b];
            memcpy(gmax + b, &bits, 4);
        }
    }
    if (feats_tm) CWCHK(c, download_T(c, c->d_feats_tm, 0, feats_tm, n));
    return CW_OK;
}

int32_t cw_test_gemm(cw_ctx* c, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias,
                     int32_t gelu, float* out) {
    void *dA = nullptr, *dW = nullptr, *dO = nullptr; float* dB = nullptr;
    const size_t e = c->esz;
    DevScope mem;
    HIPCHK(c, mem.get(&dA, (size_t)M * K * e)); HIPCHK(c, mem.get(&dW, (size_t)N * K * e));
    HIPCHK(c, mem.get(&dO, (size_t)M * N * e)); HIPCHK(c, mem.get(&dB, (size_t)N * 4));
    CWCHK(c, upload_T(c, dA, 0, A, (size_t)M * K)); CWCHK(c, upload_T(c, dW, 0, W, (size_t)N * K));
    if (bias) HIPCHK(c, hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    AParams ap{dA, K, 0, 0, 0, 0, nullptr, nullptr};
    EpiParams ep = epi0(); ep.out = dO; ep.bias = bias ? dB : nullptr; ep.ldo = N;
    int r = KD(c, cw_launch_gemm, c->bf16, gelu ? EPI_GELU : EPI_STORE, ap, dW, M, N, K, ep, c->st);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_gemm: %s", hipGetErrorString(er)); }
    if (const int reps = cw_sw::cw_switches().test_gemm_reps) {   // kernel A/B timing for the profiles (stderr only)
        hipEvent_t e0, e1;
        if (r == CW_OK && reps > 0 && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            hipEventRecord(e0, c->st);
            for (int i = 0; i < reps && r == CW_OK; ++i) r = KD(c, cw_launch_gemm, c->bf16, gelu ? EPI_GELU : EPI_STORE, ap, dW, M, N, K, ep, c->st);
            hipEventRecord(e1, c->st);
            hipEventSynchronize(e1);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            const double us = 1e3 * ms / reps;
            fprintf(stderr, "[cw_test_gemm] M=%d N=%d K=%d gelu=%d: %.2f us/launch, %.1f TFLOP/s\n", M, N, K, gelu, us, 2.0 * M * N * K / us * 1e-6);
            hipEventDestroy(e0); hipEventDestroy(e1);
        }
    }
    if (r == CW_OK) r = download_T(c, dO, 0, out, (size_t)M * N);
    return r;
}

// Prefill kernels against a host reference (prefill.hip).  cw_test_prefill_gemm: A [M][K] and W [N][K] are rounded to the engine's
// 16-bit type, W is packed fragment-major (wfrag_pack_kernel) and prefill_gemm_kernel runs with epilogue `mode`: 0 = store,
// 2 = f32 residual (out holds the residual on entry and resid + A W^T + bias on return), 3 = erf GELU; 16-bit outputs are returned
// as f32.  16-bit engines; K % 32 == 0, N % 16 == 0.
int32_t cw_test_prefill_gemm(cw_ctx* c, int32_t mode, int32_t M, int32_t N, int32_t K, const float* A, const float* W,
                             const float* bias, float* out) {
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_prefill_gemm: 16-bit engines only");
    if ((mode != PF_STORE && mode != PF_RESID && mode != PF_GELU) || M < 1 || N < 16 || N % 16 || K < 32 || K % 32)
        return fail(c, CW_ERR_INVALID, "test_prefill_gemm: bad arguments");
    void *dA = nullptr, *dW = nullptr, *dWp = nullptr, *dO = nullptr; float* dB = nullptr;
    const size_t e = c->esz;
    int r = CW_OK;
    DevScope mem;
    if (mem.get(&dA, (size_t)M * K * e) != hipSuccess || mem.get(&dW, (size_t)N * K * e) != hipSuccess ||
        mem.get(&dWp, KD(c, cw_wfrag_elems, N, K) * e) != hipSuccess || mem.get(&dO, (size_t)M * N * 4) != hipSuccess ||
        mem.get(&dB, (size_t)N * 4) != hipSuccess) r = fail(c, CW_ERR_NOMEM, "test_prefill_gemm: hipMalloc failed");
    if (r == CW_OK) r = upload_T(c, dA, 0, A, (size_t)M * K);
    if (r == CW_OK) r = upload_T(c, dW, 0, W, (size_t)N * K);
    if (r == CW_OK && bias && hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice) != hipSuccess) r = fail(c, CW_ERR_HIP, "test_prefill_gemm: copy");
    if (r == CW_OK && mode == PF_RESID && hipMemcpy(dO, out, (size_t)M * N * 4, hipMemcpyHostToDevice) != hipSuccess) r = fail(c, CW_ERR_HIP, "test_prefill_gemm: copy");
    if (r == CW_OK) r = KD(c, cw_launch_wfrag_pack, dW, N, K, dWp, c->st);
    PrefillEpi ep;
    memset(&ep, 0, sizeof(ep));
    ep.mode = mode; ep.bias = bias ? dB : nullptr;
    if (mode == PF_RESID) ep.x = (float*)dO; else ep.out = dO;
    if (r == CW_OK) r = KD(c, cw_launch_prefill_gemm, dA, dWp, ep, M, N, K, c->st);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_prefill_gemm: %s", hipGetErrorString(er)); }
    if (r == CW_OK) {
        if (mode == PF_RESID) { if (hipMemcpy(out, dO, (size_t)M * N * 4, hipMemcpyDeviceToHost) != hipSuccess) r = fail(c, CW_ERR_HIP, "test_prefill_gemm: copy"); }
        else r = download_T(c, dO, 0, out, (size_t)M * N);
    }
    return r;
}

// cw_test_score_head: the scoring head (score.hip) on its own.  x [M][D] f32 residual rows, ln_g / ln_b [D], embed [V][D] (rounded
// to the engine's 16-bit type and packed fragment-major), targets [M] -> logprob / top_id / top_logprob [M].  16-bit engines;
// D % 32 == 0.  Sizes are validated on the host before anything is allocated or launched.
// stop_logprob non-null (cw_test_score_head_stop): the STOP form over S = {eos} + {n >= timestamp_begin} instead.
static int test_score_head(cw_ctx* c, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                           const float* embed, const int32_t* targets, float* logprob, int32_t* top_id, float* top_logprob,
                           int eos, int timestamp_begin, float* stop_logprob, int k = 0, int32_t* alt_id = nullptr,
                           float* alt_logprob = nullptr, float* logits_out = nullptr, float* entropy = nullptr) {
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_score_head: 16-bit engines only");
    if (k < 0 || k > CW_TOP_LOGPROBS_MAX || (k > 0 && (!alt_id || !alt_logprob)) || (k == 0 && !entropy && logits_out))
        return fail(c, CW_ERR_INVALID, "test_score_head: k=%d outside 1 .. %d or a null alt_id / alt_logprob", k, CW_TOP_LOGPROBS_MAX);
    if (M < 1 || M > (1 << 16) || D < 32 || D % 32 || D > 8192 || V < 1 || V > (1 << 20) || !x || !ln_g || !ln_b || !embed || !targets ||
        !logprob || !top_id || !top_logprob) return fail(c, CW_ERR_INVALID, "test_score_head: bad arguments");
    for (int m = 0; m < M; ++m)
        if (targets[m] < 0 || targets[m] >= V) return fail(c, CW_ERR_INVALID, "test_score_head: target %d of row %d outside 0 .. %d", targets[m], m, V - 1);
    const size_t e = c->esz;
    const int ns = KD(c, cw_score_head_splits, M, V, nullptr);
    float *dx = nullptr, *dg = nullptr, *db = nullptr, *dlog = nullptr;
    int* dt = nullptr;
    void *dA = nullptr, *dW = nullptr, *dWp = nullptr;
    ScoreHeadOut o{};
    o.eos = eos; o.ts_begin = timestamp_begin; o.k = k;
    DevScope mem;
    bool ok = true;
    auto get = [&](auto** p, size_t bytes) { ok = ok && mem.get(p, bytes) == hipSuccess; };
    // TOPK form: the per-split lists and alt_id / alt_logprob [M][CW_TOP_LOGPROBS_MAX], each with 8 guard rows behind row M - 1,
    // filled with 0x5a: a write there is CW_ERR_STATE; f32 logits [M][V]
    const size_t tp_row = (size_t)ns * CW_TOP_LOGPROBS_MAX * sizeof(ScoreTopPart), alt_row = (size_t)CW_TOP_LOGPROBS_MAX * 4;
    if (k > 0) {
        get(&o.tpart, (size_t)(M + 8) * tp_row); get(&o.alt_id, (size_t)(M + 8) * alt_row); get(&o.alt_logprob, (size_t)(M + 8) * alt_row);
    }
    if (logits_out) get(&dlog, (size_t)M * V * 4);
    // ENT form: the per-split centred sums and entropy [M], with 8 guard rows each as above
    if (entropy) { get(&o.epart, (size_t)(M + 8) * ns * 4); get(&o.entropy, (size_t)(M + 8) * 4); }
    if (stop_logprob) { get(&o.spart, (size_t)M * ns * sizeof(ScoreStopPart)); get(&o.stop_logprob, (size_t)M * 4); }
    get(&dx, (size_t)M * D * 4); get(&dg, (size_t)D * 4); get(&db, (size_t)D * 4); get(&o.logprob, (size_t)M * 4);
    get(&o.top_logprob, (size_t)M * 4); get(&dt, (size_t)M * 4); get(&o.top_id, (size_t)M * 4); get(&dA, (size_t)M * D * e);
    get(&dW, (size_t)V * D * e); get(&dWp, KD(c, cw_wfrag_elems, V, D) * e); get(&o.part, (size_t)M * ns * sizeof(ScorePart));
    if (!ok) return fail(c, CW_ERR_NOMEM, "test_score_head: hipMalloc failed");
    if (k > 0 && (hipMemset(o.tpart, 0x5a, (size_t)(M + 8) * tp_row) != hipSuccess || hipMemset(o.alt_id, 0x5a, (size_t)(M + 8) * alt_row) != hipSuccess ||
                  hipMemset(o.alt_logprob, 0x5a, (size_t)(M + 8) * alt_row) != hipSuccess)) return fail(c, CW_ERR_HIP, "test_score_head: memset");
    if (entropy && (hipMemset(o.epart, 0x5a, (size_t)(M + 8) * ns * 4) != hipSuccess || hipMemset(o.entropy, 0x5a, (size_t)(M + 8) * 4) != hipSuccess))
        return fail(c, CW_ERR_HIP, "test_score_head: memset");
    if (hipMemcpy(dx, x, (size_t)M * D * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dg, ln_g, (size_t)D * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(db, ln_b, (size_t)D * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dt, targets, (size_t)M * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(c, CW_ERR_HIP, "test_score_head: copy");
    int r = upload_T(c, dW, 0, embed, (size_t)V * D);
    if (r == CW_OK) r = KD(c, cw_launch_wfrag_pack, dW, V, D, dWp, c->st);
    if (r == CW_OK) r = KD(c, cw_launch_score_ln, dx, nullptr, dg, db, dA, M, D, c->st);
    if (r == CW_OK) r = KD(c, cw_launch_score_head, dA, dWp, dt, M, V, D, o, c->st);
    if (r == CW_OK && logits_out) r = KD(c, cw_launch_score_head_store, dA, dWp, dt, dlog, V, M, V, D, c->st);
    if (r != CW_OK) return r;
    if (hipError_t er = hipStreamSynchronize(c->st)) return fail(c, CW_ERR_HIP, "test_score_head: %s", hipGetErrorString(er));
    if (k > 0) {
        std::vector<unsigned char> gd(8 * tp_row), ga(8 * alt_row), gl(8 * alt_row);
        if (hipMemcpy(gd.data(), (char*)o.tpart + (size_t)M * tp_row, gd.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ga.data(), (char*)o.alt_id + (size_t)M * alt_row, ga.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(gl.data(), (char*)o.alt_logprob + (size_t)M * alt_row, gl.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, CW_ERR_HIP, "test_score_head: copy");
        for (const auto* gv : {&gd, &ga, &gl})
            for (unsigned char b : *gv)
                if (b != 0x5a) return fail(c, CW_ERR_STATE, "test_score_head: a row behind M = %d was written", M);
        if (hipMemcpy(alt_id, o.alt_id, (size_t)M * alt_row, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(alt_logprob, o.alt_logprob, (size_t)M * alt_row, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, CW_ERR_HIP, "test_score_head: copy");
    }
    if (logits_out && hipMemcpy(logits_out, dlog, (size_t)M * V * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(c, CW_ERR_HIP, "test_score_head: copy");
    if (entropy) {
        std::vector<unsigned char> gp((size_t)8 * ns * 4), ge(8 * 4);
        if (hipMemcpy(gp.data(), (char*)o.epart + (size_t)M * ns * 4, gp.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ge.data(), (char*)o.entropy + (size_t)M * 4, ge.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(entropy, o.entropy, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, CW_ERR_HIP, "test_score_head: copy");
        for (const auto* gv : {&gp, &ge})
            for (unsigned char b : *gv)
                if (b != 0x5a) return fail(c, CW_ERR_STATE, "test_score_head: an entropy row behind M = %d was written", M);
    }
    if ((stop_logprob && hipMemcpy(stop_logprob, o.stop_logprob, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        hipMemcpy(logprob, o.logprob, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(top_id, o.top_id, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(top_logprob, o.top_logprob, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, CW_ERR_HIP, "test_score_head: copy");
    return CW_OK;
}

int32_t cw_test_score_head(cw_ctx* c, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                           const float* embed, const int32_t* targets, float* logprob, int32_t* top_id, float* top_logprob) {
    return test_score_head(c, M, D, V, x, ln_g, ln_b, embed, targets, logprob, top_id, top_logprob, 0, 0, nullptr);
}

int32_t cw_test_score_head_stop(cw_ctx* c, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                                const float* embed, const int32_t* targets, int32_t eos, int32_t timestamp_begin, float* logprob,
                                int32_t* top_id, float* top_logprob, float* stop_logprob) {
    if (!stop_logprob || eos < 0 || eos >= V || timestamp_begin < 0 || timestamp_begin > V)
        return fail(c, CW_ERR_INVALID, "test_score_head_stop: eos=%d inside 0 .. %d, timestamp_begin=%d inside 0 .. %d and stop_logprob are needed",
                    eos, V - 1, timestamp_begin, V);
    return test_score_head(c, M, D, V, x, ln_g, ln_b, embed, targets, logprob, top_id, top_logprob, eos, timestamp_begin, stop_logprob);
}

// cw_test_score_head_top / _stop_top: the TOPK forms of the head.  alt_id / alt_logprob [M][CW_TOP_LOGPROBS_MAX]; logits_out
// non-null: the same operands once more through the STORE form into [M][V] -- the same MFMA sequence, so the very accumulators
// the fused form selected from.
int32_t cw_test_score_head_top(cw_ctx* c, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                               const float* embed, const int32_t* targets, int32_t k, float* logprob, int32_t* top_id, float* top_logprob,
                               int32_t* alt_id, float* alt_logprob, float* logits_out) {
    if (k < 1) return fail(c, CW_ERR_INVALID, "test_score_head_top: k=%d outside 1 .. %d", k, CW_TOP_LOGPROBS_MAX);
    return test_score_head(c, M, D, V, x, ln_g, ln_b, embed, targets, logprob, top_id, top_logprob, 0, 0, nullptr, k, alt_id, alt_logprob,
                           logits_out);
}

int32_t cw_test_score_head_stop_top(cw_ctx* c, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                                    const float* embed, const int32_t* targets, int32_t eos, int32_t timestamp_begin, int32_t k,
                                    float* logprob, int32_t* top_id, float* top_logprob, float* stop_logprob, int32_t* alt_id,
                                    float* alt_logprob, float* logits_out) {
    if (k < 1) return fail(c, CW_ERR_INVALID, "test_score_head_stop_top: k=%d outside 1 .. %d", k, CW_TOP_LOGPROBS_MAX);
    if (!stop_logprob || eos < 0 || eos >= V || timestamp_begin < 0 || timestamp_begin > V)
        return fail(c, CW_ERR_INVALID, "test_score_head_stop_top: eos=%d inside 0 .. %d, timestamp_begin=%d inside 0 .. %d and stop_logprob are needed",
                    eos, V - 1, timestamp_begin, V);
    return test_score_head(c, M, D, V, x, ln_g, ln_b, embed, targets, logprob, top_id, top_logprob, eos, timestamp_begin, stop_logprob, k,
                           alt_id, alt_logprob, logits_out);
}

// cw_test_score_head_entropy: the ENT forms of the head, alone (stop_logprob NULL, k = 0) or joined with STOP (stop_logprob non-null)
// and / or TOPK (k > 0; alt_id / alt_logprob as above).  entropy [M]; logits_out as above.
int32_t cw_test_score_head_entropy(cw_ctx* c, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                                   const float* embed, const int32_t* targets, int32_t eos, int32_t timestamp_begin, int32_t k,
                                   float* logprob, int32_t* top_id, float* top_logprob, float* stop_logprob, int32_t* alt_id,
                                   float* alt_logprob, float* entropy, float* logits_out) {
    if (!entropy) return fail(c, CW_ERR_INVALID, "test_score_head_entropy: null entropy");
    if (stop_logprob && (eos < 0 || eos >= V || timestamp_begin < 0 || timestamp_begin > V))
        return fail(c, CW_ERR_INVALID, "test_score_head_entropy: eos=%d inside 0 .. %d and timestamp_begin=%d inside 0 .. %d are needed", eos,
                    V - 1, timestamp_begin, V);
    return test_score_head(c, M, D, V, x, ln_g, ln_b, embed, targets, logprob, top_id, top_logprob, stop_logprob ? eos : 0,
                           stop_logprob ? timestamp_begin : 0, stop_logprob, k, alt_id, alt_logprob, logits_out, entropy);
}

// the loop path's row kernel on caller-supplied f32 logits [rows][ldv], any engine: k = 0 without the TOPK form, entropy non-null with
// the ENT form
static int test_score_rows(cw_ctx* c, const char* who, int32_t rows, int32_t V, int32_t ldv, const float* logits, const int32_t* targets,
                           int32_t k, int32_t eos, int32_t timestamp_begin, float* logprob, int32_t* top_id, float* top_logprob,
                           float* stop_logprob, int32_t* alt_id, float* alt_logprob, float* entropy);

// cw_test_score_rows_top: the loop path's row kernel (TOPK form) on caller-supplied f32 logits [rows][ldv], any engine.  targets
// [rows] (negative: none).  stop_logprob non-null: the STOP form over S = {eos} + {n >= timestamp_begin}.  Outputs [rows] and
// alt_id / alt_logprob [rows][CW_TOP_LOGPROBS_MAX].
int32_t cw_test_score_rows_top(cw_ctx* c, int32_t rows, int32_t V, int32_t ldv, const float* logits, const int32_t* targets, int32_t k,
                               int32_t eos, int32_t timestamp_begin, float* logprob, int32_t* top_id, float* top_logprob,
                               float* stop_logprob, int32_t* alt_id, float* alt_logprob) {
    if (k < 1) return fail(c, CW_ERR_INVALID, "test_score_rows_top: bad arguments");
    return test_score_rows(c, "test_score_rows_top", rows, V, ldv, logits, targets, k, eos, timestamp_begin, logprob, top_id, top_logprob,
                           stop_logprob, alt_id, alt_logprob, nullptr);
}
// cw_test_score_rows_entropy: the same with the ENT form on: entropy [rows]; k = 0 .. CW_TOP_LOGPROBS_MAX (0: no alternatives, alt_id /
// alt_logprob may be NULL), stop_logprob as above.
int32_t cw_test_score_rows_entropy(cw_ctx* c, int32_t rows, int32_t V, int32_t ldv, const float* logits, const int32_t* targets, int32_t k,
                                   int32_t eos, int32_t timestamp_begin, float* logprob, int32_t* top_id, float* top_logprob,
                                   float* stop_logprob, int32_t* alt_id, float* alt_logprob, float* entropy) {
    if (!entropy) return fail(c, CW_ERR_INVALID, "test_score_rows_entropy: null entropy");
    return test_score_rows(c, "test_score_rows_entropy", rows, V, ldv, logits, targets, k, eos, timestamp_begin, logprob, top_id, top_logprob,
                           stop_logprob, alt_id, alt_logprob, entropy);
}
static int test_score_rows(cw_ctx* c, const char* who, int32_t rows, int32_t V, int32_t ldv, const float* logits, const int32_t* targets,
                           int32_t k, int32_t eos, int32_t timestamp_begin, float* logprob, int32_t* top_id, float* top_logprob,
                           float* stop_logprob, int32_t* alt_id, float* alt_logprob, float* entropy) {
    if (rows < 1 || rows > (1 << 16) || V < 1 || V > (1 << 20) || ldv < V || ldv > (1 << 21) || k < 0 || k > CW_TOP_LOGPROBS_MAX || !logits ||
        !targets || !logprob || !top_id || !top_logprob || (k > 0 && (!alt_id || !alt_logprob)) || (stop_logprob && (eos < 0 || timestamp_begin < 0)))
        return fail(c, CW_ERR_INVALID, "%s: bad arguments", who);
    const size_t W = CW_TOP_LOGPROBS_MAX;
    float* dl = nullptr;
    int* dt = nullptr;
    ScoreRowsOut o{};
    o.eos = eos; o.ts_begin = timestamp_begin; o.k = k;
    DevScope mem;
    if (mem.get(&dl, (size_t)rows * ldv * 4) != hipSuccess || mem.get(&dt, (size_t)rows * 4) != hipSuccess || mem.get(&o.logprob, (size_t)rows * 4) != hipSuccess ||
        mem.get(&o.top_id, (size_t)rows * 4) != hipSuccess || mem.get(&o.top_logprob, (size_t)rows * 4) != hipSuccess ||
        (stop_logprob && mem.get(&o.stop_logprob, (size_t)rows * 4) != hipSuccess) ||
        (entropy && mem.get(&o.entropy, (size_t)rows * 4) != hipSuccess) ||
        (k > 0 && (mem.get(&o.alt_id, (size_t)rows * W * 4) != hipSuccess || mem.get(&o.alt_logprob, (size_t)rows * W * 4) != hipSuccess)))
        return fail(c, CW_ERR_NOMEM, "%s: hipMalloc failed", who);
    HIPCHK(c, hipMemcpy(dl, logits, (size_t)rows * ldv * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dt, targets, (size_t)rows * 4, hipMemcpyHostToDevice));
    CWCHK(c, KD(c, cw_launch_score_rows, dl, ldv, V, dt, 1, 0, rows, o, c->st));
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(logprob, o.logprob, (size_t)rows * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(top_id, o.top_id, (size_t)rows * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(top_logprob, o.top_logprob, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (stop_logprob) HIPCHK(c, hipMemcpy(stop_logprob, o.stop_logprob, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (entropy) HIPCHK(c, hipMemcpy(entropy, o.entropy, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (k > 0) {
        HIPCHK(c, hipMemcpy(alt_id, o.alt_id, (size_t)rows * W * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(alt_logprob, o.alt_logprob, (size_t)rows * W * 4, hipMemcpyDeviceToHost));
    }
    return CW_OK;
}

// cw_test_align_cut: the cut kernel of cw_align_cut_tokens, through its launcher, on caller-supplied scores.  Row r holds n_tok[r]
// text tokens: logprob / stop_logprob / cut_ok [rows][stride] with entries 0 .. n_tok[r] used (stride > the largest n_tok).
// A row that is neither forced nor allowed any cut is refused before the launch, as the call refuses it.
int32_t cw_test_align_cut(cw_ctx* c, int32_t rows, int32_t stride, const int32_t* n_tok, const float* logprob, const float* stop_logprob,
                          const uint8_t* cut_ok, const uint8_t* force_all, int32_t* cut, float* cut_score) {
    if (rows < 1 || rows > (1 << 16) || stride < 1 || stride > (1 << 12) || !n_tok || !logprob || !stop_logprob || !cut_ok || !force_all ||
        !cut || !cut_score) return fail(c, CW_ERR_INVALID, "test_align_cut: bad arguments");
    std::vector<int> base(rows);
    for (int r = 0; r < rows; ++r) {
        if (n_tok[r] < 0 || n_tok[r] >= stride) return fail(c, CW_ERR_INVALID, "test_align_cut: n_tok[%d]=%d outside 0 .. %d", r, n_tok[r], stride - 1);
        bool any = force_all[r] != 0;
        for (int n = 0; !any && n <= n_tok[r]; ++n) any = cut_ok[(size_t)r * stride + n] != 0;
        if (!any) return fail(c, CW_ERR_INVALID, "test_align_cut: row %d is not forced and its cut_ok allows no cut", r);
        base[r] = r * stride;
    }
    const size_t n = (size_t)rows * stride;
    float *dlp = nullptr, *dsl = nullptr, *dsc = nullptr;
    unsigned char *dok = nullptr, *dfo = nullptr;
    int *dba = nullptr, *dnt = nullptr, *dcu = nullptr;
    DevScope mem;
    if (mem.get(&dlp, n * 4) != hipSuccess || mem.get(&dsl, n * 4) != hipSuccess || mem.get(&dok, n) != hipSuccess || mem.get(&dfo, rows) != hipSuccess ||
        mem.get(&dba, (size_t)rows * 4) != hipSuccess || mem.get(&dnt, (size_t)rows * 4) != hipSuccess || mem.get(&dcu, (size_t)rows * 4) != hipSuccess ||
        mem.get(&dsc, (size_t)rows * 4) != hipSuccess) return fail(c, CW_ERR_NOMEM, "test_align_cut: hipMalloc failed");
    HIPCHK(c, hipMemcpy(dlp, logprob, n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dsl, stop_logprob, n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dok, cut_ok, n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dfo, force_all, rows, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dba, base.data(), (size_t)rows * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dnt, n_tok, (size_t)rows * 4, hipMemcpyHostToDevice));
    CWCHK(c, cw_launch_align_cut(dlp, dsl, dba, dnt, dok, stride, dfo, rows, dcu, dsc, c->st));
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(cut, dcu, (size_t)rows * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(cut_score, dsc, (size_t)rows * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// cw_time_score_head: the scoring head at the context's own geometry (d_model, vocabulary, its packed tied embedding) over M
// pseudo-random residual rows: LayerNorm + fused head + combine (unfused = 0), or LayerNorm + the same GEMM storing f32 logits
// [M][Vpad] + a row-wise log-softmax pass (unfused = 1).  avg_ms: HIP-event time per repetition after one warm-up.
int32_t cw_time_score_head(cw_ctx* c, int32_t M, int32_t unfused, int32_t iters, float* avg_ms) {
    if (!c->bf16 || !c->embed_pk) return fail(c, CW_ERR_INVALID, "time_score_head: 16-bit engines with packed weights only");
    if (M < 1 || M > (1 << 15) || iters < 1 || !avg_ms) return fail(c, CW_ERR_INVALID, "time_score_head: bad arguments");
    CWCHK(c, cw_check_weights(c));
    const int D = c->d.d_model, V = c->d.vocab_size;
    const int ns = KD(c, cw_score_head_splits, M, V, nullptr);
    std::vector<float> x((size_t)M * D);
    std::vector<int> tg(M);
    unsigned int lcg = 12345u;
    for (auto& v : x) { lcg = lcg * 1664525u + 1013904223u; v = ((int)(lcg >> 8) % 4001 - 2000) * 1e-3f; }
    for (int m = 0; m < M; ++m) { lcg = lcg * 1664525u + 1013904223u; tg[m] = (int)((lcg >> 8) % (unsigned)V); }
    float *dx = nullptr, *dlog = nullptr;
    int* dt = nullptr;
    void* dA = nullptr;
    ScoreHeadOut o{};
    const bool stop = unfused == 2;              // the STOP form of the fused head, over this context's eos and timestamp ids
    if (stop) unfused = 0;
    if (stop && !c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    o.eos = c->gen.eos_token_id; o.ts_begin = c->gen.no_timestamps_token_id + 1;
    DevScope mem;
    if ((stop && (mem.get(&o.spart, (size_t)M * ns * sizeof(ScoreStopPart)) != hipSuccess || mem.get(&o.stop_logprob, (size_t)M * 4) != hipSuccess)) ||
        mem.get(&dx, x.size() * 4) != hipSuccess || mem.get(&o.logprob, (size_t)M * 4) != hipSuccess ||
        mem.get(&o.top_logprob, (size_t)M * 4) != hipSuccess || mem.get(&dt, (size_t)M * 4) != hipSuccess ||
        mem.get(&o.top_id, (size_t)M * 4) != hipSuccess || mem.get(&dA, (size_t)M * D * 2) != hipSuccess ||
        mem.get(&o.part, (size_t)M * ns * sizeof(ScorePart)) != hipSuccess ||
        (unfused && mem.get(&dlog, (size_t)M * c->Vpad * 4) != hipSuccess)) return fail(c, CW_ERR_NOMEM, "time_score_head: hipMalloc failed");
    if (hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dt, tg.data(), (size_t)M * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(c, CW_ERR_HIP, "time_score_head: copy");
    int r = CW_OK;
    for (int it = 0; it <= iters && r == CW_OK; ++it) {
        if (it == 1 && hipEventRecord(c->ev0, c->st) != hipSuccess) r = fail(c, CW_ERR_HIP, "time_score_head: event");
        if (r == CW_OK) r = KD(c, cw_launch_score_ln, dx, nullptr, c->dec_ln_g, c->dec_ln_b, dA, M, D, c->st);
        if (r == CW_OK) r = unfused ? KD(c, cw_launch_score_head_unfused, dA, c->embed_pk, dt, dlog, c->Vpad, M, V, D, o.logprob, o.top_id, o.top_logprob, c->st)
                                    : KD(c, cw_launch_score_head, dA, c->embed_pk, dt, M, V, D, o, c->st);
    }
    if (r == CW_OK) {
        float ms = 0.f;
        if (hipEventRecord(c->ev1, c->st) != hipSuccess || hipEventSynchronize(c->ev1) != hipSuccess ||
            hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) r = fail(c, CW_ERR_HIP, "time_score_head: event");
        else *avg_ms = ms / (float)iters;
    }
    hipStreamSynchronize(c->st);
    return r;
}

// cw_time_score_head_top: cw_time_score_head's fused forms (stop = 0 / 1) with k alternatives per row; k = 0: the plain forms,
// timed by this same loop
static int time_score_head_forms(cw_ctx* c, const char* who, int32_t M, int32_t k, int32_t stop, bool ent, int32_t iters, float* avg_ms);
int32_t cw_time_score_head_top(cw_ctx* c, int32_t M, int32_t k, int32_t stop, int32_t iters, float* avg_ms) {
    return time_score_head_forms(c, "time_score_head_top", M, k, stop, false, iters, avg_ms);
}
// cw_time_score_head_entropy: the same loop with the ENT form on (entropy [M] and its per-split record array beside the rest)
int32_t cw_time_score_head_entropy(cw_ctx* c, int32_t M, int32_t k, int32_t stop, int32_t iters, float* avg_ms) {
    return time_score_head_forms(c, "time_score_head_entropy", M, k, stop, true, iters, avg_ms);
}
static int time_score_head_forms(cw_ctx* c, const char* who, int32_t M, int32_t k, int32_t stop, bool ent, int32_t iters, float* avg_ms) {
    if (!c->bf16 || !c->embed_pk) return fail(c, CW_ERR_INVALID, "%s: 16-bit engines with packed weights only", who);
    if (M < 1 || M > (1 << 15) || k < 0 || k > CW_TOP_LOGPROBS_MAX || iters < 1 || !avg_ms)
        return fail(c, CW_ERR_INVALID, "%s: bad arguments", who);
    if (stop && !c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    CWCHK(c, cw_check_weights(c));
    const int D = c->d.d_model, V = c->d.vocab_size;
    const int ns = KD(c, cw_score_head_splits, M, V, nullptr);
    std::vector<float> x((size_t)M * D);
    std::vector<int> tg(M);
    unsigned int lcg = 12345u;
    for (auto& v : x) { lcg = lcg * 1664525u + 1013904223u; v = ((int)(lcg >> 8) % 4001 - 2000) * 1e-3f; }
    for (int m = 0; m < M; ++m) { lcg = lcg * 1664525u + 1013904223u; tg[m] = (int)((lcg >> 8) % (unsigned)V); }
    const size_t W = CW_TOP_LOGPROBS_MAX;
    float* dx = nullptr;
    int* dt = nullptr;
    void* dA = nullptr;
    ScoreHeadOut o{};
    o.eos = c->gen.eos_token_id; o.ts_begin = c->gen.no_timestamps_token_id + 1; o.k = k;
    DevScope mem;
    if (mem.get(&dx, x.size() * 4) != hipSuccess || mem.get(&o.logprob, (size_t)M * 4) != hipSuccess || mem.get(&o.top_logprob, (size_t)M * 4) != hipSuccess ||
        mem.get(&dt, (size_t)M * 4) != hipSuccess || mem.get(&o.top_id, (size_t)M * 4) != hipSuccess || mem.get(&dA, (size_t)M * D * 2) != hipSuccess ||
        mem.get(&o.part, (size_t)M * ns * sizeof(ScorePart)) != hipSuccess || mem.get(&o.spart, (size_t)M * ns * sizeof(ScoreStopPart)) != hipSuccess ||
        (stop && mem.get(&o.stop_logprob, (size_t)M * 4) != hipSuccess) || mem.get(&o.tpart, (size_t)M * ns * W * sizeof(ScoreTopPart)) != hipSuccess ||
        mem.get(&o.alt_id, (size_t)M * W * 4) != hipSuccess || mem.get(&o.alt_logprob, (size_t)M * W * 4) != hipSuccess ||
        (ent && (mem.get(&o.epart, (size_t)M * ns * 4) != hipSuccess || mem.get(&o.entropy, (size_t)M * 4) != hipSuccess)))
        return fail(c, CW_ERR_NOMEM, "%s: hipMalloc failed", who);
    HIPCHK(c, hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dt, tg.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    int r = CW_OK;
    for (int it = 0; it <= iters && r == CW_OK; ++it) {
        if (it == 1 && hipEventRecord(c->ev0, c->st) != hipSuccess) r = fail(c, CW_ERR_HIP, "%s: event", who);
        if (r == CW_OK) r = KD(c, cw_launch_score_ln, dx, nullptr, c->dec_ln_g, c->dec_ln_b, dA, M, D, c->st);
        if (r == CW_OK) r = KD(c, cw_launch_score_head, dA, c->embed_pk, dt, M, V, D, o, c->st);
    }
    if (r == CW_OK) {
        float ms = 0.f;
        if (hipEventRecord(c->ev1, c->st) != hipSuccess || hipEventSynchronize(c->ev1) != hipSuccess ||
            hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) r = fail(c, CW_ERR_HIP, "%s: event", who);
        else *avg_ms = ms / (float)iters;
    }
    hipStreamSynchronize(c->st);
    return r;
}

// cw_test_prefill_attention: q [rows * n_q][H * 64], k / v [rows / kv_div][H][cap][64] (f32, rounded to the 16-bit type) ->
// out [rows * n_q][H * 64]: softmax(q k^T) v over keys 0 .. n_keys-1 (causal: keys 0 .. i for query position i; n_keys >= n_q),
// cross K/V row = row / kv_div.  No scale is applied (the engine folds 1/8 into the query projections).
int32_t cw_test_prefill_attention(cw_ctx* c, int32_t rows, int32_t n_q, int32_t H, int32_t cap, int32_t n_keys, int32_t causal,
                                  int32_t kv_div, const float* q, const float* k, const float* v, float* out) {
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_prefill_attention: 16-bit engines only");
    if (rows < 1 || n_q < 1 || H < 1 || cap < 1 || n_keys < 1 || n_keys > cap || kv_div < 1 || rows % kv_div || (causal && n_keys < n_q))
        return fail(c, CW_ERR_INVALID, "test_prefill_attention: bad arguments");
    const size_t e = c->esz, nq = (size_t)rows * n_q * H * 64, nkv = (size_t)(rows / kv_div) * H * cap * 64;
    void *dQ = nullptr, *dK = nullptr, *dV = nullptr, *dO = nullptr;
    int r = CW_OK;
    DevScope mem;
    if (mem.get(&dQ, nq * e) != hipSuccess || mem.get(&dK, nkv * e) != hipSuccess || mem.get(&dV, nkv * e) != hipSuccess ||
        mem.get(&dO, nq * e) != hipSuccess) r = fail(c, CW_ERR_NOMEM, "test_prefill_attention: hipMalloc failed");
    if (r == CW_OK) r = upload_T(c, dQ, 0, q, nq);
    if (r == CW_OK) r = upload_T(c, dK, 0, k, nkv);
    if (r == CW_OK) r = upload_T(c, dV, 0, v, nkv);
    if (r == CW_OK) r = KD(c, cw_launch_prefill_attn, dQ, dK, dV, dO, rows, n_q, H, cap, n_keys, causal ? 1 : 0, kv_div, c->st);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_prefill_attention: %s", hipGetErrorString(er)); }
    if (r == CW_OK) r = download_T(c, dO, 0, out, nq);
    return r;
}

// cw_test_prefill_align_attention: the cross mode of prefill_attn_kernel with head align_head as alignment slot 0.  q [rows * n_q]
// [H * 64], k / v [rows / kv_div][H][n_keys][64] (f32, rounded to the 16-bit type) -> out [rows * n_q][H * 64] and align
// [rows][n_q][n_keys]: the recorded rows after align_normalize_kernel (the softmax weights of head align_head).
int32_t cw_test_prefill_align_attention(cw_ctx* c, int32_t rows, int32_t n_q, int32_t H, int32_t n_keys, int32_t kv_div,
                                        int32_t align_head, const float* q, const float* k, const float* v, float* out, float* align) {
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_prefill_align_attention: 16-bit engines only");
    if (rows < 1 || rows > 64 || n_q < 1 || n_q > 512 || H < 1 || H > 64 || n_keys < 1 || n_keys > 4096 || kv_div < 1 || rows % kv_div ||
        align_head < 0 || align_head >= H || !q || !k || !v || !out || !align)
        return fail(c, CW_ERR_INVALID, "test_prefill_align_attention: bad arguments");
    const size_t e = c->esz, nq = (size_t)rows * n_q * H * 64, nkv = (size_t)(rows / kv_div) * H * n_keys * 64;
    const size_t na = (size_t)rows * n_q * n_keys, nml = (size_t)rows * n_q * ATT_NS * 2;
    std::vector<int> slot(H, -1);
    slot[align_head] = 0;
    void *dQ = nullptr, *dK = nullptr, *dV = nullptr, *dO = nullptr;
    float *dA = nullptr, *dML = nullptr;
    int* dS = nullptr;
    int r = CW_OK;
    DevScope mem;
    if (mem.get(&dQ, nq * e) != hipSuccess || mem.get(&dK, nkv * e) != hipSuccess || mem.get(&dV, nkv * e) != hipSuccess ||
        mem.get(&dO, nq * e) != hipSuccess || mem.get(&dA, na * 4) != hipSuccess || mem.get(&dML, nml * 4) != hipSuccess ||
        mem.get(&dS, (size_t)H * 4) != hipSuccess) r = fail(c, CW_ERR_NOMEM, "test_prefill_align_attention: hipMalloc failed");
    if (r == CW_OK) r = upload_T(c, dQ, 0, q, nq);
    if (r == CW_OK) r = upload_T(c, dK, 0, k, nkv);
    if (r == CW_OK) r = upload_T(c, dV, 0, v, nkv);
    if (r == CW_OK && (hipMemcpy(dS, slot.data(), (size_t)H * 4, hipMemcpyHostToDevice) != hipSuccess ||
                       hipMemset(dA, 0xff, na * 4) != hipSuccess || hipMemset(dML, 0xff, nml * 4) != hipSuccess))
        r = fail(c, CW_ERR_HIP, "test_prefill_align_attention: copy");
    PrefillAlign al;
    al.out = dA; al.ml = dML; al.slot = dS; al.n_align = 1; al.rows = n_q;
    if (r == CW_OK) r = KD(c, cw_launch_prefill_attn_align, dQ, dK, dV, dO, rows, n_q, H, n_keys, n_keys, 0, kv_div, al, c->st);
    if (r == CW_OK) r = KD(c, cw_launch_align_normalize, dA, dML, rows, 1, n_q, n_q, n_keys, c->st);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_prefill_align_attention: %s", hipGetErrorString(er)); }
    if (r == CW_OK) r = download_T(c, dO, 0, out, nq);
    if (r == CW_OK && hipMemcpy(align, dA, na * 4, hipMemcpyDeviceToHost) != hipSuccess) r = fail(c, CW_ERR_HIP, "test_prefill_align_attention: copy");
    return r;
}

// e4m3 GEMM of the opt-in encoder mode: A and W are rounded to the engine's 16-bit type, quantised row-wise on the device
// (quant_rows_fp8_kernel) and multiplied by gemm_fp8_pp_kernel; out = T(A W^T + bias) (gelu optional).  N % 256 == 0, K % 128 == 0.
int32_t cw_test_gemm_fp8(cw_ctx* c, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias,
                         int32_t gelu, float* out) {
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "the fp8 GEMM belongs to the 16-bit engines");
    void *dA = nullptr, *dW = nullptr, *dO = nullptr, *dA8 = nullptr, *dW8 = nullptr; float *dB = nullptr, *dsa = nullptr, *dsw = nullptr;
    const size_t e = c->esz;
    DevScope mem;
    HIPCHK(c, mem.get(&dA, (size_t)M * K * e)); HIPCHK(c, mem.get(&dW, (size_t)N * K * e));
    HIPCHK(c, mem.get(&dA8, (size_t)M * K)); HIPCHK(c, mem.get(&dW8, (size_t)N * K));
    HIPCHK(c, mem.get(&dsa, (size_t)M * 4)); HIPCHK(c, mem.get(&dsw, (size_t)N * 4));
    HIPCHK(c, mem.get(&dO, (size_t)M * N * e)); HIPCHK(c, mem.get(&dB, (size_t)N * 4));
    CWCHK(c, upload_T(c, dA, 0, A, (size_t)M * K)); CWCHK(c, upload_T(c, dW, 0, W, (size_t)N * K));
    if (bias) HIPCHK(c, hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    EpiParams ep = epi0(); ep.out = dO; ep.bias = bias ? dB : nullptr; ep.ldo = N;
    int r = KD(c, cw_launch_quant_rows_fp8, dA, M, K, dA8, dsa, c->st);
    if (r == CW_OK) r = KD(c, cw_launch_quant_rows_fp8, dW, N, K, dW8, dsw, c->st);
    if (r == CW_OK) r = KD(c, cw_launch_gemm_fp8, gelu ? EPI_GELU : EPI_STORE, dA8, K, dW8, M, N, K, dsa, dsw, ep, c->st);
    if (r != CW_OK) fail(c, r, "test_gemm_fp8: launch rejected (M=%d N=%d K=%d)", M, N, K);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_gemm_fp8: %s", hipGetErrorString(er)); }
    if (const int reps = cw_sw::cw_switches().test_gemm_reps) {   // kernel timing for the profiles (stderr only)
        hipEvent_t e0, e1;
        if (r == CW_OK && reps > 0 && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            hipEventRecord(e0, c->st);
            for (int i = 0; i < reps && r == CW_OK; ++i) r = KD(c, cw_launch_gemm_fp8, gelu ? EPI_GELU : EPI_STORE, dA8, K, dW8, M, N, K, dsa, dsw, ep, c->st);
            hipEventRecord(e1, c->st);
            hipEventSynchronize(e1);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            const double us = 1e3 * ms / reps;
            fprintf(stderr, "[cw_test_gemm_fp8] M=%d N=%d K=%d gelu=%d: %.2f us/launch, %.1f TFLOP/s\n", M, N, K, gelu, us, 2.0 * M * N * K / us * 1e-6);
            hipEventDestroy(e0); hipEventDestroy(e1);
        }
    }
    if (r == CW_OK) r = download_T(c, dO, 0, out, (size_t)M * N);
    return r;
}

// One launch of cw_launch_gemm (fp8: cw_launch_quant_rows_fp8 twice + cw_launch_gemm_fp8) with any encoder epilogue and either
// A-operand form, AParams / EpiParams filled the way cw_encode fills them (include/crisperwhisper.h).  Everything the kernels
// derive an address from is checked here, before anything is launched; the outputs start from the caller's contents.
int32_t cw_test_gemm_epi(cw_ctx* c, const cw_test_gemm_epi_args* a) {
    if (!a) return fail(c, CW_ERR_INVALID, "test_gemm_epi: null arguments");
    const int epi = a->epi, M = a->M, N = a->N, K = a->K, ldo = a->ldo;
    const long long lim = 1ll << 26;                                  // elements per buffer: a test hook, not a workload
    if (M < 1 || N < 1 || K < 1 || (long long)M * K > lim || (long long)N * K > lim)
        return fail(c, CW_ERR_INVALID, "test_gemm_epi: shape M=%d N=%d K=%d", M, N, K);
    if (K % 64) return fail(c, CW_ERR_INVALID, "test_gemm_epi: K=%d is not a multiple of 64", K);
    if (!a->A || !a->W) return fail(c, CW_ERR_INVALID, "test_gemm_epi: null operand");
    const bool heads = epi == EPI_HEADS, f32out = epi == EPI_RESID_F32 || epi == EPI_GELU_POS_F32 || epi == EPI_STORE_F32;
    if (!(epi == EPI_STORE || epi == EPI_GELU || heads || f32out)) return fail(c, CW_ERR_INVALID, "test_gemm_epi: epilogue %d", epi);
    if (!a->out) return fail(c, CW_ERR_INVALID, "test_gemm_epi: null output");
    int n_which = 0;
    size_t n_in = (size_t)M * K, n_out = 0;
    if (heads) {
        const int T = a->T, D = a->d_model;
        if (T < 1 || M % T) return fail(c, CW_ERR_INVALID, "test_gemm_epi: M=%d is not a multiple of T=%d", M, T);
        if (D < 64 || D % 64 || a->H != D / 64) return fail(c, CW_ERR_INVALID, "test_gemm_epi: d_model=%d H=%d", D, a->H);
        if (N != 2 * D && N != 3 * D) return fail(c, CW_ERR_INVALID, "test_gemm_epi: N=%d is not 2 or 3 times d_model=%d", N, D);
        if (a->S_pad < T) return fail(c, CW_ERR_INVALID, "test_gemm_epi: S_pad=%d < T=%d", a->S_pad, T);
        n_which = N / D;
        if (!a->out1 || (n_which == 3 && !a->out2)) return fail(c, CW_ERR_INVALID, "test_gemm_epi: null head-split output");
        n_out = (size_t)(M / T) * a->H * a->S_pad * 64;
    } else {
        if (ldo < N) return fail(c, CW_ERR_INVALID, "test_gemm_epi: ldo=%d < N=%d", ldo, N);
        n_out = (size_t)M * ldo;
        if (epi == EPI_GELU_POS_F32 && (!a->pos || a->T < 1)) return fail(c, CW_ERR_INVALID, "test_gemm_epi: positions need pos and T >= 1");
    }
    if ((long long)n_out > lim) return fail(c, CW_ERR_INVALID, "test_gemm_epi: output of %zu elements", n_out);
    if (a->conv) {
        if (a->fp8) return fail(c, CW_ERR_INVALID, "test_gemm_epi: the e4m3 GEMM takes plain A only");
        if (a->C_in < 64 || a->C_in % 64 || K != 3 * a->C_in) return fail(c, CW_ERR_INVALID, "test_gemm_epi: conv gather C_in=%d K=%d", a->C_in, K);
        if (a->nb < 1 || a->T_out < 1 || (long long)a->nb * a->T_out != M || (a->stride != 1 && a->stride != 2))
            return fail(c, CW_ERR_INVALID, "test_gemm_epi: conv gather nb=%d T_out=%d stride=%d M=%d", a->nb, a->T_out, a->stride, M);
        if (a->n_rows < 1 || (long long)a->n_rows * a->C_in > lim || !a->row_off || !a->row_valid)
            return fail(c, CW_ERR_INVALID, "test_gemm_epi: conv gather input of %d rows", a->n_rows);
        for (int b = 0; b < a->nb; ++b)
            if (a->row_off[b] < 0 || a->row_valid[b] < 0 || (long long)a->row_off[b] + a->row_valid[b] > a->n_rows)
                return fail(c, CW_ERR_INVALID, "test_gemm_epi: window %d = rows [%d, %d + %d) outside the %d input rows", b, a->row_off[b],
                            a->row_off[b], a->row_valid[b], a->n_rows);
        n_in = (size_t)a->n_rows * a->C_in;
    }
    if (a->fp8) {
        if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_gemm_epi: the e4m3 GEMM belongs to the 16-bit engines");
        if (!(epi == EPI_STORE || epi == EPI_GELU || epi == EPI_HEADS || epi == EPI_RESID_F32) || N % 256 || K % 128)
            return fail(c, CW_ERR_INVALID, "test_gemm_epi: the e4m3 GEMM takes epilogues 0 / 1 / 2 / 4, N %% 256 == 0, K %% 128 == 0 (epi=%d N=%d K=%d)", epi, N, K);
    }
    const size_t e = c->esz;
    void *dA = nullptr, *dW = nullptr, *dO[3] = {nullptr, nullptr, nullptr}, *dA8 = nullptr, *dW8 = nullptr;
    float *dB = nullptr, *dR = nullptr, *dP = nullptr, *dsa = nullptr, *dsw = nullptr;
    int *doff = nullptr, *dval = nullptr;
    float* const host_out[3] = {a->out, a->out1, a->out2};
    const int n_bufs = heads ? n_which : 1;
    DevScope mem;
    HIPCHK(c, mem.get(&dA, n_in * e)); HIPCHK(c, mem.get(&dW, (size_t)N * K * e));
    CWCHK(c, upload_T(c, dA, 0, a->A, n_in)); CWCHK(c, upload_T(c, dW, 0, a->W, (size_t)N * K));
    for (int i = 0; i < n_bufs; ++i) {
        HIPCHK(c, mem.get(&dO[i], n_out * (f32out ? 4 : e)));
        if (f32out) HIPCHK(c, hipMemcpy(dO[i], host_out[i], n_out * 4, hipMemcpyHostToDevice));
        else CWCHK(c, upload_T(c, dO[i], 0, host_out[i], n_out));
    }
    if (a->bias) { HIPCHK(c, mem.get(&dB, (size_t)N * 4)); HIPCHK(c, hipMemcpy(dB, a->bias, (size_t)N * 4, hipMemcpyHostToDevice)); }
    if (epi == EPI_RESID_F32 && a->resid) { HIPCHK(c, mem.get(&dR, n_out * 4)); HIPCHK(c, hipMemcpy(dR, a->resid, n_out * 4, hipMemcpyHostToDevice)); }
    if (epi == EPI_GELU_POS_F32) {
        HIPCHK(c, mem.get(&dP, (size_t)a->T * ldo * 4));
        HIPCHK(c, hipMemcpy(dP, a->pos, (size_t)a->T * ldo * 4, hipMemcpyHostToDevice));
    }
    AParams ap{dA, K, 0, 0, 0, 0, nullptr, nullptr};
    if (a->conv) {
        HIPCHK(c, mem.get(&doff, (size_t)a->nb * 4)); HIPCHK(c, mem.get(&dval, (size_t)a->nb * 4));
        HIPCHK(c, hipMemcpy(doff, a->row_off, (size_t)a->nb * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dval, a->row_valid, (size_t)a->nb * 4, hipMemcpyHostToDevice));
        ap = AParams{dA, 0, 1, a->T_out, a->C_in, a->stride, doff, dval};
    }
    EpiParams ep = epi0();
    ep.bias = dB;
    if (heads) {
        ep.out = dO[0]; ep.out1 = dO[1]; ep.out2 = dO[2];
        ep.T = a->T; ep.S_pad = a->S_pad; ep.H = a->H; ep.d_model = a->d_model;
    } else if (f32out) {
        ep.outf = (float*)dO[0]; ep.ldo = ldo;
        if (epi == EPI_RESID_F32) ep.resid = dR ? dR : (const float*)dO[0];
        if (epi == EPI_GELU_POS_F32) { ep.pos = dP; ep.T = a->T; }
    } else {
        ep.out = dO[0]; ep.ldo = ldo;
    }
    int r;
    if (a->fp8) {
        HIPCHK(c, mem.get(&dA8, (size_t)M * K)); HIPCHK(c, mem.get(&dW8, (size_t)N * K));
        HIPCHK(c, mem.get(&dsa, (size_t)M * 4)); HIPCHK(c, mem.get(&dsw, (size_t)N * 4));
        r = KD(c, cw_launch_quant_rows_fp8, dA, M, K, dA8, dsa, c->st);
        if (r == CW_OK) r = KD(c, cw_launch_quant_rows_fp8, dW, N, K, dW8, dsw, c->st);
        if (r == CW_OK) r = KD(c, cw_launch_gemm_fp8, epi, dA8, K, dW8, M, N, K, dsa, dsw, ep, c->st);
    } else {
        r = KD(c, cw_launch_gemm, c->bf16, epi, ap, dW, M, N, K, ep, c->st);
    }
    if (r != CW_OK) return fail(c, r, "test_gemm_epi: launch rejected (epi=%d M=%d N=%d K=%d)", epi, M, N, K);
    { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_gemm_epi: %s", hipGetErrorString(er)); }
    { hipError_t er = hipGetLastError(); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_gemm_epi: %s", hipGetErrorString(er)); }
    for (int i = 0; i < n_bufs; ++i) {
        if (f32out) HIPCHK(c, hipMemcpy(host_out[i], dO[i], n_out * 4, hipMemcpyDeviceToHost));
        else CWCHK(c, download_T(c, dO[i], 0, host_out[i], n_out));
    }
    return CW_OK;
}

// One launch of a row kernel of the encoder: 0 cw_launch_layernorm, 1 cw_launch_layernorm_fp8, 2 cw_launch_quant_rows_fp8 on the
// rows rounded to the engine's 16-bit type (include/crisperwhisper.h).  The outputs start from the caller's contents.
int32_t cw_test_rownorm(cw_ctx* c, int32_t mode, int32_t rows, int32_t d, const float* x, const float* gamma, const float* beta,
                        float* out, uint8_t* out8, float* scale) {
    if (mode < 0 || mode > 2) return fail(c, CW_ERR_INVALID, "test_rownorm: mode %d", mode);
    if (rows < 1 || d < 1 || (long long)rows * d > (1ll << 26)) return fail(c, CW_ERR_INVALID, "test_rownorm: rows=%d d=%d", rows, d);
    if (mode != 0 && !c->bf16) return fail(c, CW_ERR_INVALID, "test_rownorm: the e4m3 row kernels belong to the 16-bit engines");
    if (!x || (mode != 2 && (!gamma || !beta)) || (mode == 0 ? !out : (!out8 || !scale))) return fail(c, CW_ERR_INVALID, "test_rownorm: null buffer");
    if ((mode != 2 && d % 4) || (mode == 1 && d > 2048) || (mode == 2 && d % 8)) return fail(c, CW_ERR_INVALID, "test_rownorm: mode %d does not take d=%d", mode, d);
    const size_t n = (size_t)rows * d;
    float *dx = nullptr, *dg = nullptr, *db = nullptr, *dsc = nullptr;
    void *dx16 = nullptr, *dout = nullptr;
    DevScope mem;
    int r;
    if (mode == 2) {
        HIPCHK(c, mem.get(&dx16, n * c->esz));
        CWCHK(c, upload_T(c, dx16, 0, x, n));
    } else {
        HIPCHK(c, mem.get(&dx, n * 4)); HIPCHK(c, mem.get(&dg, (size_t)d * 4)); HIPCHK(c, mem.get(&db, (size_t)d * 4));
        HIPCHK(c, hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dg, gamma, (size_t)d * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(db, beta, (size_t)d * 4, hipMemcpyHostToDevice));
    }
    if (mode == 0) {
        HIPCHK(c, mem.get(&dout, n * c->esz));
        CWCHK(c, upload_T(c, dout, 0, out, n));
        r = KD(c, cw_launch_layernorm, c->bf16, dx, dg, db, dout, rows, d, c->st);
    } else {
        HIPCHK(c, mem.get(&dout, n)); HIPCHK(c, mem.get(&dsc, (size_t)rows * 4));
        HIPCHK(c, hipMemcpy(dout, out8, n, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dsc, scale, (size_t)rows * 4, hipMemcpyHostToDevice));
        if (mode == 1) r = KD(c, cw_launch_layernorm_fp8, dx, dg, db, dout, dsc, rows, d, c->st);
        else r = KD(c, cw_launch_quant_rows_fp8, dx16, rows, d, dout, dsc, c->st);
    }
    if (r != CW_OK) return fail(c, r, "test_rownorm: launch rejected (mode=%d rows=%d d=%d)", mode, rows, d);
    { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_rownorm: %s", hipGetErrorString(er)); }
    { hipError_t er = hipGetLastError(); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_rownorm: %s", hipGetErrorString(er)); }
    if (mode == 0) {
        CWCHK(c, download_T(c, dout, 0, out, n));
    } else {
        HIPCHK(c, hipMemcpy(out8, dout, n, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(scale, dsc, (size_t)rows * 4, hipMemcpyDeviceToHost));
    }
    return CW_OK;
}

int32_t cw_test_gemv(cw_ctx* c, int32_t Mb, int32_t N, int32_t K, const float* x, const float* W, const float* bias,
                     const float* ln_g, const float* ln_b, int32_t gelu, float* out) {
    float *dx = nullptr, *dB = nullptr, *dO = nullptr, *dg = nullptr, *db = nullptr, *dxn = nullptr; void* dW = nullptr;
    DevScope mem;
    HIPCHK(c, mem.get(&dx, (size_t)Mb * K * 4)); HIPCHK(c, mem.get(&dW, (size_t)N * K * c->esz));
    HIPCHK(c, mem.get(&dO, (size_t)Mb * N * 4)); HIPCHK(c, mem.get(&dB, (size_t)N * 4));
    HIPCHK(c, mem.get(&dg, (size_t)K * 4)); HIPCHK(c, mem.get(&db, (size_t)K * 4));
    HIPCHK(c, mem.get(&dxn, (size_t)Mb * K * 4));
    HIPCHK(c, hipMemcpy(dx, x, (size_t)Mb * K * 4, hipMemcpyHostToDevice));
    CWCHK(c, upload_T(c, dW, 0, W, (size_t)N * K));
    if (bias) HIPCHK(c, hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    if (ln_g) { HIPCHK(c, hipMemcpy(dg, ln_g, (size_t)K * 4, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(db, ln_b, (size_t)K * 4, hipMemcpyHostToDevice)); }
    EpiParams ep = epi0(); ep.outf = dO; ep.bias = bias ? dB : nullptr; ep.ldo = N;
    int r = CW_OK;
    const float* xin = dx;
    if (ln_g && !c->bf16) { r = KD(c, cw_launch_layernorm_f32, dx, dg, db, dxn, Mb, K, c->st); xin = dxn; }
    if (r == CW_OK) r = KD(c, cw_launch_gemv, c->bf16, gelu ? EPI_GELU_F32 : EPI_STORE_F32, xin, Mb, K, dW, N,
                                        (ln_g && c->bf16) ? dg : nullptr, (ln_g && c->bf16) ? db : nullptr, ep, c->st, nullptr, c->d_xfrag);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_gemv: %s", hipGetErrorString(er)); }
    else fail(c, r, "test_gemv: launch rejected (Mb=%d N=%d K=%d)", Mb, N, K);
    if (r == CW_OK) { hipError_t er = hipMemcpy(out, dO, (size_t)Mb * N * 4, hipMemcpyDeviceToHost); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_gemv copy"); }
    return r;
}

// One skinny-M decoder projection (skinny.hip) on caller-supplied rows, 16-bit engines only.
//   mode 0: out[Mb][N] = n(x) W^T + bias, n = LayerNorm without affine part (folded weights), through K-split planes + finish
//   mode 1: the same through the GELU epilogue (16-bit fragment-major on the device, returned row-major as f32)
//   mode 2: out[Mb][N] (in/out, on the 2^-12 grid) += x16 W^T + bias, x16 = x rounded to the engine's 16-bit type
// nks: k-steps of 32 per block (0: the launcher's own choice).  reps > 0: the launches are also timed over `reps` rounds on
// rotating weight copies larger than the Infinity Cache (cold weights, as in a decoder pass); us[0] = GEMM, us[1] = finish.
int32_t cw_test_skinny(cw_ctx* c, int32_t mode, int32_t Mb, int32_t N, int32_t K, const float* x, const float* W, const float* bias,
                       int32_t nks, int32_t reps, float* out, float* us) {
#ifndef CW_EXPERIMENTS
    return fail(c, CW_ERR_INVALID, "cw_test_skinny: csrc/skinny.hip is an A/B build (make EXTRA=-DCW_EXPERIMENTS)");
#endif
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "cw_test_skinny: 16-bit engines only");
    const bool slice_stats = (mode & 4) != 0;   // LayerNorm statistics from the GEMM's slice records instead of re-reading x
    mode &= 3;
    if (Mb < 1 || Mb > 64 || K % 32 || N % 16 || mode < 0 || mode > 2 || (mode == 1 && N % 32)) return fail(c, CW_ERR_INVALID, "cw_test_skinny: bad shape");
    const int MT = (Mb + 15) / 16;
    if (nks <= 0) nks = KD(c, cw_skinny_pick_nks, N, K, mode == 2 ? 0 : 16);
    if (nks < 1 || (K / 32) % nks) return fail(c, CW_ERR_INVALID, "cw_test_skinny: nks %d does not divide K / 32", nks);
    const int S = (K / 32) / nks;
    const size_t wbytes = (size_t)N * K * 2;
    int ncopy = 1;
    if (reps > 0) { ncopy = (int)((size_t)320 * 1024 * 1024 / wbytes) + 1; if (ncopy > 64) ncopy = 64; }
    DevScope mem;
    float *dx = nullptr, *dB = nullptr, *dO = nullptr, *dws = nullptr, *dP = nullptr, *dst = nullptr; void *dW = nullptr, *dWp = nullptr, *dxf = nullptr, *dfr = nullptr;
    HIPCHK(c, mem.get(&dst, (size_t)64 * 64 * 2 * 4));
    HIPCHK(c, mem.get(&dx, (size_t)Mb * K * 4)); HIPCHK(c, mem.get(&dW, wbytes)); HIPCHK(c, mem.get(&dWp, wbytes * ncopy));
    HIPCHK(c, mem.get(&dO, (size_t)Mb * N * 4)); HIPCHK(c, mem.get(&dB, (size_t)N * 4)); HIPCHK(c, mem.get(&dws, (size_t)N * 4));
    HIPCHK(c, mem.get(&dP, (size_t)S * Mb * N * 4)); HIPCHK(c, mem.get(&dxf, (size_t)MT * 16 * K * 2)); HIPCHK(c, mem.get(&dfr, (size_t)MT * 16 * N * 2));
    HIPCHK(c, hipMemcpy(dx, x, (size_t)Mb * K * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(dB, 0, (size_t)N * 4));
    if (bias) HIPCHK(c, hipMemcpy(dB, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    CWCHK(c, upload_T(c, dW, 0, W, (size_t)N * K));
    CWCHK(c, KD(c, cw_launch_fold_rowvec, nullptr, nullptr, 1.0f, nullptr, dW, N, K, nullptr, dws, c->st));
    for (int i = 0; i < ncopy; ++i) CWCHK(c, KD(c, cw_launch_wfrag_pack, dW, N, K, (char*)dWp + wbytes * i, c->st));
    if (mode == 2) {
        std::vector<bf16_t> xf((size_t)MT * 16 * K, 0);
        for (int m = 0; m < Mb; ++m)
            for (int k = 0; k < K; ++k) xf[frag_index(m, k, K)] = c->f16 ? cw_host_f32_to_f16(x[(size_t)m * K + k]) : cw_host_f32_to_bf16(x[(size_t)m * K + k]);
        HIPCHK(c, hipMemcpy(dxf, xf.data(), xf.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dO, out, (size_t)Mb * N * 4, hipMemcpyHostToDevice));
    }
    SkinnyParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.x = dx; sp.xf = dxf; sp.W = dWp; sp.Mb = Mb; sp.K = K; sp.N = N; sp.planes = dP; sp.outf = dO; sp.bias = dB; sp.ldo = N;
    if (reps > 0 && getenv("CW_SK_DBG")) sp.dbg = atoi(getenv("CW_SK_DBG"));   // ablation of the timed launches (-DCW_SK_DEBUG builds; tools/skinny_ablate.py changes it between calls, so not in cw_switches)
    const int sk_dbg = sp.dbg;
    sp.dbg = 0;
    SkinnyFinishParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.planes = dP; fp.S = S; fp.Mb = Mb; fp.N = N; fp.x = dx; fp.K = K; fp.wsum = dws; fp.ep = epi0();
    fp.ep.bias = dB; fp.ep.outf = dO; fp.ep.out = dfr; fp.ep.ldo = N;
    if (slice_stats && mode != 2) {
        if (S > 16) { return fail(c, CW_ERR_INVALID, "cw_test_skinny: slice statistics need S <= 16"); }
        sp.stats = dst; fp.stats = dst;
    }
    const int epi = mode == 1 ? EPI_GELU_FRAG : EPI_STORE_F32;
    int r = KD(c, cw_launch_skinny, mode == 2 ? 1 : 0, sp, nks, c->st);
    if (r == CW_OK && mode != 2) r = KD(c, cw_launch_skinny_finish, epi, fp, c->st);
    if (r != CW_OK) fail(c, r, "cw_test_skinny: launch rejected (mode=%d Mb=%d N=%d K=%d nks=%d)", mode, Mb, N, K, nks);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "cw_test_skinny: %s", hipGetErrorString(er)); }
    if (r == CW_OK) { hipError_t er = hipGetLastError(); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "cw_test_skinny: %s", hipGetErrorString(er)); }
    if (r == CW_OK && mode == 1) {
        std::vector<bf16_t> fr((size_t)MT * 16 * N);
        if (hipMemcpy(fr.data(), dfr, fr.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) r = fail(c, CW_ERR_HIP, "cw_test_skinny copy");
        else for (int m = 0; m < Mb; ++m)
            for (int n = 0; n < N; ++n) { const bf16_t v = fr[frag_index(m, n, N)]; out[(size_t)m * N + n] = c->f16 ? cw_host_f16_to_f32(v) : cw_host_bf16_to_f32(v); }
    } else if (r == CW_OK) {
        if (hipMemcpy(out, dO, (size_t)Mb * N * 4, hipMemcpyDeviceToHost) != hipSuccess) r = fail(c, CW_ERR_HIP, "cw_test_skinny copy");
    }
    if (r == CW_OK && reps > 0 && us) {
        // `reps` dependent launches captured as one hipGraph (how the decode step runs them) and replayed; the last replay is timed
        sp.dbg = sk_dbg;
        auto time_graph = [&](const std::function<int(int)>& launch, float* us_out) -> int {
            hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
            if (hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal) != hipSuccess) return CW_ERR_HIP;
            int rr = CW_OK;
            for (int i = 0; i < reps && rr == CW_OK; ++i) rr = launch(i);
            hipError_t e = hipStreamEndCapture(c->st, &g);
            if (rr == CW_OK && e != hipSuccess) rr = CW_ERR_HIP;
            if (rr == CW_OK && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) rr = CW_ERR_HIP;
            if (g) hipGraphDestroy(g);
            if (rr != CW_OK) return rr;
            hipEvent_t e0, e1;
            hipEventCreate(&e0); hipEventCreate(&e1);
            float best = 1e30f;
            for (int k = 0; k < 4; ++k) {
                hipEventRecord(e0, c->st);
                hipGraphLaunch(ge, c->st);
                hipEventRecord(e1, c->st);
                hipEventSynchronize(e1);
                float ms = 0.f;
                hipEventElapsedTime(&ms, e0, e1);
                if (k > 0 && ms < best) best = ms;
            }
            hipEventDestroy(e0); hipEventDestroy(e1); hipGraphExecDestroy(ge);
            *us_out = 1e3f * best / reps;
            return CW_OK;
        };
        r = time_graph([&](int i) { sp.W = (char*)dWp + wbytes * (i % ncopy); return KD(c, cw_launch_skinny, mode == 2 ? 1 : 0, sp, nks, c->st); }, &us[0]);
        if (r == CW_OK && mode != 2) r = time_graph([&](int) { return KD(c, cw_launch_skinny_finish, epi, fp, c->st); }, &us[1]);
        if (r == CW_OK && mode == 2) {                       // no finish launch: the floor of an empty launch instead (negative)
            r = time_graph([&](int) { KD(c, cw_launch_skinny_empty, c->st); return (int)CW_OK; }, &us[1]);
            us[1] = -us[1];
        }
        if (r != CW_OK) fail(c, r, "cw_test_skinny: timing graph failed");
    }
    return r;
}

// One launch of the encoder self-attention on caller-supplied rows.  K and V rows S .. S_pad-1 are zero, the engine's contract
// (dmalloc zeroes kb / vb and the head-split epilogue writes rows < T only); the Q pad rows are zero too, or NaN under the option
// "attn_poison_qpad" (the kernels clamp query loads to row S-1: nothing may change).  `out` is in / out; ATTN_GUARD_ROWS rows of
// 0xFF bytes lie behind it on the device and have to come back untouched.
#define ATTN_GUARD_ROWS 64
int32_t cw_test_attention(cw_ctx* c, int32_t B, int32_t H, int32_t S, const float* q, const float* k, const float* v, float* out) {
    if (B < 1 || H < 1 || S < 1 || !q || !k || !v || !out) return fail(c, CW_ERR_INVALID, "test_attention: bad arguments (B=%d H=%d S=%d)", B, H, S);
    const int S_pad = (S + 63) & ~63;
    const size_t e = c->esz, nh = (size_t)B * H * S_pad * 64, nout = (size_t)B * S * H * 64, nguard = (size_t)ATTN_GUARD_ROWS * H * 64 * e;
    DevScope mem;
    void *dq = nullptr, *dk = nullptr, *dv = nullptr, *dout = nullptr;
    HIPCHK(c, mem.get(&dq, nh * e)); HIPCHK(c, mem.get(&dk, nh * e)); HIPCHK(c, mem.get(&dv, nh * e));
    HIPCHK(c, mem.get(&dout, nout * e + nguard));
    HIPCHK(c, hipMemset(dq, g_test_attn_poison_qpad ? 0xFF : 0, nh * e));   // all-ones is a NaN in bf16, f16 and f32
    HIPCHK(c, hipMemset(dk, 0, nh * e)); HIPCHK(c, hipMemset(dv, 0, nh * e));
    HIPCHK(c, hipMemset((char*)dout + nout * e, 0xFF, nguard));
    for (int bh = 0; bh < B * H; ++bh) {   // inputs are [B][H][S][64]
        CWCHK(c, upload_T(c, dq, (size_t)bh * S_pad * 64, q + (size_t)bh * S * 64, (size_t)S * 64));
        CWCHK(c, upload_T(c, dk, (size_t)bh * S_pad * 64, k + (size_t)bh * S * 64, (size_t)S * 64));
        CWCHK(c, upload_T(c, dv, (size_t)bh * S_pad * 64, v + (size_t)bh * S * 64, (size_t)S * 64));
    }
    CWCHK(c, upload_T(c, dout, 0, out, nout));
    int r = KD(c, cw_launch_attn_encoder, c->bf16, dq, dk, dv, dout, B, H, S, S_pad, c->st);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_attention: %s", hipGetErrorString(er)); }
    if (const int reps = cw_sw::cw_switches().test_attn_reps) {   // kernel A/B timing for the profiles (stderr only)
        hipEvent_t e0, e1;
        if (r == CW_OK && reps > 0 && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            hipEventRecord(e0, c->st);
            for (int i = 0; i < reps && r == CW_OK; ++i) r = KD(c, cw_launch_attn_encoder, c->bf16, dq, dk, dv, dout, B, H, S, S_pad, c->st);
            hipEventRecord(e1, c->st);
            hipEventSynchronize(e1);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            const double us = 1e3 * ms / reps, fl = 4.0 * B * H * (double)S * S * 64;
            fprintf(stderr, "[cw_test_attention] B=%d H=%d S=%d: %.2f us/launch, %.1f TFLOP/s\n", B, H, S, us, fl / us * 1e-6);
            hipEventDestroy(e0); hipEventDestroy(e1);
        }
    }
    if (r == CW_OK) r = download_T(c, dout, 0, out, nout);
    if (r == CW_OK) {
        std::vector<unsigned char> guard(nguard);
        HIPCHK(c, hipMemcpy(guard.data(), (const char*)dout + nout * e, nguard, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nguard; ++i)
            if (guard[i] != 0xFF) { return fail(c, CW_ERR_STATE, "test_attention: the kernel wrote behind the output (guard byte %zu)", i); }
    }
    return r;
}

// One launch of the key-split cross-attention decode kernel on caller-supplied rows: q [B][H*64] (already scaled), k / v
// [B / kv_div][H][S][64].  part_o [ATT_NS][B][H*64] and part_ml [B][H][ATT_NS][2] come back raw (the consumer's combine is the
// test's); head `align_head` is captured as alignment slot 0: align [B][S] un-normalised + align_ml [B][ATT_NS][2].
int32_t cw_test_cross_attention(cw_ctx* c, int32_t B, int32_t H, int32_t S, int32_t kv_div, const float* q, const float* k,
                                const float* v, int32_t align_head, float* part_o, float* part_ml, float* align, float* align_ml) {
    if (B < 1 || H < 1 || S < 1 || kv_div < 1 || B % kv_div || align_head < 0 || align_head >= H) return fail(c, CW_ERR_INVALID, "test_cross_attention: shape");
    const int Bk = B / kv_div, D = H * 64;
    const size_t nkv = (size_t)Bk * H * S * 64;
    float *dq = nullptr, *dpo = nullptr, *dml = nullptr, *dal = nullptr, *daml = nullptr; void *dk = nullptr, *dv = nullptr;
    int *dslot = nullptr, *dpos = nullptr;
    DevScope mem;
    HIPCHK(c, mem.get(&dq, (size_t)B * D * 4)); HIPCHK(c, mem.get(&dk, nkv * c->esz)); HIPCHK(c, mem.get(&dv, nkv * c->esz));
    HIPCHK(c, mem.get(&dpo, (size_t)ATT_NS * B * D * 4)); HIPCHK(c, mem.get(&dml, (size_t)B * H * ATT_NS * 2 * 4));
    HIPCHK(c, mem.get(&dal, (size_t)B * S * 4)); HIPCHK(c, mem.get(&daml, (size_t)B * ATT_NS * 2 * 4));
    HIPCHK(c, mem.get(&dslot, (size_t)H * 4)); HIPCHK(c, mem.get(&dpos, (size_t)B * 4));
    std::vector<int> slot(H, -1); slot[align_head] = 0;
    HIPCHK(c, hipMemcpy(dslot, slot.data(), (size_t)H * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(dpos, 0, (size_t)B * 4)); HIPCHK(c, hipMemset(dal, 0, (size_t)B * S * 4));
    HIPCHK(c, hipMemcpy(dq, q, (size_t)B * D * 4, hipMemcpyHostToDevice));
    CWCHK(c, upload_T(c, dk, 0, k, nkv)); CWCHK(c, upload_T(c, dv, 0, v, nkv));
    CrossSplitParams p{};
    p.q = dq; p.K = dk; p.V = dv; p.n_keys = S; p.part_o = dpo; p.part_ml = dml; p.align_out = dal; p.align_ml = daml;
    p.align_slot = dslot; p.pos = dpos; p.n_align = 1; p.align_rows = 1; p.B = B; p.H = H; p.kv_div = kv_div;
    // option "cross_test_fp8": the rows go through the e4m3 cache instead (quantiser + the fp8 cross-attention kernel)
    void *dk8 = nullptr, *dv8 = nullptr; float* dkvs = nullptr;
    const bool fp8 = g_test_cross_fp8 && c->bf16;
    if (fp8) {
        HIPCHK(c, mem.get(&dk8, nkv)); HIPCHK(c, mem.get(&dv8, (size_t)Bk * cw_bf16::cw_kv8_v_bytes(H, S)));
        HIPCHK(c, mem.get(&dkvs, (size_t)Bk * H * 2 * 4));
        int rq = KD(c, cw_launch_kv_quant_fp8, dk, dv, dk8, dv8, dkvs, Bk, H, S, c->st);
        if (rq != CW_OK) { return fail(c, rq, "test_cross_attention: quantiser rejected S=%d", S); }
        p.K = dk8; p.V = dv8; p.kv_scale = dkvs;
    }
    auto launch = [&]() { return fp8 ? KD(c, cw_launch_attn_cross_split_fp8, p, c->st) : KD(c, cw_launch_attn_cross_split, c->bf16, p, c->st); };
    int r = launch();
    if (r != CW_OK) fail(c, r, "test_cross_attention: launch rejected (B=%d H=%d S=%d kv_div=%d)", B, H, S, kv_div);
    if (r == CW_OK) { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) r = fail(c, CW_ERR_HIP, "test_cross_attention: %s", hipGetErrorString(er)); }
    if (const int reps = cw_sw::cw_switches().test_attn_reps) {   // kernel A/B timing for the profiles (stderr only)
        hipEvent_t e0, e1;
        if (r == CW_OK && reps > 0 && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            hipEventRecord(e0, c->st);
            for (int i = 0; i < reps && r == CW_OK; ++i) r = launch();
            hipEventRecord(e1, c->st);
            hipEventSynchronize(e1);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            fprintf(stderr, "[cw_test_cross_attention] B=%d H=%d S=%d kv_div=%d: %.2f us/launch\n", B, H, S, kv_div, 1e3 * ms / reps);
            hipEventDestroy(e0); hipEventDestroy(e1);
        }
    }
    if (r == CW_OK && (hipMemcpy(part_o, dpo, (size_t)ATT_NS * B * D * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(part_ml, dml, (size_t)B * H * ATT_NS * 2 * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(align, dal, (size_t)B * S * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(align_ml, daml, (size_t)B * ATT_NS * 2 * 4, hipMemcpyDeviceToHost) != hipSuccess))
        r = fail(c, CW_ERR_HIP, "test_cross_attention copy");
    return r;
}

// cw_test_cross_attention with the query left to the kernel (the fused out-projection stage of decfuse.hip): qa, qb [B][H*64], qw,
// qbias [H*64] and the producer's planes pstats [ceil(B / 16)][n_pstats][16][2] replace q.  CrossSplitParams as decode_step fills
// them behind X1, and its dispatch: e4m3 cache -> cw_launch_attn_cross_split_fp8, else cw_launch_attn_cross_split.
int32_t cw_test_cross_attention_fused(cw_ctx* c, int32_t B, int32_t H, int32_t S, int32_t kv_div, const float* qa, const float* qb,
                                      const float* qw, const float* qbias, const float* pstats, int32_t n_pstats, const float* k,
                                      const float* v, int32_t align_head, float* part_o, float* part_ml, float* align, float* align_ml) {
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_cross_attention_fused: 16-bit engines only");
    if (B < 1 || B > 64 || H < 1 || H > 1024 || S < 1 || S > 8192 || kv_div < 1 || B % kv_div || align_head < 0 || align_head >= H || n_pstats < 1 || n_pstats > 128)
        return fail(c, CW_ERR_INVALID, "test_cross_attention_fused: shape B=%d H=%d S=%d kv_div=%d n_pstats=%d", B, H, S, kv_div, n_pstats);
    if (!qa || !qb || !qw || !qbias || !pstats || !k || !v || !part_o || !part_ml || !align || !align_ml)
        return fail(c, CW_ERR_INVALID, "test_cross_attention_fused: null buffer");
    const bool fp8 = c->kv8;
    if (fp8 && (kv_div > 1 || !KD(c, cw_cross8_is_mfma, S)))   // refused by the launcher: here, in front of the quantiser's launch
        return fail(c, CW_ERR_INVALID, "test_cross_attention_fused: the e4m3 cache finishes the query at kv_div == 1 in the matrix-core kernel only (kv_div=%d S=%d)", kv_div, S);
    const int Bk = B / kv_div, D = H * 64, groups = (B + 15) / 16;
    const size_t nkv = (size_t)Bk * H * S * 64, nps = (size_t)groups * n_pstats * 32;
    float *dqa = nullptr, *dqb = nullptr, *dqw = nullptr, *dqc = nullptr, *dps = nullptr, *dpo = nullptr, *dml = nullptr, *dal = nullptr,
          *daml = nullptr, *dkvs = nullptr;
    void *dk = nullptr, *dv = nullptr, *dk8 = nullptr, *dv8 = nullptr;
    int *dslot = nullptr, *dpos = nullptr;
    DevScope mem;
    HIPCHK(c, mem.get(&dqa, (size_t)2 * B * D * 4)); dqb = dqa + (size_t)B * D;   // one allocation, as the engine's: the kernel takes qb as an offset from qa
    HIPCHK(c, mem.get(&dqw, (size_t)D * 4)); HIPCHK(c, mem.get(&dqc, (size_t)D * 4));
    HIPCHK(c, mem.get(&dps, (nps + 128 * 32) * 4));   // 128 further plane slots of NaN: what a read beyond n_pstats in the last group meets
    HIPCHK(c, hipMemset(dps + nps, 0xFF, (size_t)128 * 32 * 4));
    HIPCHK(c, mem.get(&dk, nkv * c->esz)); HIPCHK(c, mem.get(&dv, nkv * c->esz));
    HIPCHK(c, mem.get(&dpo, (size_t)ATT_NS * B * D * 4)); HIPCHK(c, mem.get(&dml, (size_t)B * H * ATT_NS * 2 * 4));
    HIPCHK(c, mem.get(&dal, (size_t)B * S * 4)); HIPCHK(c, mem.get(&daml, (size_t)B * ATT_NS * 2 * 4));
    HIPCHK(c, mem.get(&dslot, (size_t)H * 4)); HIPCHK(c, mem.get(&dpos, (size_t)B * 4));
    std::vector<int> slot(H, -1); slot[align_head] = 0;
    HIPCHK(c, hipMemcpy(dslot, slot.data(), (size_t)H * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(dpos, 0, (size_t)B * 4)); HIPCHK(c, hipMemset(dal, 0, (size_t)B * S * 4));
    HIPCHK(c, hipMemset(daml, 0, (size_t)B * ATT_NS * 2 * 4));
    HIPCHK(c, hipMemcpy(dqa, qa, (size_t)B * D * 4, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(dqb, qb, (size_t)B * D * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dqw, qw, (size_t)D * 4, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(dqc, qbias, (size_t)D * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dps, pstats, nps * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dpo, part_o, (size_t)ATT_NS * B * D * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dml, part_ml, (size_t)B * H * ATT_NS * 2 * 4, hipMemcpyHostToDevice));
    CWCHK(c, upload_T(c, dk, 0, k, nkv)); CWCHK(c, upload_T(c, dv, 0, v, nkv));
    CrossSplitParams p{};
    p.K = dk; p.V = dv; p.n_keys = S; p.part_o = dpo; p.part_ml = dml; p.align_out = dal; p.align_ml = daml;
    p.align_slot = dslot; p.pos = dpos; p.n_align = 1; p.align_rows = 1; p.B = B; p.H = H; p.kv_div = kv_div;
    p.qa = dqa; p.qb = dqb; p.qw = dqw; p.qbias = dqc; p.pstats = dps; p.n_pstats = n_pstats;
    if (fp8) {
        HIPCHK(c, mem.get(&dk8, nkv)); HIPCHK(c, mem.get(&dv8, (size_t)Bk * cw_bf16::cw_kv8_v_bytes(H, S)));
        HIPCHK(c, mem.get(&dkvs, (size_t)Bk * H * 2 * 4));
        int rq = KD(c, cw_launch_kv_quant_fp8, dk, dv, dk8, dv8, dkvs, Bk, H, S, c->st);
        if (rq != CW_OK) { return fail(c, rq, "test_cross_attention_fused: quantiser rejected S=%d", S); }
        p.K = dk8; p.V = dv8; p.kv_scale = dkvs;
    }
    int r = fp8 ? KD(c, cw_launch_attn_cross_split_fp8, p, c->st) : KD(c, cw_launch_attn_cross_split, true, p, c->st);
    if (r != CW_OK) {
        hipStreamSynchronize(c->st);
        return fail(c, r, "test_cross_attention_fused: launch rejected (B=%d H=%d S=%d kv_div=%d n_pstats=%d)", B, H, S, kv_div, n_pstats);
    }
    { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_cross_attention_fused: %s", hipGetErrorString(er)); }
    { hipError_t er = hipGetLastError(); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_cross_attention_fused: %s", hipGetErrorString(er)); }
    HIPCHK(c, hipMemcpy(part_o, dpo, (size_t)ATT_NS * B * D * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(part_ml, dml, (size_t)B * H * ATT_NS * 2 * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(align, dal, (size_t)B * S * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(align_ml, daml, (size_t)B * ATT_NS * 2 * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// One launch of a load-time rewrite (include/crisperwhisper.h): the launchers apply_folds / pack_decoder_weights call, on
// caller-supplied operands.  f32 operands stay f32 on the device, as the staged checkpoint tensors do; 16-bit outputs start from
// the caller's contents.
int32_t cw_test_fold(cw_ctx* c, const cw_test_fold_args* a) {
    if (!a) return fail(c, CW_ERR_INVALID, "test_fold: null arguments");
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_fold: 16-bit engines only");
    const int op = a->op, N = a->N, J = a->J, K = a->K;
    const long long lim = 1ll << 26;
    if (op < 0 || op > 3) return fail(c, CW_ERR_INVALID, "test_fold: op %d", op);
    const bool useJ = op == 1 || op == 2, useK = op != 2;
    if (N < 1 || (useJ && J < 1) || (useK && K < 1) || (useJ && (long long)N * J > lim) || (useK && (long long)N * K > lim) ||
        (op == 1 && (long long)J * K > lim))
        return fail(c, CW_ERR_INVALID, "test_fold: op %d shape N=%d J=%d K=%d", op, N, J, K);
    const size_t e = c->esz;
    DevScope mem;
    auto up = [&](float** d, const float* h, size_t n) -> int {
        HIPCHK(c, mem.get(d, n * 4));
        HIPCHK(c, hipMemcpy(*d, h, n * 4, hipMemcpyHostToDevice));
        return CW_OK;
    };
    float *dA = nullptr, *ds = nullptr, *dv = nullptr, *dc = nullptr, *dw = nullptr;
    void *d16 = nullptr, *dimg = nullptr;
    int r = CW_OK;
    if (op == 0) {
        if (!a->a || !a->s || !a->v || !a->out16 || !a->c_out) return fail(c, CW_ERR_INVALID, "test_fold: null buffer (fold_layernorm)");
        if (K % 4) return fail(c, CW_ERR_INVALID, "test_fold: fold_layernorm takes K %% 4 == 0 (K=%d)", K);
        CWCHK(c, up(&dA, a->a, (size_t)N * K)); CWCHK(c, up(&ds, a->s, K)); CWCHK(c, up(&dv, a->v, K)); CWCHK(c, up(&dc, a->c_out, N));
        HIPCHK(c, mem.get(&d16, (size_t)N * K * e)); CWCHK(c, upload_T(c, d16, 0, a->out16, (size_t)N * K));
        r = KD(c, cw_launch_fold_layernorm, dA, N, K, ds, dv, a->scale, d16, dc, c->st);
    } else if (op == 1) {
        if (!a->a || !a->v || !a->out16) return fail(c, CW_ERR_INVALID, "test_fold: null buffer (fold_product)");
        if (N % 64 || K % 64 || J % 16) return fail(c, CW_ERR_INVALID, "test_fold: fold_product takes N %% 64 == 0, K %% 64 == 0, J %% 16 == 0 (N=%d J=%d K=%d)", N, J, K);
        CWCHK(c, up(&dA, a->a, (size_t)N * J)); CWCHK(c, up(&dv, a->v, (size_t)J * K));
        if (a->s) CWCHK(c, up(&ds, a->s, J));
        HIPCHK(c, mem.get(&d16, (size_t)N * K * e)); CWCHK(c, upload_T(c, d16, 0, a->out16, (size_t)N * K));
        r = KD(c, cw_launch_fold_product, dA, ds, a->scale, dv, N, J, K, d16, c->st);
    } else if (op == 2) {
        if ((!a->c_out && !a->w_out) || (a->c_out && (!a->a || !a->v)) || (a->w_out && !a->w16)) return fail(c, CW_ERR_INVALID, "test_fold: null buffer (fold_rowvec)");
        if (a->c_out) {
            CWCHK(c, up(&dA, a->a, (size_t)N * J)); CWCHK(c, up(&dv, a->v, J)); CWCHK(c, up(&dc, a->c_out, N));
            if (a->s) CWCHK(c, up(&ds, a->s, J));
        }
        if (a->w_out) {
            CWCHK(c, up(&dw, a->w_out, N));
            HIPCHK(c, mem.get(&d16, (size_t)N * J * e)); CWCHK(c, upload_T(c, d16, 0, a->w16, (size_t)N * J));
        }
        r = KD(c, cw_launch_fold_rowvec, dA, ds, a->scale, dv, d16, N, J, dc, dw, c->st);
    } else {
        if (!a->a || !a->image) return fail(c, CW_ERR_INVALID, "test_fold: null buffer (wfrag_pack)");
        if (K % 32) return fail(c, CW_ERR_INVALID, "test_fold: wfrag_pack takes K %% 32 == 0 (K=%d)", K);
        const size_t ni = KD(c, cw_wfrag_elems, N, K);
        HIPCHK(c, mem.get(&d16, (size_t)N * K * e)); CWCHK(c, upload_T(c, d16, 0, a->a, (size_t)N * K));
        HIPCHK(c, mem.get(&dimg, ni * 2)); HIPCHK(c, hipMemcpy(dimg, a->image, ni * 2, hipMemcpyHostToDevice));
        r = KD(c, cw_launch_wfrag_pack, d16, N, K, dimg, c->st);
    }
    if (r != CW_OK) return fail(c, r, "test_fold: launch rejected (op=%d N=%d J=%d K=%d)", op, N, J, K);
    { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_fold: %s", hipGetErrorString(er)); }
    { hipError_t er = hipGetLastError(); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_fold: %s", hipGetErrorString(er)); }
    if (op == 0 || op == 1) CWCHK(c, download_T(c, d16, 0, a->out16, (size_t)N * K));
    if (dc) HIPCHK(c, hipMemcpy(a->c_out, dc, (size_t)N * 4, hipMemcpyDeviceToHost));
    if (dw) HIPCHK(c, hipMemcpy(a->w_out, dw, (size_t)N * 4, hipMemcpyDeviceToHost));
    if (op == 3) HIPCHK(c, hipMemcpy(a->image, dimg, KD(c, cw_wfrag_elems, N, K) * 2, hipMemcpyDeviceToHost));
    return CW_OK;
}

// One cw_launch_gemv_stack call on caller-supplied operands (include/crisperwhisper.h).  The block count of a segment follows
// from the launcher's rule for nt (decfuse.hip: cw_launch_gemv_stack / launch_stack_nt), restated here so that every pstats
// buffer can be sized, and the caller's idea of it checked, before the launch.
#define STACK_GUARD_FLOATS 1024
int32_t cw_test_gemv_stack(cw_ctx* c, const cw_test_gemv_stack_args* a) {
    if (!a) return fail(c, CW_ERR_INVALID, "test_gemv_stack: null arguments");
    if (!c->bf16) return fail(c, CW_ERR_INVALID, "test_gemv_stack: 16-bit engines only");
    const int Mb = a->Mb, K = a->K, nseg = a->nseg;
    if (Mb < 1 || Mb > 64 || K < 128 || K % 128 || K > 1280 || nseg < 1 || nseg > 3 || a->nt < 0 || a->nt > 3 || !a->W)
        return fail(c, CW_ERR_INVALID, "test_gemv_stack: Mb=%d K=%d nseg=%d nt=%d", Mb, K, nseg, a->nt);
    int tiles = 0;
    for (int s = 0; s < nseg; ++s) {
        const cw_test_stack_seg& g = a->seg[s];
        if (g.n_tiles < 1 || g.n_tiles > 4096 || g.nt < 0 || g.nt > 3 || g.epi < 0 || g.epi > 2 || !g.x || !g.out)
            return fail(c, CW_ERR_INVALID, "test_gemv_stack: segment %d n_tiles=%d nt=%d epi=%d", s, g.n_tiles, g.nt, g.epi);
        if (g.epi == 1 ? (!g.resid || g.wsum) : (g.resid || g.out2 || g.pstats))
            return fail(c, CW_ERR_INVALID, "test_gemv_stack: segment %d: a buffer its epilogue %d does not use, or no resid", s, g.epi);
        for (int t = 0; t < s; ++t)
            if (a->seg[t].out == g.out && (g.epi != 2 || a->seg[t].epi != 2 || a->seg[t].n_tiles != g.n_tiles))
                return fail(c, CW_ERR_INVALID, "test_gemv_stack: segments %d and %d share `out`", t, s);
        tiles += g.n_tiles;
    }
    // the launcher's nt: 0 = the smallest of 1 .. 3 that keeps the launch within 256 blocks; a segment's own nt where it is smaller
    int nt = a->nt;
    if (nt <= 0) {
        for (nt = 1;; ++nt) {
            int blocks = 0;
            for (int s = 0; s < nseg; ++s) {
                const int snt = a->seg[s].nt > 0 && a->seg[s].nt < nt ? a->seg[s].nt : nt;
                blocks += (a->seg[s].n_tiles + snt - 1) / snt;
            }
            if (blocks <= 256 || nt == 3) break;
        }
    }
    int seg_blocks[3] = {0, 0, 0}, blocks = 0;
    for (int s = 0; s < nseg; ++s) {
        const int snt = a->seg[s].nt > 0 && a->seg[s].nt < nt ? a->seg[s].nt : nt;
        seg_blocks[s] = (a->seg[s].n_tiles + snt - 1) / snt;
        blocks += seg_blocks[s];
        if (a->seg[s].pstats && a->seg[s].pstats_blocks != seg_blocks[s])
            return fail(c, CW_ERR_INVALID, "test_gemv_stack: segment %d has %d blocks, pstats_blocks=%d", s, seg_blocks[s], a->seg[s].pstats_blocks);
    }
    if (a->zero && (a->zero_n4 < 1 || (long long)blocks * 256 < a->zero_n4))
        return fail(c, CW_ERR_INVALID, "test_gemv_stack: zero_n4=%d with %d blocks", a->zero_n4, blocks);
    const int groups = (Mb + 15) / 16;
    const size_t e = c->esz, nW = (size_t)tiles * 16 * K;
    DevScope mem;
    void *dW = nullptr, *dWp = nullptr;
    HIPCHK(c, mem.get(&dW, nW * e));
    CWCHK(c, upload_T(c, dW, 0, a->W, nW));
    if (a->wpk) {
        HIPCHK(c, mem.get(&dWp, KD(c, cw_wfrag_elems, tiles * 16, K) * e));
        CWCHK(c, KD(c, cw_launch_wfrag_pack, dW, tiles * 16, K, dWp, c->st));
    }
    auto up = [&](float** d, const float* h, size_t n, size_t guard = 0) -> int {
        HIPCHK(c, mem.get(d, (n + guard) * 4));
        HIPCHK(c, hipMemcpy(*d, h, n * 4, hipMemcpyHostToDevice));
        if (guard) HIPCHK(c, hipMemset(*d + n, 0xFF, guard * 4));
        return CW_OK;
    };
    StackParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.W = a->wpk ? dWp : dW; sp.wpk = a->wpk ? 1 : 0; sp.wnt = (!c->sw.no_wnt && !g_test_no_wnt) ? 1 : 0; sp.K = K; sp.Mb = Mb; sp.nseg = nseg;
    float *dout[3] = {}, *dout2[3] = {}, *dps[3] = {}, *dzero = nullptr;
    int tile0 = 0;
    for (int s = 0; s < nseg; ++s) {
        const cw_test_stack_seg& g = a->seg[s];
        const size_t n = (size_t)g.n_tiles * 16, no = (size_t)Mb * n;
        float *dx = nullptr, *db = nullptr, *dws = nullptr, *dr = nullptr;
        CWCHK(c, up(&dx, g.x, (size_t)Mb * K));
        if (g.bias) CWCHK(c, up(&db, g.bias, n));
        if (g.wsum) CWCHK(c, up(&dws, g.wsum, n));
        if (g.resid) CWCHK(c, up(&dr, g.resid, no));
        for (int t = 0; t < s; ++t) if (a->seg[t].out == g.out) dout[s] = dout[t];   // the two accumulating halves of X2
        if (!dout[s]) CWCHK(c, up(&dout[s], g.out, no));
        if (g.out2) CWCHK(c, up(&dout2[s], g.out2, no));
        if (g.pstats) CWCHK(c, up(&dps[s], g.pstats, (size_t)groups * seg_blocks[s] * 32, STACK_GUARD_FLOATS));
        StackSeg& q = sp.seg[s];
        q.x = dx; q.bias = db; q.wsum = dws; q.resid = dr; q.out = dout[s]; q.out2 = dout2[s]; q.pstats = dps[s];
        q.tile0 = tile0; q.n_tiles = g.n_tiles; q.nt = g.nt; q.epi = g.epi;
        tile0 += g.n_tiles;
    }
    if (a->zero) { CWCHK(c, up(&dzero, a->zero, (size_t)a->zero_n4 * 4)); sp.zero = dzero; sp.zero_n4 = a->zero_n4; }
    int r = KD(c, cw_launch_gemv_stack, sp, a->nt, c->st);
    if (r != CW_OK) {
        hipStreamSynchronize(c->st);
        return fail(c, r, "test_gemv_stack: launch rejected (Mb=%d K=%d nseg=%d nt=%d)", Mb, K, nseg, a->nt);
    }
    { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_gemv_stack: %s", hipGetErrorString(er)); }
    { hipError_t er = hipGetLastError(); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_gemv_stack: %s", hipGetErrorString(er)); }
    for (int s = 0; s < nseg; ++s) {
        const cw_test_stack_seg& g = a->seg[s];
        const size_t no = (size_t)Mb * g.n_tiles * 16;
        HIPCHK(c, hipMemcpy(g.out, dout[s], no * 4, hipMemcpyDeviceToHost));
        if (g.out2) HIPCHK(c, hipMemcpy(g.out2, dout2[s], no * 4, hipMemcpyDeviceToHost));
        if (g.pstats) {
            const size_t np = (size_t)groups * seg_blocks[s] * 32;
            HIPCHK(c, hipMemcpy(g.pstats, dps[s], np * 4, hipMemcpyDeviceToHost));
            std::vector<unsigned int> guard(STACK_GUARD_FLOATS);
            HIPCHK(c, hipMemcpy(guard.data(), dps[s] + np, (size_t)STACK_GUARD_FLOATS * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < guard.size(); ++i)
                if (guard[i] != 0xFFFFFFFFu) { return fail(c, CW_ERR_STATE, "test_gemv_stack: segment %d wrote behind its pstats planes (guard element %zu)", s, i); }
        }
    }
    if (a->zero) HIPCHK(c, hipMemcpy(a->zero, dzero, (size_t)a->zero_n4 * 16, hipMemcpyDeviceToHost));
    return CW_OK;
}

// One call of a launcher of the decode GEMV dispatcher (include/crisperwhisper.h) with the arguments decode_step / gemv_ln give
// it.  Every device output is followed by GEMV_EPI_GUARD bytes of 0xFF; fragment-major outputs are filled with 0xA5 bytes in their
// pad rows.  The scratch and every fragment-major operand hold 64 rows: gemv_mt_kernel's row-group blocks request the row tiles of
// both groups whatever Mb is (as decode_step's d_xfrag does).
#define GEMV_EPI_GUARD 4096
int32_t cw_test_gemv_epi(cw_ctx* c, const cw_test_gemv_epi_args* a) {
    if (!a) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null arguments");
    const int op = a->op, epi = a->epi, Mb = a->Mb, N = a->N, K = a->K;
    if (op < 0 || op > 3) return fail(c, CW_ERR_INVALID, "test_gemv_epi: op %d", op);
    const bool comb = a->part_o || a->part_ml;
    if (!c->bf16 && !(op == 0 && (epi == EPI_RESID_F32 || epi == EPI_STORE_F32 || epi == EPI_QKV_CACHE || epi == EPI_GELU_F32) && !a->ln_g &&
                      !a->ln_b && !comb && !a->wpk && !a->x16 && !a->frag_in))
        return fail(c, CW_ERR_INVALID, "test_gemv_epi: the f32 engine takes op 0 with epi 2 / 5 / 6 / 7 on plain rows and row-major weights only");
    if (Mb < 1 || N < 1 || K < 1) return fail(c, CW_ERR_INVALID, "test_gemv_epi: size < 1 (Mb=%d N=%d K=%d)", Mb, N, K);
    if (Mb > 64) return fail(c, CW_ERR_INVALID, "test_gemv_epi: Mb=%d > 64", Mb);
    if (K % 128 || K > 5120) return fail(c, CW_ERR_INVALID, "test_gemv_epi: K=%d is not a multiple of 128 up to 5120", K);
    if (N > 65536) return fail(c, CW_ERR_INVALID, "test_gemv_epi: N=%d > 65536", N);
    if (op != 1 && !a->W) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer W");
    const int H = a->H, cap = a->cap, dm = a->d_model;
    int ldo = a->ldo;
    if (comb || op == 1) {
        if (!a->part_o || !a->part_ml) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer (a combine takes part_o and part_ml)");
        if (H < 1 || H * 64 != K) return fail(c, CW_ERR_INVALID, "test_gemv_epi: combine with H=%d, H * 64 != K=%d", H, K);
        if (a->ln_g) return fail(c, CW_ERR_INVALID, "test_gemv_epi: combine in front of a LayerNorm");
    }
    if (!a->out) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer out");
    if (op == 0) {
        if (epi != EPI_GELU && epi != EPI_RESID_F32 && epi != EPI_STORE_F32 && epi != EPI_QKV_CACHE && epi != EPI_GELU_F32 && epi != EPI_GELU_FRAG)
            return fail(c, CW_ERR_INVALID, "test_gemv_epi: epi %d", epi);
        if (!comb && !a->x) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer x");
        if (a->ln_b && !a->ln_g) return fail(c, CW_ERR_INVALID, "test_gemv_epi: ln_b without ln_g");
        if (epi != EPI_RESID_F32 && (a->inplace || a->resid)) return fail(c, CW_ERR_INVALID, "test_gemv_epi: inplace / resid with epi %d", epi);
        if (epi == EPI_RESID_F32 && !a->inplace && !a->resid) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer resid");
        if (epi == EPI_RESID_F32 && a->inplace && a->resid) return fail(c, CW_ERR_INVALID, "test_gemv_epi: inplace with a separate resid");
        if (a->frag_in && comb) return fail(c, CW_ERR_INVALID, "test_gemv_epi: frag_in with a combine");
        if (epi == EPI_QKV_CACHE) {
            if (dm < 64 || dm % 64) return fail(c, CW_ERR_INVALID, "test_gemv_epi: d_model=%d %% 64", dm);
            if (N != 3 * dm) return fail(c, CW_ERR_INVALID, "test_gemv_epi: N=%d != 3 d_model=%d", N, 3 * dm);
            if (H * 64 != dm) return fail(c, CW_ERR_INVALID, "test_gemv_epi: H=%d, H * 64 != d_model=%d", H, dm);
            if (cap < 1 || cap > 8192) return fail(c, CW_ERR_INVALID, "test_gemv_epi: cap=%d", cap);
            if (!a->pos || !a->sk || !a->sv) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer (epi 6 takes pos, sk and sv)");
            for (int b = 0; b < Mb; ++b)
                if (a->pos[b] < 0 || a->pos[b] >= cap) return fail(c, CW_ERR_INVALID, "test_gemv_epi: pos[%d]=%d outside [0, cap=%d)", b, a->pos[b], cap);
            ldo = dm;
        } else if (epi == EPI_GELU_FRAG) {
            if (ldo != N) return fail(c, CW_ERR_INVALID, "test_gemv_epi: epi 8 takes ldo == N (ldo=%d N=%d)", ldo, N);
        } else if (ldo < N) return fail(c, CW_ERR_INVALID, "test_gemv_epi: ldo=%d < N=%d", ldo, N);
    } else if (op == 1) {
        if (a->pstats ? (!a->cvec || a->n_pstats < 1 || a->n_pstats > 256) : (a->cvec != nullptr))
            return fail(c, CW_ERR_INVALID, "test_gemv_epi: op 1 takes pstats with n_pstats in 1 .. 256 (%d) and cvec, or neither", a->n_pstats);
    } else if (op == 2) {
        if (!a->x || !a->cvec_in || !a->y || !a->stats) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer (op 2 takes x, cvec_in, y and stats)");
    } else {
        if (!a->x || !a->stats_in || !a->wsum) return fail(c, CW_ERR_INVALID, "test_gemv_epi: null buffer (op 3 takes x, stats_in and wsum)");
        if (a->n_stats < 1) return fail(c, CW_ERR_INVALID, "test_gemv_epi: n_stats=%d < 1", a->n_stats);
    }
    const size_t e = c->esz;
    const int Mpad = (Mb + 15) & ~15;
    DevScope mem;
    struct Guarded { void* d; size_t bytes; const char* name; };
    std::vector<Guarded> guards;
    auto getg = [&](void** d, size_t bytes, const char* name) -> int {   // an output: guard bytes behind it
        HIPCHK(c, mem.get(d, bytes + GEMV_EPI_GUARD));
        HIPCHK(c, hipMemset((char*)*d + bytes, 0xFF, GEMV_EPI_GUARD));
        guards.push_back({*d, bytes, name});
        return CW_OK;
    };
    auto upf = [&](float** d, const float* h, size_t n) -> int {
        HIPCHK(c, mem.get(d, n * 4));
        HIPCHK(c, hipMemcpy(*d, h, n * 4, hipMemcpyHostToDevice));
        return CW_OK;
    };
    auto to16 = [&](float v) -> bf16_t { return c->f16 ? cw_host_f32_to_f16(v) : cw_host_f32_to_bf16(v); };
    auto from16 = [&](bf16_t v) -> float { return c->f16 ? cw_host_f16_to_f32(v) : cw_host_bf16_to_f32(v); };
    // host rows [rows][cols] -> a fragment-major 16-bit image of `prows` rows, every other element `fill`
    auto frag_up = [&](void* d, const float* h, int rows, int cols, int prows, unsigned short fill) -> int {
        std::vector<bf16_t> img((size_t)prows * cols, (bf16_t)fill);
        for (int m = 0; m < rows; ++m)
            for (int k = 0; k < cols; ++k) img[frag_index(m, k, cols)] = to16(h[(size_t)m * cols + k]);
        HIPCHK(c, hipMemcpy(d, img.data(), img.size() * 2, hipMemcpyHostToDevice));
        return CW_OK;
    };
    bool tail_ok = true;
    auto frag_down = [&](const void* d, float* h, int rows, int cols, int prows, unsigned short fill) -> int {
        std::vector<bf16_t> img((size_t)prows * cols);
        HIPCHK(c, hipMemcpy(img.data(), d, img.size() * 2, hipMemcpyDeviceToHost));
        for (int m = 0; m < prows; ++m)
            for (int k = 0; k < cols; ++k) {
                const bf16_t v = img[frag_index(m, k, cols)];
                if (m < rows) h[(size_t)m * cols + k] = from16(v);
                else if (v != (bf16_t)fill) tail_ok = false;
            }
        return CW_OK;
    };
    // weights
    void *dW = nullptr, *dWp = nullptr;
    if (op != 1) {
        HIPCHK(c, mem.get(&dW, (size_t)N * K * e));
        CWCHK(c, upload_T(c, dW, 0, a->W, (size_t)N * K));
        if (a->wpk) {
            HIPCHK(c, mem.get(&dWp, KD(c, cw_wfrag_elems, N, K) * e));
            CWCHK(c, KD(c, cw_launch_wfrag_pack, dW, N, K, dWp, c->st));
        }
    }
    const void* Wd = a->wpk ? dWp : dW;
    float *dbias = nullptr, *dg = nullptr, *dbeta = nullptr, *dpo = nullptr, *dml = nullptr;
    if (a->bias && op != 1) CWCHK(c, upf(&dbias, a->bias, (size_t)N));
    if (comb || op == 1) {
        CWCHK(c, upf(&dpo, a->part_o, (size_t)ATT_NS * Mb * K));
        CWCHK(c, upf(&dml, a->part_ml, (size_t)Mb * H * ATT_NS * 2));
    }
    void* dscr = nullptr;                                       // 64 fragment-major rows
    HIPCHK(c, mem.get(&dscr, (size_t)64 * K * 2));
    HIPCHK(c, hipMemset(dscr, 0, (size_t)64 * K * 2));
    int r = CW_OK;
    void *dout = nullptr, *dsk = nullptr, *dsv = nullptr, *dy = nullptr;
    float *dstats = nullptr, *dcvec = nullptr;
    int own_nt = 0, slots = 0;
    size_t ncache = 0;
    const unsigned short FILL = 0xA5A5;
    if (op == 0) {
        float* dx = nullptr; void* dx16 = nullptr;
        if (!comb) {
            if (a->frag_in) CWCHK(c, frag_up(dscr, a->x, Mb, K, 64, 0));
            else if (a->x16) { HIPCHK(c, mem.get(&dx16, (size_t)Mb * K * 2)); CWCHK(c, upload_T(c, dx16, 0, a->x, (size_t)Mb * K)); }
            else CWCHK(c, upf(&dx, a->x, (size_t)Mb * K));
        }
        if (a->ln_g) CWCHK(c, upf(&dg, a->ln_g, (size_t)K));
        if (a->ln_b) CWCHK(c, upf(&dbeta, a->ln_b, (size_t)K));
        EpiParams ep = epi0();
        ep.bias = dbias; ep.ldo = a->ldo; ep.x16 = a->x16 ? 1 : 0;
        if (epi == EPI_GELU) {
            CWCHK(c, getg(&dout, (size_t)Mb * ldo * 2, "out"));
            CWCHK(c, upload_T(c, dout, 0, a->out, (size_t)Mb * ldo));
            ep.out = dout;
        } else if (epi == EPI_GELU_FRAG) {
            CWCHK(c, getg(&dout, (size_t)Mpad * N * 2, "out"));
            CWCHK(c, frag_up(dout, a->out, Mb, N, Mpad, FILL));
            ep.out = dout;
        } else {
            CWCHK(c, getg(&dout, (size_t)Mb * ldo * 4, "out"));
            HIPCHK(c, hipMemcpy(dout, a->out, (size_t)Mb * ldo * 4, hipMemcpyHostToDevice));
            ep.outf = (float*)dout;
        }
        if (epi == EPI_RESID_F32) {
            if (a->inplace) ep.resid = (const float*)dout;
            else { float* dr = nullptr; CWCHK(c, upf(&dr, a->resid, (size_t)Mb * ldo)); ep.resid = dr; }
        }
        if (epi == EPI_QKV_CACHE) {
            int* dpos = nullptr;
            ncache = (size_t)Mb * H * cap * 64;
            HIPCHK(c, mem.get(&dpos, (size_t)Mb * 4));
            HIPCHK(c, hipMemcpy(dpos, a->pos, (size_t)Mb * 4, hipMemcpyHostToDevice));
            CWCHK(c, getg(&dsk, ncache * e, "sk")); CWCHK(c, getg(&dsv, ncache * e, "sv"));
            CWCHK(c, upload_T(c, dsk, 0, a->sk, ncache)); CWCHK(c, upload_T(c, dsv, 0, a->sv, ncache));
            ep.out1 = dsk; ep.out2 = dsv; ep.H = H; ep.S_pad = cap; ep.d_model = dm; ep.row_pos = dpos; ep.ldo = 0;
        }
        CombineParams cb{dml, H, Mb * K, nullptr, 0, nullptr};
        const float* xin = comb ? dpo : a->frag_in ? nullptr : a->x16 ? (const float*)dx16 : dx;
        const bool wpacked = c->bf16 && a->wpk;
        r = KD(c, cw_launch_gemv, c->bf16, epi, xin, Mb, K, Wd, N, dg, dbeta, ep, c->st, comb ? &cb : nullptr,
               (Mb <= 16 || wpacked) ? dscr : nullptr, wpacked, !c->sw.no_wnt && !g_test_no_wnt);
    } else if (op == 1) {
        CWCHK(c, getg(&dout, (size_t)Mpad * K * 2, "out"));
        CWCHK(c, frag_up(dout, a->out, Mb, K, Mpad, FILL));
        CombineParams cb{dml, H, Mb * K, nullptr, 0, nullptr};
        if (a->pstats) {
            float* dps = nullptr;
            CWCHK(c, upf(&dps, a->pstats, (size_t)(Mpad / 16) * a->n_pstats * 32));
            CWCHK(c, getg((void**)&dcvec, (size_t)Mb * 4, "cvec"));
            HIPCHK(c, hipMemcpy(dcvec, a->cvec, (size_t)Mb * 4, hipMemcpyHostToDevice));
            cb.pstats = dps; cb.n_pstats = a->n_pstats; cb.cvec_out = dcvec;
        }
        r = KD(c, cw_launch_rows_combine, dpo, Mb, K, cb, dout, c->st);
    } else if (op == 2) {
        own_nt = KD(c, cw_gemv_own_nt, N);
        slots = (N + 16 * own_nt - 1) / (16 * own_nt);
        if (a->nt) *a->nt = own_nt;
        float* dcin = nullptr;
        CWCHK(c, frag_up(dscr, a->x, Mb, K, 64, 0));
        CWCHK(c, upf(&dcin, a->cvec_in, (size_t)Mb));
        CWCHK(c, getg(&dout, (size_t)Mb * N * 4, "out"));
        HIPCHK(c, hipMemcpy(dout, a->out, (size_t)Mb * N * 4, hipMemcpyHostToDevice));
        CWCHK(c, getg(&dy, (size_t)Mpad * N * 2, "y"));
        CWCHK(c, frag_up(dy, a->y, Mb, N, Mpad, FILL));
        CWCHK(c, getg((void**)&dstats, (size_t)slots * 128 * 4, "stats"));
        HIPCHK(c, hipMemcpy(dstats, a->stats, (size_t)slots * 128 * 4, hipMemcpyHostToDevice));
        EpiParams ep = epi0();
        ep.outf = (float*)dout; ep.resid = (const float*)dout; ep.bias = dbias; ep.ldo = N;
        r = KD(c, cw_launch_gemv_own, dscr, Mb, K, Wd, N, ep, dcin, dy, dstats, c->st, a->wpk != 0);
    } else {
        float *dsi = nullptr, *dws = nullptr;
        CWCHK(c, frag_up(dscr, a->x, Mb, K, 64, 0));
        CWCHK(c, upf(&dsi, a->stats_in, (size_t)a->n_stats * 128));
        CWCHK(c, upf(&dws, a->wsum, (size_t)N));
        CWCHK(c, getg(&dout, (size_t)Mpad * N * 2, "out"));
        CWCHK(c, frag_up(dout, a->out, Mb, N, Mpad, FILL));
        EpiParams ep = epi0();
        ep.out = dout; ep.bias = dbias; ep.ldo = N;
        r = KD(c, cw_launch_gemv_lna, dscr, Mb, K, Wd, N, ep, dsi, a->n_stats, dws, c->st, a->wpk != 0);
    }
    if (r != CW_OK) {
        hipStreamSynchronize(c->st);
        return fail(c, r, "test_gemv_epi: launch rejected (op=%d epi=%d Mb=%d N=%d K=%d wpk=%d)", op, epi, Mb, N, K, a->wpk);
    }
    { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_gemv_epi: %s", hipGetErrorString(er)); }
    { hipError_t er = hipGetLastError(); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_gemv_epi: %s", hipGetErrorString(er)); }
    if (op == 0) {
        if (epi == EPI_GELU) CWCHK(c, download_T(c, dout, 0, a->out, (size_t)Mb * ldo));
        else if (epi == EPI_GELU_FRAG) CWCHK(c, frag_down(dout, a->out, Mb, N, Mpad, FILL));
        else HIPCHK(c, hipMemcpy(a->out, dout, (size_t)Mb * ldo * 4, hipMemcpyDeviceToHost));
        if (epi == EPI_QKV_CACHE) { CWCHK(c, download_T(c, dsk, 0, a->sk, ncache)); CWCHK(c, download_T(c, dsv, 0, a->sv, ncache)); }
    } else if (op == 1) {
        CWCHK(c, frag_down(dout, a->out, Mb, K, Mpad, FILL));
        if (dcvec) HIPCHK(c, hipMemcpy(a->cvec, dcvec, (size_t)Mb * 4, hipMemcpyDeviceToHost));
    } else if (op == 2) {
        HIPCHK(c, hipMemcpy(a->out, dout, (size_t)Mb * N * 4, hipMemcpyDeviceToHost));
        CWCHK(c, frag_down(dy, a->y, Mb, N, Mpad, FILL));
        HIPCHK(c, hipMemcpy(a->stats, dstats, (size_t)slots * 128 * 4, hipMemcpyDeviceToHost));
    } else {
        CWCHK(c, frag_down(dout, a->out, Mb, N, Mpad, FILL));
    }
    if (a->frag_tail_ok) *a->frag_tail_ok = tail_ok ? 1 : 0;
    std::vector<unsigned char> gb(GEMV_EPI_GUARD);
    for (const Guarded& g : guards) {
        HIPCHK(c, hipMemcpy(gb.data(), (const char*)g.d + g.bytes, GEMV_EPI_GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < gb.size(); ++i)
            if (gb[i] != 0xFF) return fail(c, CW_ERR_STATE, "test_gemv_epi: the launch wrote behind `%s` (guard byte %zu)", g.name, i);
    }
    return CW_OK;
}

// One launch of the decode self-attention dispatcher (cw_launch_attn_decode) on caller-supplied rows, parameters filled the way
// decode_step fills them: q [B][H*64] (already scaled), k / v [B / kv_div][H][cap][64]; per-row histories (n_keys = 0: pos[b] + 1
// keys) or a fixed n_keys (the f32 engine's cross-attention; pos[b] = alignment row).  anc [B][cap]: beam-search ancestry.
// out_frag: the kernel writes the 16-bit MFMA fragment-major buffer; it comes back un-permuted as [B][H*64] and *frag_tail_ok
// says whether its rows B .. 16-padded were left untouched.  align_head >= 0: that head is the only alignment slot; align
// [B][align_rows][n_keys] is uploaded as the initial contents and downloaded after the launch.  Every index the kernels can
// derive from the inputs is checked here, before anything is launched.
int32_t cw_test_self_attention(cw_ctx* c, int32_t B, int32_t H, int32_t cap, int32_t kv_div, const float* q, const float* k,
                               const float* v, const int32_t* pos, int32_t n_keys, const int32_t* anc, int32_t short_hist,
                               int32_t out_frag, int32_t align_head, int32_t align_rows, float* out, float* align,
                               int32_t* frag_tail_ok) {
    if (B < 1 || H < 1 || cap < 1 || cap > 8192 || kv_div < 1 || B % kv_div)
        return fail(c, CW_ERR_INVALID, "test_self_attention: shape B=%d H=%d cap=%d kv_div=%d", B, H, cap, kv_div);
    if (!q || !k || !v || !pos || !out || (out_frag && !frag_tail_ok)) return fail(c, CW_ERR_INVALID, "test_self_attention: null buffer");
    if (n_keys < 0 || n_keys > cap) return fail(c, CW_ERR_INVALID, "test_self_attention: n_keys=%d outside [0, cap=%d]", n_keys, cap);
    for (int b = 0; b < B; ++b)
        if (pos[b] < 0 || pos[b] >= cap) return fail(c, CW_ERR_INVALID, "test_self_attention: pos[%d]=%d outside [0, cap=%d)", b, pos[b], cap);
    if (anc) {
        if (kv_div > 1 || n_keys > 0 || align_head >= 0)
            return fail(c, CW_ERR_INVALID, "test_self_attention: anc with kv_div=%d / n_keys=%d / align_head=%d", kv_div, n_keys, align_head);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t <= pos[b]; ++t)
                if (anc[(size_t)b * cap + t] < 0 || anc[(size_t)b * cap + t] >= B)
                    return fail(c, CW_ERR_INVALID, "test_self_attention: anc[%d][%d]=%d outside [0, B=%d)", b, t, anc[(size_t)b * cap + t], B);
    }
    if (align_head < -1 || align_head >= H) return fail(c, CW_ERR_INVALID, "test_self_attention: align_head=%d", align_head);
    if (align_head >= 0) {   // the capture's row stride is n_keys: only defined for a fixed key count
        if (n_keys < 1 || align_rows < 1 || !align)
            return fail(c, CW_ERR_INVALID, "test_self_attention: alignment capture needs a fixed n_keys (%d) and align_rows (%d)", n_keys, align_rows);
        for (int b = 0; b < B; ++b)
            if (pos[b] >= align_rows) return fail(c, CW_ERR_INVALID, "test_self_attention: pos[%d]=%d >= align_rows=%d", b, pos[b], align_rows);
    }
    const int D = H * 64, Mpad = (B + 15) & ~15;
    const size_t nkv = (size_t)(B / kv_div) * H * cap * 64, nal = align_head >= 0 ? (size_t)B * align_rows * n_keys : 0;
    float *dq = nullptr, *dout = nullptr, *dal = nullptr;
    void *dk = nullptr, *dv = nullptr;
    int *dpos = nullptr, *danc = nullptr, *dslot = nullptr;
    unsigned short* dfrag = nullptr;
    DevScope mem;
    HIPCHK(c, mem.get(&dq, (size_t)B * D * 4)); HIPCHK(c, mem.get(&dk, nkv * c->esz)); HIPCHK(c, mem.get(&dv, nkv * c->esz));
    HIPCHK(c, mem.get(&dpos, (size_t)B * 4)); HIPCHK(c, mem.get(&dout, (size_t)B * D * 4));
    HIPCHK(c, hipMemcpy(dq, q, (size_t)B * D * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dpos, pos, (size_t)B * 4, hipMemcpyHostToDevice));
    CWCHK(c, upload_T(c, dk, 0, k, nkv)); CWCHK(c, upload_T(c, dv, 0, v, nkv));
    DecAttnParams p = dec_attn(dq, dk, dv, cap, n_keys, dpos, dout, B, H);
    p.kv_div = kv_div; p.short_hist = short_hist ? 1 : 0;
    if (anc) {
        HIPCHK(c, mem.get(&danc, (size_t)B * cap * 4));
        HIPCHK(c, hipMemcpy(danc, anc, (size_t)B * cap * 4, hipMemcpyHostToDevice));
        p.anc = danc;
    }
    if (out_frag) {
        HIPCHK(c, mem.get(&dfrag, (size_t)Mpad * D * 2));
        HIPCHK(c, hipMemsetAsync(dfrag, 0xA5, (size_t)Mpad * D * 2, c->st));
        p.out_frag = dfrag;
    }
    if (align_head >= 0) {
        std::vector<int> slot(H, -1);
        slot[align_head] = 0;
        HIPCHK(c, mem.get(&dal, nal * 4)); HIPCHK(c, mem.get(&dslot, (size_t)H * 4));
        HIPCHK(c, hipMemcpy(dal, align, nal * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(dslot, slot.data(), (size_t)H * 4, hipMemcpyHostToDevice));
        p.align_out = dal; p.align_slot = dslot; p.n_align = 1; p.align_rows = align_rows;
    }
    int r = KD(c, cw_launch_attn_decode, c->bf16, p, c->st);
    if (r != CW_OK) return fail(c, r, "test_self_attention: launch rejected");
    { hipError_t er = hipStreamSynchronize(c->st); if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_self_attention: %s", hipGetErrorString(er)); }
    if (out_frag) {
        std::vector<unsigned short> f((size_t)Mpad * D);
        HIPCHK(c, hipMemcpy(f.data(), dfrag, f.size() * 2, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < D; ++j) {
                const unsigned short h = f[frag_index(b, j, D)];
                out[(size_t)b * D + j] = c->f16 ? cw_host_f16_to_f32(h) : cw_host_bf16_to_f32(h);
            }
        int ok = 1;
        for (int b = B; b < Mpad; ++b)
            for (int j = 0; j < D; ++j) ok &= f[frag_index(b, j, D)] == 0xA5A5;
        *frag_tail_ok = ok;
    } else {
        HIPCHK(c, hipMemcpy(out, dout, (size_t)B * D * 4, hipMemcpyDeviceToHost));
    }
    if (align_head >= 0) HIPCHK(c, hipMemcpy(align, dal, nal * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// The beam-search state of the first `rows` rows after cw_beam_begin / cw_beam_advance: token history ids [rows][TGT], cache
// ancestry anc [rows][TGT] and decoder input position pos [rows], as the device holds them.
int32_t cw_test_beam_state(cw_ctx* c, int32_t rows, int32_t* ids, int32_t* anc, int32_t* pos) {
    const int TGT = c->d.max_target_positions;
    if (c->beam_K <= 0 || !c->d_anc) return fail(c, CW_ERR_STATE, "cw_beam_begin not called");
    if (rows < 1 || rows > c->Bm || rows > 64 || !ids || !anc || !pos) return fail(c, CW_ERR_INVALID, "test_beam_state: rows=%d", rows);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(ids, c->d_ids, (size_t)rows * TGT * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(anc, c->d_anc, (size_t)rows * TGT * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(pos, c->d_pos, (size_t)rows * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// One launch of the beam-search candidate selection, exactly as cw_beam_step launches it (launch_beam_topk), on caller-supplied
// rows: logits [nb][V] raw f32, ids [nb][t] = prompt + generated so far.  The pad columns V .. Vpad-1 hold +75 during the call, the
// candidate buffers are filled with 0xff bytes and every float of the slice-record scratch with 1e30 beforehand: a pad column that
// counted, a stale or unwritten list entry would win every selection.  cand_val / cand_id [max_batch * 64]: the WHOLE candidate
// buffers as the device holds them afterwards ([nb][n_cand] written, 0xff behind).
int32_t cw_test_beam_topk(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                          int32_t min_new_tokens, int32_t n_cand, float* cand_val, int32_t* cand_id) {
    const int V = c->d.vocab_size, TGT = c->d.max_target_positions, Bm = c->Bm;
    if (!logits || !ids || !cand_val || !cand_id) return fail(c, CW_ERR_INVALID, "test_beam_topk: null argument");
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (c->beam_K > 0) return fail(c, CW_ERR_STATE, "test_beam_topk: a beam search is open (the hook overwrites its state)");
    if (nb < 1 || nb > Bm || nb > 64) return fail(c, CW_ERR_INVALID, "test_beam_topk: nb=%d outside 1 .. %d", nb, Bm < 64 ? Bm : 64);
    if (n_cand < 1 || n_cand > 64) return fail(c, CW_ERR_INVALID, "test_beam_topk: n_cand=%d outside 1 .. 64", n_cand);
    if (n_prompt < 1 || t < n_prompt || t >= TGT) return fail(c, CW_ERR_INVALID, "test_beam_topk: t=%d / n_prompt=%d out of range", t, n_prompt);
    if (min_new_tokens < 0) return fail(c, CW_ERR_INVALID, "test_beam_topk: min_new_tokens=%d is negative", min_new_tokens);
    std::vector<int> hid((size_t)nb * TGT, c->gen.pad_token_id), posv(nb, t - 1);
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < t; ++k) {
            const int tok = ids[(size_t)b * t + k];
            if (tok < 0 || tok >= V) return fail(c, CW_ERR_INVALID, "test_beam_topk: token %d out of range", tok);
            hid[(size_t)b * TGT + k] = tok;
        }
    CWCHK(c, beam_alloc(c));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(c->d_ids, hid.data(), hid.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_pos, posv.data(), (size_t)nb * 4, hipMemcpyHostToDevice));
    const int cfg[4] = {n_prompt, min_new_tokens, TGT, 0};
    HIPCHK(c, hipMemcpy(c->d_cfg, cfg, sizeof(cfg), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy2D(c->dlogits, (size_t)c->Vpad * 4, logits, (size_t)V * 4, (size_t)V * 4, nb, hipMemcpyHostToDevice));
    const int n_padcol = c->Vpad - V;
    if (n_padcol > 0) {                               // the pad columns hold +75 for this call: they must never count
        const std::vector<float> hot((size_t)nb * n_padcol, 75.0f);
        HIPCHK(c, hipMemcpy2D(c->dlogits + V, (size_t)c->Vpad * 4, hot.data(), (size_t)n_padcol * 4, (size_t)n_padcol * 4, nb, hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemset(c->d_cand_val, 0xff, (size_t)Bm * 64 * 4));
    HIPCHK(c, hipMemset(c->d_cand_id, 0xff, (size_t)Bm * 64 * 4));
    const std::vector<float> poison(KD(c, cw_beam_topk_scratch_floats, Bm), 1e30f);
    HIPCHK(c, hipMemcpy(c->d_topk_scratch, poison.data(), poison.size() * 4, hipMemcpyHostToDevice));
    const int r = launch_beam_topk(c, nb, n_cand);
    if (r != CW_OK) fail(c, r, "test_beam_topk: launch rejected");
    hipError_t er = hipStreamSynchronize(c->st);
    if (er == hipSuccess) er = hipGetLastError();
    if (n_padcol > 0) HIPCHK(c, hipMemset2D(c->dlogits + V, (size_t)c->Vpad * 4, 0, (size_t)n_padcol * 4, nb));
    if (r != CW_OK) return r;
    if (er != hipSuccess) return fail(c, CW_ERR_HIP, "test_beam_topk: %s", hipGetErrorString(er));
    HIPCHK(c, hipMemcpy(cand_val, c->d_cand_val, (size_t)Bm * 64 * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(cand_id, c->d_cand_id, (size_t)Bm * 64 * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// The decoder input rows of the next step as the device holds them: x [rows][d_model] (what cw_beam_advance / the sampler wrote).
// Read-only.
int32_t cw_test_beam_x(cw_ctx* c, int32_t rows, float* x) {
    if (rows < 1 || rows > c->Bm || !x) return fail(c, CW_ERR_INVALID, "test_beam_x: rows=%d", rows);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(x, c->dx, (size_t)rows * c->d.d_model * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// What the last decoder forward left on the device (differential tests of the decode step's launch plans):
//   what 0: the cross-query x term qa of the last layer that ran, [rows][d_model] f32 (fused layers only)
//   what 1 / 2: rows 0 .. n_pos - 1 of the self-attention key / value cache of `layer`, [rows][heads][n_pos][64] in the engine's element type
//   what 3: one int32, 1 when a forward of `rows` rows takes the x term in qkv_self_kernel and the two-segment stack launch (plan_step)
int32_t cw_test_decode_state(cw_ctx* c, int32_t what, int32_t layer, int32_t rows, int32_t n_pos, void* out) {
    const int D = c->d.d_model, H = c->d.n_heads, TGT = c->d.max_target_positions;
    if (!out || rows < 1 || rows > c->Bm || what < 0 || what > 3) return fail(c, CW_ERR_INVALID, "test_decode_state: what=%d rows=%d", what, rows);
    if (what == 3) { *(int32_t*)out = step_plan_xq(c, rows) ? 1 : 0; return CW_OK; }
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (what == 0) {
        HIPCHK(c, hipMemcpy(out, c->d_qa, (size_t)rows * D * 4, hipMemcpyDeviceToHost));
        return CW_OK;
    }
    if (layer < 0 || layer >= c->d.dec_layers || n_pos < 1 || n_pos > TGT) return fail(c, CW_ERR_INVALID, "test_decode_state: layer=%d n_pos=%d", layer, n_pos);
    const void* src = what == 1 ? c->dec[layer].sk : c->dec[layer].sv;
    const size_t row_bytes = (size_t)64 * c->esz;
    HIPCHK(c, hipMemcpy2D(out, (size_t)n_pos * row_bytes, src, (size_t)TGT * row_bytes, (size_t)n_pos * row_bytes, (size_t)rows * H, hipMemcpyDeviceToHost));
    return CW_OK;
}

// One call of the fused logits-processor + argmax kernel (sample_kernel) on caller-supplied rows: logits [nb][V],
// ids [nb][t] = prompt + generated so far (the kernel's grammar state is rebuilt from it), choice_out [nb] = the
// token the kernel picks for index t.  Differential test against TF/generation/logits_process.py:203-260, 1816-2047.
static int test_sample(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                       int32_t min_new_tokens, int32_t max_length, int32_t* choice_out, const int32_t* forced_tok = nullptr,
                       float* lp_out = nullptr, int32_t* top_id_out = nullptr, float* top_lp_out = nullptr, float* ent_out = nullptr);
int32_t cw_test_sample(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                       int32_t min_new_tokens, int32_t max_length, int32_t* choice_out) {
    return test_sample(c, nb, logits, ids, t, n_prompt, min_new_tokens, max_length, choice_out);
}
// The same two launches under a sampling setting of their own; the context's setting (cw_set_sampling) is put back afterwards.
int32_t cw_test_sample_seeded(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                              int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                              const uint64_t* row_streams, int32_t* choice_out) {
    if (!logits || !ids || !choice_out) return fail(c, CW_ERR_INVALID, "test_sample_seeded: null argument");
    if (nb < 1 || nb > c->Bm || nb > 64) return fail(c, CW_ERR_INVALID, "test_sample_seeded: nb=%d outside 1 .. %d", nb, c->Bm < 64 ? c->Bm : 64);
    if (max_length <= n_prompt || max_length > c->d.max_target_positions || min_new_tokens < 0)
        return fail(c, CW_ERR_INVALID, "test_sample_seeded: max_length=%d / min_new_tokens=%d out of range", max_length, min_new_tokens);
    if (temperature > 0.f && !row_streams) return fail(c, CW_ERR_INVALID, "test_sample_seeded: a positive temperature needs row_streams");
    const std::vector<unsigned int> keep = c->samp_host;
    CWCHK(c, write_sampling(c, temperature, seed, row_streams, nb, "test_sample_seeded"));
    const int r = test_sample(c, nb, logits, ids, t, n_prompt, min_new_tokens, max_length, choice_out);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(c->d_samp, keep.data(), keep.size() * 4, hipMemcpyHostToDevice));
    c->samp_host = keep;
    return r;
}
// ... and with the per-token log-probability store switched on for this call only: lp_out [nb] = what the kernels stored at
// [b][t]; forced_tok [nb] (or NULL; -1 = not forced) is written at t in place of the choice, choice_out stays the un-forced choice.
int32_t cw_test_sample_logprobs(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                                int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                                const uint64_t* row_streams, const int32_t* forced_tok, int32_t* choice_out, float* lp_out) {
    if (!logits || !ids || !choice_out || !lp_out) return fail(c, CW_ERR_INVALID, "test_sample_logprobs: null argument");
    if (nb < 1 || nb > c->Bm || nb > 64) return fail(c, CW_ERR_INVALID, "test_sample_logprobs: nb=%d outside 1 .. %d", nb, c->Bm < 64 ? c->Bm : 64);
    if (max_length <= n_prompt || max_length > c->d.max_target_positions || min_new_tokens < 0)
        return fail(c, CW_ERR_INVALID, "test_sample_logprobs: max_length=%d / min_new_tokens=%d out of range", max_length, min_new_tokens);
    if (temperature > 0.f && !row_streams) return fail(c, CW_ERR_INVALID, "test_sample_logprobs: a positive temperature needs row_streams");
    if (forced_tok)
        for (int b = 0; b < nb; ++b)
            if (forced_tok[b] >= c->d.vocab_size) return fail(c, CW_ERR_INVALID, "test_sample_logprobs: forced token %d out of range", forced_tok[b]);
    const bool was_on = c->tok_lp_on;
    CWCHK(c, cw_set_token_logprobs(c, 1));
    const std::vector<unsigned int> keep = c->samp_host;
    CWCHK(c, write_sampling(c, temperature, seed, row_streams, nb, "test_sample_logprobs"));
    const int r = test_sample(c, nb, logits, ids, t, n_prompt, min_new_tokens, max_length, choice_out, forced_tok, lp_out);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(c->d_samp, keep.data(), keep.size() * 4, hipMemcpyHostToDevice));
    c->samp_host = keep;
    if (!was_on) CWCHK(c, cw_set_token_logprobs(c, 0));
    return r;
}
// ... and with the alternatives on as well: k = 1 .. CW_TOP_LOGPROBS_MAX, top_id_out / top_lp_out [nb][k] = what the kernels stored
// at [b][t][0 .. k-1].  The context's settings are restored afterwards.
int32_t cw_test_sample_top_logprobs(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                                    int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                                    const uint64_t* row_streams, const int32_t* forced_tok, int32_t k, int32_t* choice_out,
                                    float* lp_out, int32_t* top_id_out, float* top_lp_out) {
    if (!logits || !ids || !choice_out || !lp_out || !top_id_out || !top_lp_out) return fail(c, CW_ERR_INVALID, "test_sample_top_logprobs: null argument");
    if (k < 1 || k > CW_TOP_LOGPROBS_MAX) return fail(c, CW_ERR_INVALID, "test_sample_top_logprobs: k=%d outside 1 .. %d", k, CW_TOP_LOGPROBS_MAX);
    if (nb < 1 || nb > c->Bm || nb > 64) return fail(c, CW_ERR_INVALID, "test_sample_top_logprobs: nb=%d outside 1 .. %d", nb, c->Bm < 64 ? c->Bm : 64);
    if (max_length <= n_prompt || max_length > c->d.max_target_positions || min_new_tokens < 0)
        return fail(c, CW_ERR_INVALID, "test_sample_top_logprobs: max_length=%d / min_new_tokens=%d out of range", max_length, min_new_tokens);
    if (temperature > 0.f && !row_streams) return fail(c, CW_ERR_INVALID, "test_sample_top_logprobs: a positive temperature needs row_streams");
    if (forced_tok)
        for (int b = 0; b < nb; ++b)
            if (forced_tok[b] >= c->d.vocab_size) return fail(c, CW_ERR_INVALID, "test_sample_top_logprobs: forced token %d out of range", forced_tok[b]);
    const bool was_on = c->tok_lp_on;
    const int was_k = c->top_k;
    CWCHK(c, cw_set_token_logprobs(c, 1));
    CWCHK(c, cw_set_top_logprobs(c, k));
    const std::vector<unsigned int> keep = c->samp_host;
    CWCHK(c, write_sampling(c, temperature, seed, row_streams, nb, "test_sample_top_logprobs"));
    const int r = test_sample(c, nb, logits, ids, t, n_prompt, min_new_tokens, max_length, choice_out, forced_tok, lp_out, top_id_out, top_lp_out);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(c->d_samp, keep.data(), keep.size() * 4, hipMemcpyHostToDevice));
    c->samp_host = keep;
    CWCHK(c, cw_set_top_logprobs(c, was_on ? was_k : 0));
    if (!was_on) CWCHK(c, cw_set_token_logprobs(c, 0));
    return r;
}
// ... and with the token entropy on for this call (cw_set_token_entropy): ent_out [nb] = what the kernels stored at [b][t].  k = 0 ..
// CW_TOP_LOGPROBS_MAX: the alternatives ride along (top_id_out / top_lp_out [nb][k], NULL when k = 0), so that every instantiation
// the entropy joins can be driven.  The pad columns of the logits hold +75 during the call.  The context's settings are restored.
int32_t cw_test_sample_entropy(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                               int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                               const uint64_t* row_streams, const int32_t* forced_tok, int32_t k, int32_t* choice_out,
                               float* lp_out, float* ent_out, int32_t* top_id_out, float* top_lp_out) {
    if (!logits || !ids || !choice_out || !lp_out || !ent_out) return fail(c, CW_ERR_INVALID, "test_sample_entropy: null argument");
    if (k < 0 || k > CW_TOP_LOGPROBS_MAX || (k > 0 && (!top_id_out || !top_lp_out)))
        return fail(c, CW_ERR_INVALID, "test_sample_entropy: k=%d outside 0 .. %d, or no room for the alternatives", k, CW_TOP_LOGPROBS_MAX);
    if (nb < 1 || nb > c->Bm || nb > 64) return fail(c, CW_ERR_INVALID, "test_sample_entropy: nb=%d outside 1 .. %d", nb, c->Bm < 64 ? c->Bm : 64);
    if (max_length <= n_prompt || max_length > c->d.max_target_positions || min_new_tokens < 0)
        return fail(c, CW_ERR_INVALID, "test_sample_entropy: max_length=%d / min_new_tokens=%d out of range", max_length, min_new_tokens);
    if (temperature > 0.f && !row_streams) return fail(c, CW_ERR_INVALID, "test_sample_entropy: a positive temperature needs row_streams");
    if (forced_tok)
        for (int b = 0; b < nb; ++b)
            if (forced_tok[b] >= c->d.vocab_size) return fail(c, CW_ERR_INVALID, "test_sample_entropy: forced token %d out of range", forced_tok[b]);
    const bool was_on = c->tok_lp_on, was_ent = c->tok_ent_on;
    const int was_k = c->top_k;
    CWCHK(c, cw_set_token_logprobs(c, 1));
    CWCHK(c, cw_set_top_logprobs(c, k));
    CWCHK(c, cw_set_token_entropy(c, 1));
    const std::vector<unsigned int> keep = c->samp_host;
    CWCHK(c, write_sampling(c, temperature, seed, row_streams, nb, "test_sample_entropy"));
    const int r = test_sample(c, nb, logits, ids, t, n_prompt, min_new_tokens, max_length, choice_out, forced_tok, lp_out,
                              k > 0 ? top_id_out : nullptr, k > 0 ? top_lp_out : nullptr, ent_out);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(c->d_samp, keep.data(), keep.size() * 4, hipMemcpyHostToDevice));
    c->samp_host = keep;
    CWCHK(c, cw_set_token_entropy(c, was_ent ? 1 : 0));
    CWCHK(c, cw_set_top_logprobs(c, was_on ? was_k : 0));
    if (!was_on) CWCHK(c, cw_set_token_logprobs(c, 0));
    return r;
}
// ... and with a sequence_bias table for this call only; proc_lp_out [nb] = what the step added to the processed-score sum.
int32_t cw_test_sample_biased(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                              int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                              const uint64_t* row_streams, const int32_t* forced_tok, int32_t k, int32_t n_seq,
                              const int32_t* seq_tokens, const int32_t* seq_lengths, const float* seq_bias, int32_t* choice_out,
                              float* lp_out, int32_t* top_id_out, float* top_lp_out, float* proc_lp_out) {
    if (!proc_lp_out) return fail(c, CW_ERR_INVALID, "test_sample_biased: null argument");
    if (c->beam_K > 0) return fail(c, CW_ERR_STATE, "test_sample_biased: a beam search is open");
    std::vector<int> tab;
    CWCHK(c, seq_bias_table(c, n_seq, seq_tokens, seq_lengths, seq_bias, &tab, "test_sample_biased"));
    const std::vector<int> keep = c->sb_host;
    const int keep_n = c->sb_n;
    const bool keep_score = c->score_tokens;
    CWCHK(c, seq_bias_install(c, tab, n_seq));
    c->score_tokens = true;
    HIPCHK(c, hipMemset(c->d_lp_sum, 0, (size_t)c->Bm * 4));
    HIPCHK(c, hipMemset(c->d_lp_cnt, 0, (size_t)c->Bm * 4));
    const int r = cw_test_sample_top_logprobs(c, nb, logits, ids, t, n_prompt, min_new_tokens, max_length, temperature, seed, row_streams,
                                              forced_tok, k, choice_out, lp_out, top_id_out, top_lp_out);
    c->score_tokens = keep_score;
    int r2 = CW_OK;
    if (r == CW_OK) {
        hipError_t e = hipMemcpy(proc_lp_out, c->d_lp_sum, (size_t)nb * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r2 = fail(c, CW_ERR_HIP, "test_sample_biased: %s", hipGetErrorString(e));
    }
    drop_step_graphs(c);                                       // (cw_set_top_logprobs dropped them already)
    CWCHK(c, seq_bias_install(c, keep, keep_n));
    return r != CW_OK ? r : r2;
}
static int test_sample(cw_ctx* c, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                       int32_t min_new_tokens, int32_t max_length, int32_t* choice_out, const int32_t* forced_tok, float* lp_out,
                       int32_t* top_id_out, float* top_lp_out, float* ent_out) {
    const int V = c->d.vocab_size, TGT = c->d.max_target_positions;
    if (!c->gen_set) return fail(c, CW_ERR_STATE, "cw_set_generation not called");
    if (nb < 1 || nb > c->Bm || t < n_prompt || t < 1 || t >= TGT || n_prompt < 1) return fail(c, CW_ERR_INVALID, "test_sample: bad args");
    const int tb = c->gen.no_timestamps_token_id + 1;
    std::vector<int> hid((size_t)nb * TGT, c->gen.pad_token_id), last(nb, -1), posv(64, t - 1);
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < t; ++k) {
            const int tok = ids[(size_t)b * t + k];
            if (tok < 0 || tok >= V) return fail(c, CW_ERR_INVALID, "test_sample: token %d out of range", tok);
            hid[(size_t)b * TGT + k] = tok;
            if (k >= n_prompt && tok >= tb) last[b] = tok;
        }
    HIPCHK(c, hipMemcpy(c->d_ids, hid.data(), hid.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_last_ts, last.data(), nb * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_pos, posv.data(), 64 * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->d_finished, 0, nb * 4));
    HIPCHK(c, hipMemset(c->d_argmax, 0xff, (size_t)nb * TGT * 4));
    if (forced_tok) {
        std::vector<int> fr((size_t)nb * TGT, -1);
        for (int b = 0; b < nb; ++b) fr[(size_t)b * TGT + t] = forced_tok[b];
        HIPCHK(c, hipMemcpy(c->d_forced, fr.data(), fr.size() * 4, hipMemcpyHostToDevice));
    }
    if (lp_out) HIPCHK(c, hipMemset(c->d_tok_lp, 0xff, (size_t)nb * TGT * 4));
    if (ent_out) HIPCHK(c, hipMemset(c->d_tok_ent, 0xff, (size_t)nb * TGT * 4));
    if (top_id_out) {
        HIPCHK(c, hipMemset(c->d_top_id, 0xff, (size_t)nb * TGT * CW_TOP_LOGPROBS_MAX * 4));
        HIPCHK(c, hipMemset(c->d_top_lp, 0xff, (size_t)nb * TGT * CW_TOP_LOGPROBS_MAX * 4));
    }
    const int cfg[4] = {n_prompt, min_new_tokens, max_length, forced_tok ? 1 : 0};
    HIPCHK(c, hipMemcpy(c->d_cfg, cfg, sizeof(cfg), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy2D(c->dlogits, (size_t)c->Vpad * 4, logits, (size_t)V * 4, (size_t)V * 4, nb, hipMemcpyHostToDevice));
    const int n_padcol = c->Vpad - V;
    const bool hot_pad = (top_id_out || ent_out) && n_padcol > 0;
    if (hot_pad) {                                    // the pad columns hold +75 for this call: they must never count
        const std::vector<float> hot((size_t)nb * n_padcol, 75.0f);
        HIPCHK(c, hipMemcpy2D(c->dlogits + V, (size_t)c->Vpad * 4, hot.data(), (size_t)n_padcol * 4, (size_t)n_padcol * 4, nb, hipMemcpyHostToDevice));
    }
    CWCHK(c, launch_sample(c, nb));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (hot_pad) HIPCHK(c, hipMemset2D(c->dlogits + V, (size_t)c->Vpad * 4, 0, (size_t)n_padcol * 4, nb));
    std::vector<int> am((size_t)nb * TGT);
    HIPCHK(c, hipMemcpy(am.data(), c->d_argmax, am.size() * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < nb; ++b) choice_out[b] = am[(size_t)b * TGT + t];
    if (lp_out) {
        std::vector<float> lp((size_t)nb * TGT);
        HIPCHK(c, hipMemcpy(lp.data(), c->d_tok_lp, lp.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < nb; ++b) lp_out[b] = lp[(size_t)b * TGT + t];
    }
    if (ent_out) {
        std::vector<float> en((size_t)nb * TGT);
        HIPCHK(c, hipMemcpy(en.data(), c->d_tok_ent, en.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < nb; ++b) ent_out[b] = en[(size_t)b * TGT + t];
    }
    if (top_id_out) {
        const int k = c->top_k;
        std::vector<int> ti((size_t)nb * TGT * k); std::vector<float> tl(ti.size());
        CWCHK(c, cw_get_top_logprobs(c, ti.data(), tl.data(), nb));
        for (int b = 0; b < nb; ++b) {
            memcpy(top_id_out + (size_t)b * k, &ti[((size_t)b * TGT + t) * k], (size_t)k * 4);
            memcpy(top_lp_out + (size_t)b * k, &tl[((size_t)b * TGT + t) * k], (size_t)k * 4);
        }
    }
    return CW_OK;
}

int32_t cw_test_language_probs(cw_ctx* c, const float* logits, int32_t nb, const int32_t* lang_ids, int32_t n_lang,
                               int32_t nospeech_token, int32_t* best, float* prob, float* no_speech) {
    const int V = c->d.vocab_size;
    if (!logits || !best) return fail(c, CW_ERR_INVALID, "test_language_probs: null argument");
    if (nb < 1 || nb > c->Bm) return fail(c, CW_ERR_INVALID, "test_language_probs: nb=%d outside 1 .. %d", nb, c->Bm);
    if (nospeech_token < -1 || nospeech_token >= V) return fail(c, CW_ERR_INVALID, "test_language_probs: nospeech_token %d out of range", nospeech_token);
    if (c->beam_K > 0) return fail(c, CW_ERR_STATE, "test_language_probs: a beam search is open (the hook overwrites its logits)");
    CWCHK(c, check_lang_ids(c, "test_language_probs", lang_ids, n_lang));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy2D(c->dlogits, (size_t)c->Vpad * 4, logits, (size_t)V * 4, (size_t)V * 4, nb, hipMemcpyHostToDevice));
    const int n_padcol = c->Vpad - V;
    if (n_padcol > 0) {                               // the pad columns hold +75 for this call: they must never count
        const std::vector<float> hot((size_t)nb * n_padcol, 75.0f);
        HIPCHK(c, hipMemcpy2D(c->dlogits + V, (size_t)c->Vpad * 4, hot.data(), (size_t)n_padcol * 4, (size_t)n_padcol * 4, nb, hipMemcpyHostToDevice));
    }
    const int r = language_probs(c, nb, lang_ids, n_lang, nospeech_token, best, prob, no_speech);
    if (n_padcol > 0) HIPCHK(c, hipMemset2D(c->dlogits + V, (size_t)c->Vpad * 4, 0, (size_t)n_padcol * 4, nb));
    return r;
}

// cw_test_align_similarity: the similarity kernel, through cw_align_heads' launcher, on caller-supplied normalised rows.
int32_t cw_test_align_similarity(cw_ctx* c, const float* attn, int32_t B, int32_t Ha, int32_t N, int32_t S, const int32_t* n_cols,
                                 const float* ref_begin, const float* ref_end, int32_t clip_frames, float* out) {
    if (!attn || !n_cols || !ref_begin || !ref_end || !out) return fail(c, CW_ERR_INVALID, "test_align_similarity: null argument");
    if (B < 1 || Ha < 1 || N < 1 || S < 4 || S % 4 || (size_t)B * Ha * N * S > ((size_t)1 << 28))
        return fail(c, CW_ERR_INVALID, "test_align_similarity: B=%d Ha=%d N=%d S=%d unsupported (S a multiple of 4, at most 2^28 elements)", B, Ha, N, S);
    for (int b = 0; b < B; ++b)
        if (n_cols[b] < 0 || n_cols[b] > S) return fail(c, CW_ERR_INVALID, "test_align_similarity: n_cols[%d]=%d outside 0 .. %d", b, n_cols[b], S);
    float *dw = nullptr, *db = nullptr, *de = nullptr, *dout = nullptr;
    int* dn = nullptr;
    const size_t nw = (size_t)B * Ha * N * S, nr = (size_t)B * N, no = (size_t)Ha * B * N;
    DevScope mem;
    if (mem.get(&dw, nw * 4) != hipSuccess || mem.get(&dn, (size_t)B * 4) != hipSuccess || mem.get(&db, nr * 4) != hipSuccess ||
        mem.get(&de, nr * 4) != hipSuccess || mem.get(&dout, no * 4) != hipSuccess)
        return fail(c, CW_ERR_NOMEM, "test_align_similarity: hipMalloc failed");
    HIPCHK(c, hipMemcpy(dw, attn, nw * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dn, n_cols, (size_t)B * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(db, ref_begin, nr * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(de, ref_end, nr * 4, hipMemcpyHostToDevice));
    CWCHK(c, cw_launch_align_similarity(dw, B, Ha, N, S, 0, N, dn, db, de, clip_frames, dout, c->st));
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(out, dout, no * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// cw_test_align_path_scores: the path-score kernel, through the timestamp stage's launcher, on caller-supplied rows.
int32_t cw_test_align_path_scores(cw_ctx* c, const float* attn, int32_t B, int32_t Ha, int32_t N, int32_t S, const int32_t* n_cols,
                                  const int32_t* first_col, int32_t collar_frames, float* mass, float* spread) {
    if (!attn || !n_cols || !first_col || !mass || !spread) return fail(c, CW_ERR_INVALID, "test_align_path_scores: null argument");
    if (B < 1 || Ha < 1 || N < 1 || S < 4 || S % 4 || (size_t)B * Ha * N * S > ((size_t)1 << 28))
        return fail(c, CW_ERR_INVALID, "test_align_path_scores: B=%d Ha=%d N=%d S=%d unsupported (S a multiple of 4, at most 2^28 elements)", B, Ha, N, S);
    if (collar_frames < 0) return fail(c, CW_ERR_INVALID, "test_align_path_scores: collar_frames=%d is negative", collar_frames);
    for (int b = 0; b < B; ++b) {
        if (n_cols[b] < 0 || n_cols[b] > S) return fail(c, CW_ERR_INVALID, "test_align_path_scores: n_cols[%d]=%d outside 0 .. %d", b, n_cols[b], S);
        for (int i = 0; i < N; ++i)
            if (first_col[(size_t)b * N + i] > S) return fail(c, CW_ERR_INVALID, "test_align_path_scores: first_col[%d][%d]=%d above %d", b, i, first_col[(size_t)b * N + i], S);
    }
    float *dw = nullptr, *dm = nullptr, *ds = nullptr;
    int *dn = nullptr, *df = nullptr;
    const size_t nw = (size_t)B * Ha * N * S, nr = (size_t)B * N;
    DevScope mem;
    if (mem.get(&dw, nw * 4) != hipSuccess || mem.get(&dn, (size_t)B * 4) != hipSuccess || mem.get(&df, nr * 4) != hipSuccess ||
        mem.get(&dm, nr * 4) != hipSuccess || mem.get(&ds, nr * 4) != hipSuccess)
        return fail(c, CW_ERR_NOMEM, "test_align_path_scores: hipMalloc failed");
    HIPCHK(c, hipMemcpy(dw, attn, nw * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dn, n_cols, (size_t)B * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(df, first_col, nr * 4, hipMemcpyHostToDevice));
    CWCHK(c, cw_launch_align_path_score(dw, B, Ha, N, S, 0, N, dn, df, collar_frames, dm, ds, c->st));
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(mass, dm, nr * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(spread, ds, nr * 4, hipMemcpyDeviceToHost));
    return CW_OK;
}

// ------------------------------------------------------------------------------------------------
// measurement
// ------------------------------------------------------------------------------------------------
int32_t cw_stage_times(cw_ctx* c, float* ms, int32_t* calls, int32_t reset) {
    for (int i = 0; i < CW_N_STAGES; ++i) {
        if (ms) ms[i] = c->stage_ms[i];
        if (calls) calls[i] = c->stage_calls[i];
        if (reset) { c->stage_ms[i] = 0.f; c->stage_calls[i] = 0; }
    }
    return CW_OK;
}

int32_t cw_time_kernel(cw_ctx* c, int32_t which, int32_t nb, int32_t iters, float* avg_ms, double* algo_bytes) {
    if (iters > 0) CWCHK(c, epoch_hygiene(c, (long long)iters + 8));
    if (which == 100 || which == 101) {
        // launch-boundary floor: a captured graph of `iters` dependent near-empty kernels (100), or the same
        // launched eagerly (101); avg_ms = time per kernel
        hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
        if (which == 100) {
            HIPCHK(c, hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal));
            for (int i = 0; i < iters; ++i) KD(c, cw_launch_set_pos, c->d_pos, 64, nb, c->st);
            HIPCHK(c, hipStreamEndCapture(c->st, &g));
            HIPCHK(c, hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
            HIPCHK(c, hipGraphLaunch(ge, c->st));
            HIPCHK(c, hipStreamSynchronize(c->st));
        }
        HIPCHK(c, hipEventRecord(c->ev0, c->st));
        if (which == 100) { for (int r = 0; r < 5; ++r) HIPCHK(c, hipGraphLaunch(ge, c->st)); }
        else for (int r = 0; r < 5; ++r) for (int i = 0; i < iters; ++i) KD(c, cw_launch_set_pos, c->d_pos, 64, nb, c->st);
        HIPCHK(c, hipEventRecord(c->ev1, c->st));
        HIPCHK(c, hipEventSynchronize(c->ev1));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *avg_ms = ms / (5.0f * iters);
        *algo_bytes = 0;
        if (ge) hipGraphExecDestroy(ge);
        if (g) hipGraphDestroy(g);
        return CW_OK;
    }
    const int D = c->d.d_model, H = c->d.n_heads, F = c->d.ffn_dim;
    if (nb < 1 || nb > c->Bm || iters < 1) return fail(c, CW_ERR_INVALID, "time_kernel: bad args");
    const int TGT = c->d.max_target_positions, V = c->d.vocab_size;
    // launches cycle through the decoder layers, as the real step does: every launch streams its weights / K,V cache
    // from HBM (one layer's 61 MB cross cache alone would otherwise sit in the 256 MB Infinity Cache and flatter the
    // kernel: 11.6 us "hot" vs 14.1 us inside the step)
    int launch_no = 0;
    const bool hot = which >= 200;                              // 200 + k: kernel k on ONE layer's operands (L2 / Infinity-Cache resident)
    if (hot) which -= 200;
    auto launch = [&]() -> int {
        LayerW& L = c->dec[hot ? 0 : (launch_no++) % c->d.dec_layers];
        switch (which) {
            case 0: {   // fc1: LN + GEMV + GELU
                EpiParams ep = epi0(); ep.outf = c->dmid; ep.bias = L.b1; ep.ldo = F;
                return gemv_ln(c, EPI_GELU_F32, c->dx, nb, D, L.w1, F, L.ln2_g, c->ln_folded ? nullptr : L.ln2_b, ep);
            }
            case 1: {   // cross-attention (the variant the decode step launches: with the fused stage in front it finishes the query)
                if (c->bf16) {
                    CrossSplitParams p{c->dq, L.ck, L.cv, CW_N_CTX, c->d_part_o, c->d_part_ml, nullptr, c->d_align_ml, nullptr,
                                       c->d_pos, 0, 0, nb, H};
                    if (c->fuse6_ready && !c->sw.no_fuse6 && c->ln_folded && nb <= 16 && (!c->kv8 || KD(c, cw_cross8_is_mfma, CW_N_CTX))) {
                        p.kv_div = 1; p.qa = c->d_qa; p.qb = c->d_qb; p.qw = L.q_wsum; p.qbias = L.bq_c;
                        p.pstats = c->d_pstats; p.n_pstats = D / 16;
                    }
                    return cross_attn(c, L, p);
                }
                DecAttnParams p = dec_attn(c->dq, L.ck, L.cv, CW_N_CTX, CW_N_CTX, nullptr, c->dattn, nb, H);
                return KD(c, cw_launch_attn_decode, c->bf16, p, c->st);
            }
            case 2: return gemv_resid(c, false, c->dattn, nullptr, nb, D, L.wo, L.bo, c->dx);   // self-attention out projection (in-place residual, K split)
            case 3: return gemv_ln(c, EPI_QKV_CACHE, c->dx, nb, D, L.wqkv, 3 * D, L.ln1_g, c->ln_folded ? nullptr : L.ln1_b, qkv_epi(c, L));   // LN + qkv + cache append
            case 4: return gemv_ln(c, EPI_STORE_F32, c->dx, nb, D, L.wq_c, D, L.lnc_g, c->ln_folded ? nullptr : L.lnc_b, cross_q_epi(c, L));   // LN + cross q
            case 5: return gemv_resid(c, false, c->dmid, nullptr, nb, F, L.w2, L.b2, c->dx);   // fc2
            case 6: return KD(c, cw_launch_attn_decode, c->bf16, dec_attn(c->dq, L.sk, L.sv, TGT, 0, c->d_pos, c->dattn, nb, H), c->st);   // self-attention at the positions in d_pos
            case 7: return launch_logits(c, nb, c->dx);
            case 8:     // near-empty kernel: launch/boundary floor
                return KD(c, cw_launch_set_pos, c->d_pos, 64, nb, c->st);
            case 9: {   // persistent stage A (declayer.hip) behind a near-empty launch that bumps the granule epoch (as the step's sampler does):
                        // without it the polls would find the previous launch's granules
                if (!c->bf16 || !c->fuse6_ready || !c->wpacked || nb > 8) return CW_ERR_INVALID;
                int r = KD(c, cw_launch_set_pos, c->d_pos, 64, nb, c->st, c->d_epoch);
                if (r != CW_OK) return r;
                return KD(c, cw_launch_dec_layer, dec_layer_params(c, (launch_no - 1) % c->d.dec_layers, nb, c->dx, c->dx1), c->n_cu, c->st);
            }
            default: return CW_ERR_INVALID;
        }
    };
    if (which == 6 || which == 3) { CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, 64, nb, c->st)); }
    for (int i = 0; i < 3; ++i) CWCHK(c, launch());
    HIPCHK(c, hipEventRecord(c->ev0, c->st));
    for (int i = 0; i < iters; ++i) CWCHK(c, launch());
    HIPCHK(c, hipEventRecord(c->ev1, c->st));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms = ms / iters;
    const double e = (double)c->esz;
    switch (which) {
        case 0: *algo_bytes = (double)F * D * e + (double)nb * D * 4 + (double)nb * F * 4; break;
        case 1: *algo_bytes = 2.0 * nb * H * CW_N_CTX * 64 * (c->kv8 ? 1.0 : e) + 2.0 * nb * D * 4; break;
        case 9: *algo_bytes = 2.0 * nb * H * CW_N_CTX * 64 * e + 3.0 * D * D * e + 6.0 * nb * D * 4; break;
        case 2: case 4: *algo_bytes = (double)D * D * e + 2.0 * nb * D * 4; break;
        case 3: *algo_bytes = 3.0 * D * D * e + 4.0 * nb * D * 4; break;
        case 5: *algo_bytes = (double)F * D * e + (double)nb * (D + F) * 4; break;
        case 6: *algo_bytes = 2.0 * nb * H * 65 * 64 * e + 2.0 * nb * D * 4; break;
        case 7: *algo_bytes = (double)V * D * e + (double)nb * (D + V) * 4; break;
        default: *algo_bytes = 0; break;
    }
    return CW_OK;
}

// kernel launches behind stage `stage` of the layer as last enumerated by cw_time_decode_stage (17..64 rows: 2 where a preparation launch precedes the GEMV)
int32_t cw_decode_stage_launches(cw_ctx* c, int32_t stage) {
    return (stage >= 0 && stage < c->stage_count && stage < CW_MAX_DEC_STAGES) ? c->stage_launches[stage] : 0;
}
const char* cw_decode_stage_name(int32_t kind) { return (kind >= 0 && kind < DST_N) ? kDecStageName[kind] : "?"; }

// One launch of the decoder layer AS decode_step ISSUES IT at nb rows (same code path, same arguments), `iters` times back to back,
// cycling through the layers so that every launch streams its operands from HBM.  stage = index of the launch inside the layer
// (0 .. *n_stages - 1; the count depends on the rows, the dtype and the switches); stage == -1: the whole layer (all its launches).
int32_t cw_time_decode_stage(cw_ctx* c, int32_t nb, int32_t stage, int32_t iters, float* avg_ms, double* algo_bytes, int32_t* kind,
                             int32_t* n_stages) {
    if (nb < 1 || nb > c->Bm || iters < 1 || stage < -1 || stage >= CW_MAX_DEC_STAGES) return fail(c, CW_ERR_INVALID, "time_decode_stage: bad args");
    if (c->beam_K > 0) return fail(c, CW_ERR_STATE, "time_decode_stage: greedy rows only");
    // the launches run for real at decoder position 64: they append to the self-attention cache and write alignment rows there
    if (c->d.max_target_positions <= 65) return fail(c, CW_ERR_INVALID, "time_decode_stage: needs max_target_positions > 65 (has %d)", c->d.max_target_positions);
    CWCHK(c, cw_check_weights(c));
    CWCHK(c, epoch_hygiene(c, (long long)iters + 8));
    if (nb > c->nb_encoded) return fail(c, CW_ERR_STATE, "time_decode_stage: nb=%d but %d windows encoded (the cross-attention reads their K/V)", nb, c->nb_encoded);
    const int D = c->d.d_model, H = c->d.n_heads, F = c->d.ffn_dim, NL = c->d.dec_layers;
    // a hand-off that gave up while timing (shared GPU) must not send the next cw_decode to the fallback path: drain and clear
    struct Restore { cw_ctx* c; ~Restore() { c->stage_sel = -1; c->layer_sel = -1; (void)hipStreamSynchronize(c->st); (void)hipMemset(c->d_err, 0, 4); } } restore{c};
    c->hist_short = false;                                       // position 64: 65 keys
    CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, 64, nb, c->st, c->d_epoch));
    // which launches does a layer have at this row count?  (nothing is launched: no stage has this index)
    c->stage_sel = CW_MAX_DEC_STAGES; c->layer_sel = 0;
    CWCHK(c, decode_step(c, nb, false));
    const int ns = c->stage_count;
    if (n_stages) *n_stages = ns;
    if (stage >= ns) return fail(c, CW_ERR_INVALID, "time_decode_stage: the layer has %d launches at %d rows", ns, nb);
    c->stage_sel = stage;
    auto one = [&](int i) -> int {
        c->layer_sel = i % NL;
        // granule tags are (epoch, layer): a second pass over the layers must not find the first pass's granules valid
        if (c->layer_sel == 0) CWCHK(c, KD(c, cw_launch_set_pos, c->d_pos, 64, nb, c->st, c->d_epoch));
        return decode_step(c, nb, false);
    };
    for (int i = 0; i < 3; ++i) CWCHK(c, one(i));
    HIPCHK(c, hipEventRecord(c->ev0, c->st));
    for (int i = 0; i < iters; ++i) CWCHK(c, one(3 + i));
    HIPCHK(c, hipEventRecord(c->ev1, c->st));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms = ms / iters;
    // algorithmic bytes: the weights of the projection(s), the cache rows, the activation rows in and out (f32 unless noted)
    const double e = (double)c->esz, act = (double)nb * D * 4.0;
    auto bytes_of = [&](int k) -> double {
        const double self_kv = 2.0 * nb * H * 65 * 64 * e;                                        // 65 cached positions (d_pos = 64)
        const double cross_kv = 2.0 * nb * H * CW_N_CTX * 64 * (c->kv8 ? 1.0 : e);
        switch (k) {
            case DST_QKV: return 3.0 * D * D * e + 4.0 * act;
            case DST_SELF_ATTN: return self_kv + 2.0 * act;
            case DST_QKV_SELF: return 3.0 * D * D * e + self_kv + 2.0 * act;
            case DST_O_PROJ: case DST_CROSS_Q: return (double)D * D * e + 2.0 * act;
            case DST_STACK: return 3.0 * D * D * e + 5.0 * act;                                   // x, a in; qa, qb, x1 out
            case DST_CROSS_ATTN: return cross_kv + 2.0 * act;
            case DST_STACK_CROSS: return 3.0 * D * D * e + cross_kv + 4.0 * act;
            case DST_CROSS_O: return (double)D * D * e + 2.0 * act;
            case DST_FC1: return (double)F * D * e + act + (double)nb * F * e;
            case DST_FC2: return (double)F * D * e + (double)nb * F * e + 2.0 * act;
            case DST_MLP_PAIR: case DST_MLP_CHAIN: return 2.0 * F * D * e + 3.0 * act;
            default: return 0.0;
        }
    };
    if (stage >= 0) {
        if (kind) *kind = c->stage_kind[stage];
        *algo_bytes = bytes_of(c->stage_kind[stage]);
    } else {
        if (kind) *kind = -1;
        double t = 0.0;
        for (int i = 0; i < ns && i < CW_MAX_DEC_STAGES; ++i) t += bytes_of(c->stage_kind[i]);
        *algo_bytes = t;
    }
    return CW_OK;
}

}  // extern "C"
