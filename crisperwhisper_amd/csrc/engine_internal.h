// Internals of the engine shared by engine.hip (the product) and engine_hooks.hip (the test / bench hooks): the context, the
// error plumbing, call-local device memory and the engine helpers the hooks drive.  Nothing here is exported by the library.
#pragma once
#include <chrono>
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <string>
#include <vector>
#include <limits>
#include <functional>
#include <algorithm>

#include "../../include/crisperwhisper.h"
#include "kernels.h"

#pragma GCC visibility push(hidden)

// dtype dispatch: the 16-bit kernels exist twice (namespace cw_bf16 / cw_f16, see kernels.h); the f32 parity kernels are
// identical in both builds
#define KD(c, fn, ...) ((c)->f16 ? cw_f16::fn(__VA_ARGS__) : cw_bf16::fn(__VA_ARGS__))

// launches of one decoder layer, as decode_step issues them (cw_time_decode_stage / cw_decode_stage_name)
#define CW_MAX_DEC_STAGES 24
enum DecStageKind { DST_OTHER = 0, DST_QKV_SELF, DST_QKV, DST_SELF_ATTN, DST_O_PROJ, DST_STACK, DST_STACK_CROSS, DST_CROSS_Q, DST_CROSS_ATTN,
                    DST_CROSS_O, DST_FC1, DST_FC2, DST_MLP_PAIR, DST_MLP_CHAIN, DST_N };
static const char* const kDecStageName[DST_N] = {
    "other (A/B path)", "LayerNorm + q/k/v projection + self-attention (qkv_self_kernel)", "LayerNorm + q/k/v projection + cache append",
    "self-attention", "self-attention out-projection", "fused out-projection + cross-query stage (gemv_stack_kernel)",
    "fused stage + cross-attention (dec_layer_a_kernel)", "LayerNorm + cross-attention query projection", "cross-attention",
    "cross-attention out-projection (combines the key-split partials)", "LayerNorm + fc1 + GELU", "fc2", "fc1 + fc2 (mlp_pair_kernel)",
    "LayerNorm + fc1 + GELU + fc2 in one launch (mlp_chain_kernel)"};

struct LayerW {
    void* wqkv = nullptr; float* bqkv = nullptr;
    void *wqkv8 = nullptr, *w18 = nullptr, *w28 = nullptr, *wkv_c8 = nullptr;   // e4m3 copies (option encoder_gemm_fp8) ...
    float *sqkv = nullptr, *s1 = nullptr, *s2 = nullptr, *skv_c = nullptr;        // ... and their per-output-row scales
    void* wo = nullptr; float* bo = nullptr;
    float *ln1_g = nullptr, *ln1_b = nullptr;
    void* wq_c = nullptr; float* bq_c = nullptr;
    void* wkv_c = nullptr; float* bkv_c = nullptr;
    void* wo_c = nullptr; float* bo_c = nullptr;
    float *lnc_g = nullptr, *lnc_b = nullptr;
    void* w1 = nullptr; float* b1 = nullptr;
    void* w2 = nullptr; float* b2 = nullptr;
    float *ln2_g = nullptr, *ln2_b = nullptr;
    void *ck = nullptr, *cv = nullptr;   // cross K/V cache   [Bm][H][1500][64]
    void *ck8 = nullptr, *cv8 = nullptr; // opt-in fp8 (e4m3) copy of it, one byte per element
    float* kvs = nullptr;                // [Bm][H][2] dequantisation scales (K, V)
    void *sk = nullptr, *sv = nullptr;   // self  K/V cache   [Bm][H][448][64]
    // six-launch decoder layer (decfuse.hip), 16-bit engines: row-stacked weights [W'q_c ; W'q_c Wo ; Wo] and
    // [W'1 ; W'1 Wo_c ; Wo_c] -- wq_c / wo / w1 / wo_c above point into them -- and the per-column constants
    void *ws3 = nullptr, *ws5 = nullptr;
    float *qa_bias = nullptr, *q_wsum = nullptr;     // [D]  W'q_c bo ;  W'q_c 1
    float *u1_bias = nullptr, *u1_wsum = nullptr;    // [F]  W'1 bo_c ;  W'1 1
    float* qkv_wsum = nullptr;                       // [3D] W'qkv 1 (17..64-row path: LayerNorm through its linearity)
};

struct cw_ctx {
    cw_model_desc d;
    bool bf16 = false;         // 16-bit engine (bfloat16 or, with f16, IEEE binary16 -- the reference's GPU dtype)
    bool f16 = false;
    int device = 0;
    int Bm = 0, S_pad = 0, Vpad = 0;
    size_t esz = 4;
    hipStream_t st = nullptr;
    hipStream_t st2 = nullptr;          // side stream of the decode step: run-ahead prefetch of the next layer's streams (CW_PREFETCH)
    hipEvent_t ev_pf[2] = {nullptr, nullptr};
    unsigned int* d_pf_sink = nullptr;
    cw_sw::Switches sw{};               // this context's A/B switches (switches.def): the environment when it was created, then its own to edit
                                        // (cw_set_option "no_wnt" / "no_xq_in_qkv" / "rows_ln" / "skinny"; handoffs_off)
    std::vector<void*> allocs;
    char err[512] = "";
    bool err_set = false;      // a specific message is pending (set by fail(), cleared by cw_last_error)
    std::vector<int> align_layers, align_heads;
    // bf16 decode engine: projections fed by a LayerNorm keep their f32 checkpoint values on the device until every
    // tensor is in, then the LayerNorm's gamma / beta are folded into them (gemm.hip: fold_layernorm_kernel)
    struct Fold { float* stage; int N, K; void* w_dst; size_t w_off; float* b_dst; size_t b_off; float scale; int layer, which; };
    std::vector<Fold> folds;
    struct OutStage { float* stage; int layer, which; };   // f32 copies of the decoder out-projections (which: 0 self, 1 cross)
    std::vector<OutStage> out_stages;
    bool fuse6_ready = false;       // product matrices of the fused decoder stages are in place
    bool rows_ln_ready = false;     // row sums of the LayerNorm-folded q/k/v, cross-q and fc1 weights are in place (gemv_rows_kernel)
    // sw.skinny, 17..64 rows (skinny.hip / attention.hip: attn_cross_full_kernel): 0 (default) round-3 path; 1 greedy rows:
    // cross-attention query as a K-split skinny GEMM whose planes the one-block-per-(row, head) cross-attention finishes, which also
    // writes the out-projection's rows (no LayerNorm preparation, no finish, no combine launch); 2 = 1 + q/k/v and fc1 through
    // planes + finish launch.  Both measured slower in the step (profiles/r04_b64_*_rejected_*): A/B only
    float* d_planes = nullptr;      // [S][rows][N] K-split partial products of the LayerNorm projections (skinny.hip)
    size_t planes_cap = 0;          // floats
    float* d_sk_stats = nullptr;    // [16][64][2] slice statistics of the rows (skinny.hip)
    float* d_rstats = nullptr;      // [max(D, F) / 16][64][2] per-block LayerNorm partial sums of the 17..64-row producers
    unsigned int* d_bar = nullptr; int* d_err = nullptr;   // group barriers of mlp_pair_kernel; "a block gave up waiting" flag
    int handoff_fallbacks = 0;      // times this context left the in-launch hand-offs for the launch-per-stage path because a wait gave up
    int handoff_resumes = 0;        // ... of which the decode call resumed at the failed position instead of starting over
    long long forwards_since_reset = 0;   // upper bound of the decoder forwards since the granule epoch last started at 1 (epoch_hygiene)
    int fail_pos = -1;              // test hook (option "handoff_fail_pos"): qkv_self_kernel gives up at this decoder position
    // persistent decoder-layer kernels (declayer.hip), rows <= 8: granule buffers, the epoch counter their tags carry, CU count.
    // Behind qkv_self_kernel (unless sw.no_xq_in_qkv) its V-tile blocks also compute the cross-query x term W'q_c x, its attention
    // epilogue leaves the 16-bit rows, and the fused stage is the two-segment gemv_stack_a16_kernel (DESIGN.md 6g''')
    unsigned long long *d_gq = nullptr, *d_gps = nullptr, *d_gq2 = nullptr, *d_gkv = nullptr, *d_gflag = nullptr;
    void* d_attn16 = nullptr;       // [8][D] self-attention output in the engine's 16-bit type (qkv_self_kernel<.., XQ> -> gemv_stack_a16_kernel)
    unsigned int* d_epoch = nullptr;
    int n_cu = 0;
    bool ln_folded = false;         // decoder LN-GEMVs run plain normalisation (affine part is inside W / bias)
    std::set<std::string> loaded;   // HF tensor names received through cw_load_tensor
    bool weights_ok = false;        // every tensor of the geometry has been loaded (checked once, see cw_check_weights)
    bool wpacked = false;           // the decoder's GEMV matrices are in fragment-major order (gemm.hip: wfrag_pack_kernel)
    void* embed_pk = nullptr;       // fragment-major copy of the tied embedding for the logits GEMV (the row-major one serves the token lookup)

    // weights
    void *conv1_w = nullptr, *conv2_w = nullptr, *embed = nullptr;
    float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr, *dec_pos = nullptr;
    float *enc_ln_g = nullptr, *enc_ln_b = nullptr, *dec_ln_g = nullptr, *dec_ln_b = nullptr;
    std::vector<LayerW> enc, dec;

    // front end
    MelTables mel{};
    float *d_pcm = nullptr, *d_logspec = nullptr, *d_feats_hf = nullptr;
    unsigned int* d_gmax = nullptr;
    void* d_feats_tm = nullptr;
    std::vector<int> n_frames_items;

    // encoder workspace
    void *c1 = nullptr, *h = nullptr, *qb = nullptr, *kb = nullptr, *vb = nullptr, *ao = nullptr, *mid = nullptr,
         *enc_out = nullptr;
    float* x = nullptr;
    int *d_row_off = nullptr, *d_row_valid = nullptr, *d_row_off2 = nullptr, *d_row_valid2 = nullptr;
    int nb_encoded = 0;

    // decoder state
    float *dx = nullptr, *dxn = nullptr, *dq = nullptr, *dattn = nullptr, *dmid = nullptr, *dlogits = nullptr;
    float *dx1 = nullptr, *dx2c = nullptr, *d_qa = nullptr, *d_qb = nullptr, *d_u1 = nullptr, *d_pstats = nullptr;   // fused decoder stages (decfuse.hip)
    float *d_cvec = nullptr, *d_ostats = nullptr;             // 33..64 rows: row centres and per-(column pair, row) LayerNorm partial sums of the column-owning out-projection
    void *d_xfrag = nullptr, *d_xfrag2 = nullptr;             // bf16 [64][5120] fragment-major activations of the 17..64-row GEMV path
    int *d_ids = nullptr, *d_forced = nullptr, *d_argmax = nullptr, *d_last_ts = nullptr, *d_finished = nullptr,
        *d_nunf = nullptr, *d_align_slot = nullptr;
    unsigned char* d_mask = nullptr;
    float* d_lp_sum = nullptr; int* d_lp_cnt = nullptr;      // per-row sum / count of chosen-token log-probabilities (score_tokens)
    bool score_tokens = false;
    float* d_tok_lp = nullptr;                                // [Bm][max_target] log_softmax(raw logits)[token] (cw_set_token_logprobs)
    bool tok_lp_on = false;
    std::vector<std::vector<float>> tr_lp;                    // ... of the last cw_transcribe, per item, aligned with its tokens
    // the top_k best raw logits of every step (cw_set_top_logprobs; needs tok_lp_on)
    int top_k = 0;                                            // 0: off
    int* d_top_id = nullptr; float* d_top_lp = nullptr;       // [Bm][max_target][CW_TOP_LOGPROBS_MAX]
    void* d_top_part = nullptr;                               // [Bm][16][CW_TOP_LOGPROBS_MAX] (value, id) pairs of the sampler's stage 1
    std::vector<std::vector<int>> tr_top_id;                  // ... of the last cw_transcribe: top_k entries per token of every item
    std::vector<std::vector<float>> tr_top_lp;
    // predictive entropy of every step's raw distribution (cw_set_token_entropy; needs tok_lp_on)
    bool tok_ent_on = false;
    float* d_tok_ent = nullptr;                               // [Bm][max_target], NaN where d_tok_lp is
    float* d_ent_part = nullptr;                              // [Bm][16] centred sums of the sampler's stage 1
    std::vector<std::vector<float>> tr_ent;                   // ... of the last cw_transcribe, per item, aligned with its tokens
    // sequence_bias (cw_set_sequence_bias): the device table in the layout of kernels.h, its host copy and entry count (0: off)
    int* d_seq_bias = nullptr;
    std::vector<int> sb_host;
    int sb_n = 0;
    float logprob_thr = NAN, no_speech_thr = NAN;             // cw_set_thresholds (NaN: unset)
    void* d_sample_part = nullptr;            // [Bm][16] 32-byte slice records of the two-stage sampler
    void* d_sample_pert = nullptr;            // [Bm][16] 16-byte records of the perturbed winners (seeded sampling)
    unsigned int* d_samp = nullptr;           // [4 + 2 * Bm] temperature bits, seed, per-row stream ids (cw_set_sampling); zero = greedy
    std::vector<unsigned int> samp_host;      // what d_samp holds
    float* d_align = nullptr;
    int align_rows = 0;                   // rows per (item, slot) of d_align / d_align_ml: max_target_positions (cw_align_heads: its capture's)
    float *d_part_o = nullptr, *d_part_ml = nullptr, *d_align_ml = nullptr;   // split cross-attention partials
    bool align_unnormalized = false;
    int* h_nunf = nullptr;  // pinned
    int *d_pos = nullptr, *d_cfg = nullptr;   // per-row decoder input position; [n_prompt, min_new, max_length, use_forced]
    hipGraphExec_t step_graph[130] = {};      // captured decode step (layers + logits + sampling) per batch size; + 65: the short-history form (hist_short)
    bool hist_short = false;                  // every row attends over <= 64 self-attention keys in the forward being launched (host knows the position)
    cw_gen_cfg gen{};
    bool gen_set = false;
    bool kv8 = false;                    // cross-attention reads the fp8 cache (cw_set_option "cross_kv_fp8")
    bool enc8 = false;                   // encoder linear layers + cross-K/V projection as e4m3 GEMMs ("encoder_gemm_fp8")
    int enc8_mask = 0;                   // which of them: 1 q/k/v, 2 fc1, 4 fc2, 8 cross-K/V projection (option value 1 = all, 16 + mask = subset)
    bool enc8_stale = false;             // a tensor was (re)loaded after the e4m3 copies were made
    void *h8 = nullptr, *mid8 = nullptr; float *sa8 = nullptr, *smid8 = nullptr;   // e4m3 activations and their row scales
    // beam search (cw_beam_*): rows = items x beams; self-attention keys are found through the ancestry table
    int beam_K = 0, beam_items = 0, beam_n_prompt = 0;
    int beam_pos = 0, beam_max_len = 0;   // position of the last decoder input / length limit (cw_beam_step refuses to run past it)
    int *d_anc = nullptr, *d_anc_tmp = nullptr, *d_ids_tmp = nullptr, *d_parent = nullptr, *d_tok = nullptr, *d_cand_id = nullptr,
        *d_rowmap = nullptr;
    float *d_cand_val = nullptr, *d_align_g = nullptr, *d_topk_scratch = nullptr;
    const float* align_cur = nullptr;     // alignment rows the timestamp stage reads (d_align, or the beam-gathered copy)
    float* logits_capture = nullptr;
    int logits_capture_steps = 0;
    int last_L = 0, last_nb = 0;

    // timestamps workspace
    float *d_mean = nullptr, *d_std = nullptr, *d_mat = nullptr, *d_skew = nullptr;
    size_t skew_cap = 0;
    unsigned char* d_trace = nullptr;
    int *d_first_col = nullptr, *d_path_text = nullptr, *d_path_time = nullptr, *d_path_len = nullptr,
        *d_ncols = nullptr;
    // alignment scores (cw_set_alignment_scores): the path-score kernel behind every DTW of the timestamp stage
    bool as_on = false;
    int as_collar = 0;
    float *d_as_mass = nullptr, *d_as_spread = nullptr;       // [Bm][max_target] per (sequence, token row) of the last DTW launch
    std::vector<std::vector<float>> as_mass, as_spread;       // rows of the last timestamp stage, each [L + 1] in cw_token_timestamps' indexing
    std::vector<std::vector<float>> tr_as_mass, tr_as_spread; // ... of the last cw_transcribe, per item, aligned with its tokens
    // language identification (langid.hip, cw_detect_language): candidate table and the per-row records, allocated on first use
    int* d_lang_ids = nullptr;                                // [CW_LANG_IDS_MAX]
    float* d_lang_out = nullptr;                              // [Bm][CW_LANG_IDS_MAX + 2]
    std::vector<int> tr_lang;                                 // language token every item of the last cw_transcribe was decoded with
    std::vector<float> tr_lang_prob;                          // ... its detection probability (NaN: forced)

    double* d_pause = nullptr;   // persistent scratch for cw_adjust_pauses: [4][pause_cap]
    int pause_cap = 0;

    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_step[2] = {nullptr, nullptr};
    // cw_time_decode_stage: one launch (stage_sel) of one layer (layer_sel) of decode_step; -1 = everything (the step itself)
    int stage_sel = -1, layer_sel = -1, stage_count = 0;
    // decoder prompt prefill (prefill.hip): on by default on the 16-bit engines; cw_set_option "prompt_prefill" = 0 forces the
    // per-position loop (A/B).  Work buffers for rows x positions, grown on demand and freed by cw_destroy.
    bool prompt_prefill = true;
    bool align_prefill = true;         // cw_align_tokens: the teacher-forced forward as one prefill ("align_prefill" = 0: the loop)
    float align_heads_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // last cw_align_heads: forward, normalise, similarity, timestamps, similarity kernel alone (cw_align_heads_times)
    int align_prefill_runs = 0;        // cw_align_tokens calls whose forward ran as the prefill (cw_align_prefill_runs)
    int pf_prefix = 0;                 // prompt_ids in front of the init tokens of the coming decoder inputs ("prompt_prefix")
    size_t pf_rows = 0;
    float* pf_x = nullptr;
    void *pf_a = nullptr, *pf_q = nullptr, *pf_o = nullptr, *pf_h = nullptr;
    // scoring (score.hip, cw_score_tokens): the teacher-forced forward as one prefill with the scoring head ("score_prefill" = 0:
    // the per-position loop, the only path of the f32 engine and the e4m3 cross cache).  Buffers for the scored positions grow
    // on demand; sc_step_*: [Bm][TGT] results of the loop, filled position by position while score_hook is set.
    bool score_prefill = true;
    int score_prefill_runs = 0;
    size_t sc_rows = 0, sc_parts = 0;
    int *sc_src = nullptr, *sc_tgt = nullptr, *sc_ti = nullptr;
    void* sc_a = nullptr;
    ScorePart* sc_part = nullptr;
    float *sc_lp = nullptr, *sc_tl = nullptr;
    bool score_hook = false;
    float *sc_step_lp = nullptr, *sc_step_tl = nullptr;
    int* sc_step_ti = nullptr;
    // cw_align_cut_tokens: the STOP form of the head (stop_logprob beside the scores; score_stop switches the loop's hook to it)
    // and the cut kernel's arguments and results, [Bm] each, cut_ok [Bm][TGT] bytes
    bool score_stop = false;
    size_t sc_stop_rows = 0, sc_sparts = 0;
    float* sc_stop = nullptr;
    ScoreStopPart* sc_spart = nullptr;
    float* sc_step_stop = nullptr;
    int *cut_base = nullptr, *cut_ntok = nullptr, *cut_out = nullptr;
    float* cut_score = nullptr;
    unsigned char *cut_force = nullptr, *cut_ok = nullptr;
    // cw_set_score_top_logprobs: the TOPK forms of the head and of the loop's row kernel.  sc_tpart: the head's per-split lists,
    // sc_alt_*: [M][CW_TOP_LOGPROBS_MAX] of the head, sc_step_alt_*: [Bm][TGT][CW_TOP_LOGPROBS_MAX] of the loop; all allocated on
    // first use.  sc_top_ids / sc_top_lps: the last scoring call's alternatives [sc_top_rows][sc_top_stride][CW_TOP_LOGPROBS_MAX]
    int sc_top_k = 0;
    size_t sc_tparts = 0, sc_alt_rows = 0;
    ScoreTopPart* sc_tpart = nullptr;
    int *sc_alt_id = nullptr, *sc_step_alt_id = nullptr;
    float *sc_alt_lp = nullptr, *sc_step_alt_lp = nullptr;
    std::vector<int32_t> sc_top_ids;
    std::vector<float> sc_top_lps;
    int sc_top_rows = 0, sc_top_stride = 0;
    // cw_set_score_entropy: the ENT forms of the head and of the loop's row kernel.  sc_epart: the head's per-split centred sums,
    // sc_ent: [M] of the head, sc_step_ent: [Bm][TGT] of the loop; all allocated on first use.  sc_ents: the last scoring call's
    // entropies [sc_ent_nrows][sc_ent_stride], NaN where nothing was scored
    bool sc_ent_on = false;
    size_t sc_eparts = 0, sc_ent_rows = 0;
    float *sc_epart = nullptr, *sc_ent = nullptr, *sc_step_ent = nullptr;
    std::vector<float> sc_ents;
    int sc_ent_nrows = 0, sc_ent_stride = 0;
    int stage_kind[CW_MAX_DEC_STAGES] = {};
    int stage_launches[CW_MAX_DEC_STAGES] = {};   // kernel launches behind each stage (2 where gemv_prep_kernel precedes gemv_mt_kernel)
    float stage_ms[CW_N_STAGES] = {};
    int stage_calls[CW_N_STAGES] = {};
};

int fail(cw_ctx* c, int code, const char* fmt, ...);
// outer frames keep the innermost message and only add one when the callee reported a bare code
int fail_ctx(cw_ctx* c, int code, const char* call, const char* file, int line);

#define HIPCHK(c, call)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) return fail(c, CW_ERR_HIP, "%s failed: %s (%s:%d)", #call,            \
                                          hipGetErrorString(e_), __FILE__, __LINE__);               \
    } while (0)
#define CWCHK(c, call)                                                          \
    do {                                                                        \
        int r_ = (call);                                                        \
        if (r_ != CW_OK) return fail_ctx(c, r_, #call, __FILE__, __LINE__); \
    } while (0)
#define KCHK(c) HIPCHK(c, hipGetLastError())

template <typename P>
static int dmalloc(cw_ctx* c, P** p, size_t bytes, bool zero = true) {
    void* q = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(c, CW_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    if (zero) hipMemset(q, 0, bytes);
    c->allocs.push_back(q);
    *p = (P*)q;
    return CW_OK;
}

struct StageTimer {
    cw_ctx* c; int stage;
    StageTimer(cw_ctx* c_, int s) : c(c_), stage(s) { hipEventRecord(c->ev0, c->st); }
    void stop() {
        hipEventRecord(c->ev1, c->st);
        hipEventSynchronize(c->ev1);
        float ms = 0.f;
        hipEventElapsedTime(&ms, c->ev0, c->ev1);
        c->stage_ms[stage] += ms;
        c->stage_calls[stage] += 1;
    }
};

// Call-local device memory of a test / bench hook or an entry point: everything allocated through `get` is freed when the scope
// ends, on every exit path (they return through HIPCHK / CWCHK from many places; tools call the hooks in loops).
struct DevScope {
    std::vector<void*> ptrs;
    template <typename P> hipError_t get(P** p, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : 1);
        if (e == hipSuccess) ptrs.push_back(q);
        *p = (P*)q;
        return e;
    }
    ~DevScope() { for (void* q : ptrs) hipFree(q); }
};

// engine helpers the hooks call (defined in engine.hip)
int upload_T(cw_ctx* c, void* dst, size_t off, const float* src, size_t n, float scale = 1.0f);   // host f32 -> device T at element `off`
int download_T(cw_ctx* c, const void* src, size_t off, float* dst, size_t n);                     // device T -> host f32
extern "C" {   // (engine.hip defines them inside its extern "C" block)
EpiParams epi0();
DecAttnParams dec_attn(const float* q, const void* K, const void* V, int cap, int n_keys, const int* pos, float* out, int B, int H);
int gemv_ln(cw_ctx* c, int epi, const float* x, int Mb, int K, const void* W, int N, const float* g, const float* b, const EpiParams& ep);
int launch_logits(cw_ctx* c, int nb, const float* x);
EpiParams qkv_epi(cw_ctx* c, LayerW& L);
EpiParams cross_q_epi(cw_ctx* c, LayerW& L);
int gemv_resid(cw_ctx* c, bool frag, const float* a, void* xf, int nb, int K, const void* W, const float* bias, float* x, int x16 = 0);
int cross_attn(cw_ctx* c, LayerW& L, CrossSplitParams p);
DecLayerParams dec_layer_params(cw_ctx* c, int l, int nb, const float* xin, float* xalt);
int decode_step(cw_ctx* c, int nb, bool want_logits);
bool step_plan_xq(const cw_ctx* c, int nb);
int launch_sample(cw_ctx* c, int nb);
void drop_step_graphs(cw_ctx* c);
int epoch_hygiene(cw_ctx* c, long long upcoming_forwards);
int seq_bias_table(cw_ctx* c, int n_seq, const int32_t* tokens, const int32_t* lengths, const float* bias, std::vector<int>* out, const char* who);
int seq_bias_install(cw_ctx* c, const std::vector<int>& tab, int n_seq);
int write_sampling(cw_ctx* c, float temperature, uint64_t seed, const uint64_t* row_streams, int nb, const char* who);
int check_lang_ids(cw_ctx* c, const char* who, const int32_t* lang_ids, int n_lang);
int language_probs(cw_ctx* c, int nb, const int32_t* lang_ids, int n_lang, int ns_tok, int32_t* best, float* prob, float* no_speech);
int beam_alloc(cw_ctx* c);
int launch_beam_topk(cw_ctx* c, int rows, int n_cand);
}

#pragma GCC visibility pop
