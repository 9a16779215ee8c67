/*
 * crisperwhisper.h -- C ABI of the MI355X-native CrisperWhisper inference-and-alignment path.
 *
 * The reference (nyrahealth/CrisperWhisper @ 2024-10-22) has no FFI layer: its hot path is reached
 * through the HuggingFace pipeline object protocol (REF/transcribe.py:21-33).  This header declares
 * the device-side replacement for each internal seam of that protocol; the
 * Python shim in crisperwhisper_amd/ binds it with ctypes and re-implements the
 * pipeline call surface on top.  "TF/" = site-packages/transformers 5.15.0, "REF/" = the reference.
 *
 * Conventions: every function returns 0 on success or a negative errno-style code (cw_last_error()
 * gives the message); no exceptions cross the ABI; all pointer arguments are caller-owned HOST
 * buffers unless the name ends in _dev; the context owns all device memory and one HIP stream; one
 * context per device per process; a context is not re-entrant (external locking).
 */
#ifndef CRISPERWHISPER_H
#define CRISPERWHISPER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cw_ctx cw_ctx;

#define CW_DTYPE_F32 0   /* parity mode: f32 weights, activations and arithmetic                       */
#define CW_DTYPE_BF16 1  /* performance mode: bf16 weights/activations, f32 accumulation + residuals   */
#define CW_DTYPE_F16 2   /* same engine in IEEE binary16, the reference's GPU dtype (REF/transcribe.py:10,  */
                         /* REF/app.py:111): same MFMA rate, 3 more significand bits than bfloat16           */

#define CW_N_SAMPLES 480000  /* 30 s @ 16 kHz  (TF/models/whisper/feature_extraction_whisper.py:88-93) */
#define CW_N_FRAMES 3000     /* mel frames per window                                                  */
#define CW_N_CTX 1500        /* encoder frames (max_source_positions)                                  */

/* Model geometry: the fields of WhisperConfig the path reads (TF/models/whisper/configuration_whisper.py). */
typedef struct {
    int32_t d_model, n_heads, ffn_dim, enc_layers, dec_layers, n_mels, vocab_size;
    int32_t max_target_positions;   /* 448                                                             */
    int32_t median_filter_width;    /* config.median_filter_width, read at generation_whisper.py:346   */
    int32_t dtype;                  /* CW_DTYPE_*                                                      */
    int32_t max_batch;              /* chunks in flight (pipeline batch_size, REF/transcribe.py:27)    */
    int32_t n_align;                /* generation_config.alignment_heads                               */
    const int32_t* align_layers;    /* [n_align]                                                       */
    const int32_t* align_heads;     /* [n_align]                                                       */
} cw_model_desc;

/* Generation settings: what WhisperGenerationMixin.generate derives from generation_config
 * (TF/models/whisper/generation_whisper.py:650-722, 1774-1812).                                       */
typedef struct {
    int32_t eos_token_id, pad_token_id;
    int32_t no_timestamps_token_id;          /* timestamp_begin = this + 1                              */
    int32_t max_initial_timestamp_index;     /* < 0: unset                                              */
    const int32_t* suppress_tokens; int32_t n_suppress;
    const int32_t* begin_suppress_tokens; int32_t n_begin_suppress;
} cw_gen_cfg;

int32_t cw_abi_version(void);
cw_ctx* cw_create(const cw_model_desc* desc, int32_t device);
void cw_destroy(cw_ctx* ctx);
const char* cw_last_error(cw_ctx* ctx);          /* ctx may be NULL after a failed cw_create           */
int32_t cw_sync(cw_ctx* ctx);

/* Weights: one call per tensor of WhisperForConditionalGeneration.state_dict() (HF names, f32 host data,
 * replaces AutoModelForSpeechSeq2Seq.from_pretrained + model.to(device), REF/transcribe.py:14-17).
 * The context fuses q/k/v projections, folds the 1/8 query scale (modeling_whisper.py:309) and re-lays
 * the conv kernels for implicit GEMM.  proj_out.weight is tied to embed_tokens (:965) and ignored.     */
int32_t cw_load_tensor(cw_ctx* ctx, const char* hf_name, const float* data, const int64_t* shape, int32_t ndim);
/* 0 when every tensor of the geometry has been received, else CW_ERR_STATE with the missing names in cw_last_error
 * (also enforced by the first cw_encode: device buffers start zero-filled, a partial checkpoint must not run).     */
int32_t cw_check_weights(cw_ctx* ctx);
int32_t cw_set_generation(cw_ctx* ctx, const cw_gen_cfg* cfg);
/* Context options (before cw_encode).  "cross_kv_fp8" = 1: the cross-attention K/V cache is additionally stored in OCP
 * e4m3 with one scale per (chunk, head, K|V) and the decode step streams that copy (half the bytes of the dominant
 * stream; 16-bit engines only; an accuracy-gated performance mode, BASELINE configs[3], not the parity path).  The copy is
 * read by v_mfma_f32_16x16x32_fp8_fp8 (K row-major, V in the fragment order of the B operand; csrc/attention.hip).
 * "encoder_gemm_fp8" = 1 (after the weights are loaded; 16-bit engines): e4m3 copies of the encoder's qkv / fc1 / fc2 and the
 * decoder's cross-K/V weights are made with one scale per output row, the LayerNorms in front of those GEMMs emit e4m3 rows with
 * one scale per row, and the GEMMs run on v_mfma_scale_f32_16x16x128_f8f6f4 -- the fp8 MFMA half of BASELINE configs[3];
 * accuracy-gated like the cache option, 0 switches back.
 * "prompt_prefix" = n (default 0): the coming cw_decode / cw_beam_begin inputs start with n prompt_ids in front of the init
 * tokens (cw_transcribe_prompted sets it for its own calls).  With n > 0 and "prompt_prefill" (default 1) the forward-only
 * positions run as ONE multi-token decoder forward on the matrix cores (csrc/prefill.hip) on 16-bit engines with the 16-bit cross
 * cache; "prompt_prefill" = 0, n = 0 and every other engine run them through the per-position decoder step.                 */
int32_t cw_set_option(cw_ctx* ctx, const char* name, int32_t value);

/* ---- audio ingest (the step in front of seam 1) -------------------------------------------------
 * cw_ingest: interleaved little-endian sample frames as they sit in a RIFF/WAVE data chunk -> mono f32 at sr_out, on
 * device: integer formats scaled to [-1, 1), channels averaged (what `ffmpeg -ac 1 -ar 16000 -f f32le` of
 * TF/pipelines/audio_utils.py:9-45 delivers), optional (y - mean) / std / 8 of REF/app.py:85-93, then
 * torchaudio.functional.resample with its defaults (sinc_interp_hann, lowpass_filter_width = 6, rolloff = 0.99:
 * TF/pipelines/automatic_speech_recognition.py:398-412, REF/app.py:94-95).  out holds
 * cw_resampled_length(n_frames, sr_in, sr_out) = ceil(n_frames * sr_out / sr_in) floats.
 * cw_resample_taps exposes the tap table [new][2*width + orig] (f64 arithmetic rounded to f32) for differential tests. */
#define CW_PCM_U8 0
#define CW_PCM_S16 1
#define CW_PCM_S24 2
#define CW_PCM_S32 3
#define CW_PCM_F32 4
#define CW_PCM_F64 5
int64_t cw_resampled_length(int64_t n_frames, int32_t sr_in, int32_t sr_out);
int32_t cw_ingest(cw_ctx* ctx, const void* raw, int32_t fmt, int32_t channels, int64_t n_frames, int32_t sr_in,
                  int32_t sr_out, int32_t normalise, float* out);
int32_t cw_resample_taps(int32_t sr_in, int32_t sr_out, float* taps, int32_t cap, int32_t* orig, int32_t* nw,
                         int32_t* width);

/* FLAC container (host, no GPU): the part of `ffmpeg_read` (TF/pipelines/audio_utils.py:9-45) that turns a .flac file into
 * integer samples -- RFC 9639 decoder with CRC-8 / CRC-16 / STREAMINFO-MD5 verification (csrc/flac.cpp).  cw_flac_decode writes
 * interleaved samples left-justified to 32 bits ([frames][channels] int32: exactly what cw_ingest(CW_PCM_S32) scales by
 * 2^-31, i.e. ffmpeg's s16 / s32 -> f32 conversion); pcm_s32 == NULL only reports the frame count.  cap_frames > 0 also
 * bounds the decoding: the frame loop stops with an error as soon as more frames than that were produced (a decompression
 * bomb never materialises); with pcm_s32 == NULL it is the most the caller would accept, 0 = unbounded.  Errors: negative
 * code, text in cw_flac_last_error().                                                                                 */
int32_t cw_flac_info(const uint8_t* data, int64_t n_bytes, int32_t* sample_rate, int32_t* channels,
                     int32_t* bits_per_sample, int64_t* total_frames);
int32_t cw_flac_decode(const uint8_t* data, int64_t n_bytes, int32_t* pcm_s32, int64_t cap_frames, int64_t* n_frames);
const char* cw_flac_last_error(void);

/* ---- seam 1: feature extractor (WhisperFeatureExtractor.__call__, feature_extraction_whisper.py:193-346)
 * pcm: [B][n_samples[b]] packed back to back (each <= CW_N_SAMPLES; zero-padded to 30 s on device).
 * feats_out (nullable): [B][n_mels][3000] f32, HF layout.  n_frames_out (nullable): attention_mask.sum(-1).
 * Features stay resident in the context as items 0..B-1 for cw_encode.                                 */
int32_t cw_mel(cw_ctx* ctx, const float* pcm, int32_t B, const int32_t* n_samples, float* feats_out,
               int32_t* n_frames_out);
/* Same, split so a benchmark can keep the PCM resident in HBM and time only device work.               */
int32_t cw_upload_pcm(cw_ctx* ctx, const float* pcm, int32_t B, const int32_t* n_samples);
int32_t cw_mel_resident(cw_ctx* ctx, int32_t B);
/* Test hook: install externally computed features ([B][n_mels][3000] f32) as items 0..B-1.             */
int32_t cw_set_features(cw_ctx* ctx, const float* feats, int32_t B);

/* ---- seam 2: model.generate, split into its device stages ------------------------------------------
 * cw_encode: WhisperEncoder.forward (modeling_whisper.py:590-646) on the 3000-frame windows
 *   features[item[i]][:, seek[i] : seek[i] + n_frames[i]] zero-padded to 3000 (generation_whisper.py:1831-1852),
 *   followed by the cross-attention K/V projection of all decoder layers (:322-335).                   */
int32_t cw_encode(cw_ctx* ctx, int32_t nb, const int32_t* item, const int32_t* seek, const int32_t* n_frames);
int32_t cw_get_encoder_output(cw_ctx* ctx, float* out /* [nb][1500][d_model] */, int32_t nb);

/* cw_decode: one greedy GenerationMixin.generate call (TF/generation/utils.py:2783-2973) over the nb
 * encoded windows: decoder forward with KV caches, logits processors (logits_process.py:203-260,
 * 1816-2047), argmax, eos/pad bookkeeping, until every row is finished.  Alignment-head cross-attention
 * rows are retained on device for cw_token_timestamps.
 *   prompt [nb][n_prompt]; max_new_tokens < 0: bounded by max_length; forced (nullable) [nb][max_target]:
 *   entries >= 0 teacher-force that sequence position (the un-forced choice still goes to argmax_out).
 *   sequences [nb][max_target] (prompt included), lengths [nb] = prompt + generated,
 *   argmax_out (nullable) [nb][max_target].                                                            */
int32_t cw_decode(cw_ctx* ctx, int32_t nb, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                  int32_t min_new_tokens, const int32_t* forced, int32_t* sequences, int32_t* lengths,
                  int32_t* argmax_out);
/* Deterministic half of generate_with_fallback (generation_whisper.py:970-1116, _need_fallback :1243-1287) at temperature 0:
 * with both thresholds set, a window whose average token log-probability (log_softmax of the processed scores at the
 * generated tokens, eos included, :1958-1974) is below logprob_threshold AND whose no-speech probability
 * (WhisperNoSpeechDetection, logits_process.py:2050-2112: softmax of the raw logits at the <|startoftranscript|> position, token
 * no_timestamps_token_id - 1) is above no_speech_threshold is skipped: seek advances by the window, no segment (:879-881).
 * NaN = unset.  cw_transcribe applies them; stage-wise callers use cw_no_speech_probs before cw_decode and
 * cw_get_avg_logprobs after it (token scores are tracked while a logprob threshold is set).  The stochastic half --
 * re-decoding the windows that fail a threshold at higher temperatures -- is built from cw_set_sampling and cw_decode_rows
 * below by the host seek loop (crisperwhisper_amd/generation.py); cw_transcribe itself stays greedy, without fallback.      */
int32_t cw_set_thresholds(cw_ctx* ctx, float logprob_threshold, float no_speech_threshold);
/* Seeded sampling for the coming cw_decode / cw_decode_rows calls (greedy rows only; beam search is never sampled,
 * generation_whisper.py:1004-1005).  The token written at sequence position t of a row is
 *     argmax over the tokens v the logits processors allow of   fl(fl(s_v / T) + g_v),     lowest v on an exact tie,
 * s the processed f32 score, T = temperature, g_v = -log(-log(u_v)) (Gumbel-max: an exact draw from softmax(s / T)).  Once
 * the timestamp rule (logits_process.py:2040-2045) has fired -- it is evaluated on the unperturbed scores, as are the
 * log-probability sums behind cw_get_avg_logprobs -- the argmax runs over the allowed timestamp tokens alone.
 * The noise is counter-based: (x_0, x_1, x_2, x_3) = Philox4x32-10(key = (seed_lo, seed_hi), counter = (v >> 2, t, stream_lo,
 * stream_hi)) (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011; multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85), word x_{v & 3} belongs to token v, and u = ((x >> 8) + 0.5) * 2^-24 as a real number in
 * (0, 1) -- never 0 or 1.  u is exact in f32 for x >> 8 < 2^23; above that 1 - u is, and the kernel takes -log(u) as
 * -log1p(-(1 - u)) there.  seed_lo / seed_hi and stream_lo / stream_hi are the low / high 32 bits of `seed` and of
 * row_streams[b]: a token depends on (seed, stream of its row, t, logits) only, never on the row index or the batch.
 * temperature 0 or row_streams == NULL: greedy again, bit for bit the path that never called this.  A negative, NaN or
 * infinite temperature and nb outside 1 .. max_batch are refused.  The values live in device memory the sampler kernels read,
 * so captured decode steps stay valid.                                                                                     */
int32_t cw_set_sampling(cw_ctx* ctx, float temperature, uint64_t seed, const uint64_t* row_streams /* [nb] */, int32_t nb);
/* cw_decode with only some rows live: row_active [nb] (NULL: all), a row with 0 starts finished -- the decoder still steps
 * it (the step streams weights; an idle row costs nothing measurable), but its ids on device and its log-probability sum and
 * count (cw_get_avg_logprobs) stay what the previous decode left, and its lengths entry is 0.  Its cache and alignment rows
 * are overwritten: take cw_token_timestamps of a row after the decode that settled it.  No active row is refused.          */
int32_t cw_decode_rows(cw_ctx* ctx, int32_t nb, const int32_t* prompt, int32_t n_prompt, int32_t max_length,
                       int32_t min_new_tokens, const int32_t* forced, const int32_t* row_active, int32_t* sequences,
                       int32_t* lengths, int32_t* argmax_out);
int32_t cw_no_speech_probs(cw_ctx* ctx, int32_t nb, int32_t sot_token, float* out /* [nb] */);
int32_t cw_get_avg_logprobs(cw_ctx* ctx, float* out /* [nb] */, int32_t nb);
/* Per-token log-probabilities of the free-running decode (word confidence).  With the switch on (default off), the sampler
 * kernels store for every row and sequence position t it writes
 *     logprob[t] = logits[tok_t] - logsumexp(logits[0 .. vocab_size-1]),
 * logits = the raw f32 logits of the step that produced tok_t (no suppress lists, no timestamp rule, no temperature; pad
 * columns never count), tok_t = what was written at t: the arg-max, the sampled or the forced token.  It is the quantity
 * cw_score_tokens reports, taken where the token is chosen: no extra launch, no extra forward.  expf / logf throughout.
 * cw_set_token_logprobs allocates a [max_batch][max_target_positions] f32 buffer on first use and drops the captured decode
 * steps when the value changes.  cw_get_token_logprobs is valid after cw_decode / cw_decode_rows and aligned with `sequences`:
 * NaN marks prompt positions, positions behind a row's end and rows never decoded (0.0 is a legitimate value); a row that
 * cw_decode_rows masks keeps the values of the decode before.  With the switch on a lost in-launch hand-off repeats the
 * whole cw_decode call on the launch-per-stage kernels (as with a logprob threshold) instead of resuming mid-sequence.
 * cw_transcribe / cw_transcribe_prompted carry the values through segment slicing exactly as they carry token timestamps;
 * cw_get_transcribe_token_logprobs returns those of the last call, aligned with its `tokens` (NaN behind lens[i]).          */
int32_t cw_set_token_logprobs(cw_ctx* ctx, int32_t on);
int32_t cw_get_token_logprobs(cw_ctx* ctx, float* out /* [nb][max_target_positions] */, int32_t nb);
int32_t cw_get_transcribe_token_logprobs(cw_ctx* ctx, float* out /* [B][cap] */, int32_t B, int32_t cap);
/* top_logprobs: what else the model considered.  With k = 1 .. CW_TOP_LOGPROBS_MAX (0 = off, the default) the sampler kernels
 * also store, for every row and sequence position t they write, the k best raw logits of the step:
 *   candidates  the columns v < vocab_size with logits[v] > -inf: the RAW f32 logits (no suppress lists, no timestamp rule, no
 *               temperature, no Gumbel noise: masked tokens count; pad columns never count; a NaN logit is never a candidate)
 *   order       value descending, token id ascending on an exact tie
 *   top_id[t][j]       the id of the j-th candidate
 *   top_logprob[t][j]  logits[id] - logsumexp(logits[0 .. vocab_size-1]) with the very normaliser of logprob[t] above, so where
 *                      the written token is among the k its value is bit-identical to cw_get_token_logprobs at t
 * A rank at or beyond the number of candidates holds id -1 / NaN, and so do all k entries wherever cw_get_token_logprobs holds
 * NaN.  The written token (arg-max, sampled or forced) need not be among the alternatives.  A row masked by cw_decode_rows
 * keeps its entries.  No launch and no forward is added: stage 1 of the sampler selects the k best of each of its 16 slices
 * from the registers it already holds, stage 2 merges the 16 x k pairs in one wave.
 * cw_set_top_logprobs: CW_ERR_INVALID outside 0 .. CW_TOP_LOGPROBS_MAX; CW_ERR_STATE for k > 0 while cw_set_token_logprobs is
 * off (switching that off switches this off too).  Allocates [max_batch][max_target_positions][CW_TOP_LOGPROBS_MAX] int32 and
 * f32 on first use; drops the captured decode steps when the value changes.  Greedy / sampled decoding only: beam search does
 * not carry alternatives.
 * cw_get_top_logprobs: [nb][max_target_positions][k], aligned with `sequences`.  cw_get_transcribe_top_logprobs: those of the
 * last cw_transcribe / cw_transcribe_prompted, [B][cap][k] aligned with its `tokens` (-1 / NaN behind lens[i]).             */
#define CW_TOP_LOGPROBS_MAX 8
int32_t cw_set_top_logprobs(cw_ctx* ctx, int32_t k);
int32_t cw_get_top_logprobs(cw_ctx* ctx, int32_t* ids_out, float* lp_out /* [nb][max_target_positions][k] */, int32_t nb);
int32_t cw_get_transcribe_top_logprobs(cw_ctx* ctx, int32_t* ids_out, float* lp_out /* [B][cap][k] */, int32_t B, int32_t cap);
/* Token entropy: how flat the whole next-token distribution was at the step that wrote a token.  With the switch on (default
 * off) the sampler kernels also store, for every row and sequence position t they write, the predictive entropy in nats
 *     F = { v < vocab_size : logits[v] > -inf },  m = max_F logits,
 *     S = sum_F exp(logits[v] - m),  Zc = sum_F exp(logits[v] - m) (logits[v] - m),
 *     entropy[t] = log S - Zc / S                                  0 <= entropy[t] <= log |F|
 * on the RAW f32 logits of the step, the distribution of logprob[t] above: no suppress lists, no timestamp rule, no temperature,
 * no Gumbel noise, no sequence_bias; masked tokens count, pad columns never do.  It does not depend on which token was written
 * (arg-max, sampled or forced), so free-running and teacher-forced numbers are comparable.  NaN where F is empty or a logit
 * v < vocab_size is NaN or +inf.  A value that f32 rounding leaves below 0 (a one-point distribution) is stored as 0.  No launch, no forward and no stored logits are added: stage 1 of the sampler keeps Zc beside the
 * (max, sum exp) pair it keeps for logprob[t]; partials (m_i, S_i, Zc_i) move to a common centre M as
 *     S = sum S_i e^(m_i - M),  Zc = sum (Zc_i + S_i (m_i - M)) e^(m_i - M)
 * in a fixed order (thread, block, the 16 slices), without atomics: a row's value is bit-identical from run to run and whatever
 * else is in the batch.
 * cw_set_token_entropy: CW_ERR_STATE while cw_set_token_logprobs is off (switching that off switches this off too).  Allocates
 * [max_batch][max_target_positions] f32 and the slice partials on first use; drops the captured decode steps when the value
 * changes.  Greedy / sampled decoding only: beam search does not carry it.
 * cw_get_token_entropy: [nb][max_target_positions], aligned with `sequences`: NaN at every position where cw_get_token_logprobs
 * holds NaN (prompt positions, behind a row's end, rows never decoded; both are stored by one branch), and besides only at a step
 * whose logits hold a NaN or +inf -- there the log-probability may still be finite, because its log-sum-exp steps over a NaN that
 * a thread meets before any finite logit, while the entropy is NaN for every such row.  A row masked by cw_decode_rows keeps its
 * values.  cw_get_transcribe_token_entropy: those of the last cw_transcribe /
 * cw_transcribe_prompted, carried through segment slicing as the token log-probabilities are (NaN behind lens[i]).          */
int32_t cw_set_token_entropy(cw_ctx* ctx, int32_t on);
int32_t cw_get_token_entropy(cw_ctx* ctx, float* out /* [nb][max_target_positions] */, int32_t nb);
int32_t cw_get_transcribe_token_entropy(cw_ctx* ctx, float* out /* [B][cap] */, int32_t B, int32_t cap);
/* sequence_bias: steer the free-running decode towards (or away from) known token sequences -- the contract of transformers'
 * SequenceBiasLogitsProcessor.  The table is a set of n_seq distinct token sequences (`tokens` = their concatenation, lengths[i]
 * tokens each, 1 .. CW_SEQUENCE_BIAS_MAX_LEN) with one finite bias each.  At the step that writes sequence index t (ids[0 .. t-1]
 * exist: decoder prompt, prompt_ids prefix and what was generated) a sequence of length L applies to a row iff L == 1, or L <= t
 * and ids[t-L+1 .. t-1] equals its first L-1 tokens; a sequence with L == t + 1 is skipped although its prefix would fit, as
 * transformers skips it.  The row's bias of token v is the float32 sum of: the length-1 entry of v, then the applying longer
 * sequences ending in v in table order.  The sampler kernels consume fl32(logits[v] + bias[v]) wherever they consumed logits[v]:
 * suppress lists and timestamp grammar (a suppressed or -inf token stays -inf), the log-sum-exp timestamp rule, the arg-max,
 * score / T + Gumbel under sampling, and the processed-score log-probability behind cw_get_avg_logprobs.  What reports RAW scores
 * does not move: cw_get_token_logprobs, cw_get_top_logprobs, language detection, the no-speech probability.  A forced token is
 * still written; only the un-forced choice moves.  The match and the add run inside the two sampler kernels: no launch, no
 * forward and no host round trip per step is added.
 * n_seq == 0 switches it off (the pointers may then be NULL).  Refused before any state changes: CW_ERR_INVALID for a null
 * pointer, n_seq outside 0 .. CW_SEQUENCE_BIAS_MAX, a length outside 1 .. CW_SEQUENCE_BIAS_MAX_LEN, an id outside
 * 0 .. vocab_size-1, a non-finite bias, a duplicate sequence; CW_ERR_STATE while a beam search is open.  Beam search does not
 * carry the bias (there it would be added to log_softmax(raw), which moves the normaliser): cw_beam_begin returns CW_ERR_STATE
 * while a table is set.  Only switching between off and on drops the captured decode steps; new contents are one device copy.
 * cw_decode, cw_decode_rows, cw_transcribe and cw_transcribe_prompted all honour it.                                        */
#define CW_SEQUENCE_BIAS_MAX 256
#define CW_SEQUENCE_BIAS_MAX_LEN 16
int32_t cw_set_sequence_bias(cw_ctx* ctx, int32_t n_seq, const int32_t* tokens, const int32_t* lengths /* [n_seq] */,
                             const float* bias /* [n_seq] */);
int32_t cw_get_logits(cw_ctx* ctx, float* out /* [nb][vocab] */, int32_t nb);       /* last sampled step */
int32_t cw_set_logits_capture(cw_ctx* ctx, float* host_buf, int32_t max_steps);    /* [steps][nb][vocab] */
int32_t cw_get_alignment(cw_ctx* ctx, float* out /* [nb][n_align][L][1500] */, int32_t nb, int32_t L);

/* cw_transcribe: the whole of WhisperGenerationMixin.generate(return_timestamps=True, return_token_timestamps=True)
 * for the B feature items resident after cw_mel -- init tokens incl. language detection (:1455-1608, :1610-1673,
 * reusing the first encoder pass), the seek loop with batch shrinking (:785-903), eos/pad stripping (:1060-1082),
 * _retrieve_segment (:1977-2074) -- on top of cw_encode / cw_decode / cw_token_timestamps.  Greedy, no fallback.
 * Output per item: the concatenated segment tokens and their absolute token timestamps (what the pipeline hands to
 * _decode_asr, TF/pipelines/automatic_speech_recognition.py:529-540): tokens/token_ts [B][cap], lens [B].          */
typedef struct {
    int32_t sot_token;               /* decoder_start_token_id (<|startoftranscript|>)                             */
    int32_t language_token;          /* e.g. id of <|en|>; -1: detect per item                                   */
    int32_t task_token;              /* id of <|transcribe|> / <|translate|>; -1: none (only valid with detection) */
    int32_t max_new_tokens;          /* -1: bounded by max_length                                                  */
    int32_t min_new_tokens;          /* 0: none                                                                    */
    int32_t max_length;              /* generation_config.max_length (448)                                         */
    const int32_t* lang_ids; int32_t n_lang_ids;   /* generation_config.lang_to_id values (for detection)         */
} cw_transcribe_cfg;
int32_t cw_transcribe(cw_ctx* ctx, int32_t B, const int32_t* num_frames, const cw_transcribe_cfg* cfg,
                      int32_t* tokens, float* token_ts, int32_t* lens, int32_t cap, int32_t* n_passes);
/* cw_transcribe_prompted: the same with generate(prompt_ids=...) (generation_whisper.py:1909-1913): prefix[n_prefix]
 * (<|startofprev|> p1 .. pk) goes in front of every window's {sot, lang[, task]} after language detection, and every pass
 * of the seek loop starts from that same decoder input (condition_on_prev_tokens = False).  With a prefix the length
 * rules are transformers' _set_max_new_tokens_and_length (:1920-1946): n_prompt + max_new_tokens > max_target_positions
 * fails; without max_new_tokens max_length = min(cfg->max_length + min(max_target / 2 - 1, n_prompt), max_target).
 * The prefix is never part of the output.  A prefix fails while either threshold of cw_set_thresholds is set (not NaN).
 * cw_transcribe(...) == cw_transcribe_prompted(..., NULL, 0, ...).                                                 */
int32_t cw_transcribe_prompted(cw_ctx* ctx, int32_t B, const int32_t* num_frames, const cw_transcribe_cfg* cfg,
                               const int32_t* prefix, int32_t n_prefix, int32_t* tokens, float* token_ts, int32_t* lens,
                               int32_t cap, int32_t* n_passes);

/* Language identification (Whisper's detect_language, generation_whisper.py:1610-1673) over the nb windows already encoded:
 * one decoder forward on <|startoftranscript|> at position 0, made as cw_decode makes its position 0 (the same kernels at
 * every row count, so the logits are those of cw_decode(prompt = sot, max_length 2) bit for bit), then one kernel
 * (csrc/langid.hip) on the logits where the forward left them -- they never leave the device; the results are one copy of
 * nb * (n_lang + 2) * 4 bytes.  lang_ids [n_lang]: the candidate language tokens, 1 .. CW_LANG_IDS_MAX distinct ids inside
 * the vocabulary (all of generation_config.lang_to_id, or the languages a deployment expects).
 *   best [nb]             the candidate with the largest logit, lowest token id on an exact tie; a NaN logit is never a candidate
 *   prob [nb][n_lang]     (nullable) expf(l_k - m) / S in table order, m the maximum over the candidates and S the f32 sum of
 *                         expf(l_j - m) over the candidates: softmax with every other column masked, not a softmax over the
 *                         vocabulary.  A candidate at -inf gets exactly 0.  No candidate above -inf: best is the lowest
 *                         candidate id and every prob is NaN.
 *   no_speech [nb]        (nullable) softmax of the same logits over the whole vocabulary at token no_timestamps_token_id - 1
 *                         (the quantity of cw_no_speech_probs, in f32 on the device).
 * cw_get_logits afterwards returns the logits the kernel consumed.  Refused before anything is launched: CW_ERR_INVALID for a
 * null lang_ids / best, n_lang outside 1 .. CW_LANG_IDS_MAX, an id outside the vocabulary, a duplicate id; CW_ERR_STATE for nb
 * above the encoded windows or before cw_set_generation.
 * cw_transcribe / cw_transcribe_prompted with language_token < 0 detect through it over cfg->lang_ids: an id listed more than
 * once there counts once, as it always has; more than CW_LANG_IDS_MAX distinct ids are refused with CW_ERR_INVALID (the host
 * loop this replaces took any number; Whisper has at most 100 languages).
 * cw_get_transcribe_languages: the language token every item of the last cw_transcribe / cw_transcribe_prompted was decoded
 * with, and its detection probability (NaN where the language was forced).  A forced cfg->language_token that is not among
 * cfg->lang_ids (when those are given) is no language: -1 is reported for it.                                              */
#define CW_LANG_IDS_MAX 128
int32_t cw_detect_language(cw_ctx* ctx, int32_t nb, int32_t sot_token, const int32_t* lang_ids, int32_t n_lang,
                           int32_t* best /* [nb] */, float* prob /* [nb][n_lang], nullable */,
                           float* no_speech /* [nb], nullable */);
int32_t cw_get_transcribe_languages(cw_ctx* ctx, int32_t* lang_token /* [B] */, float* prob /* [B] */, int32_t B);
/* cw_test_language_probs: the kernel of cw_detect_language, through the same launcher, on caller-supplied rows: logits [nb][V]
 * go into the context's logits buffer with its real row stride, the pad columns hold +75 during the call (they must never
 * count).  nospeech_token -1: no no-speech part (no_speech, if given, is NaN).                                              */
int32_t cw_test_language_probs(cw_ctx* ctx, const float* logits /* [nb][V] */, int32_t nb, const int32_t* lang_ids,
                               int32_t n_lang, int32_t nospeech_token, int32_t* best, float* prob, float* no_speech);

/* ---- beam search (the transformers 5.x ASR pipeline defaults to num_beams = 5,
 * TF/pipelines/automatic_speech_recognition.py:160-163): device half of GenerationMixin._beam_search
 * (TF/generation/utils.py:3208-3520) over the encoded windows 0..n_items-1, items x beams decoder rows (row = item *
 * num_beams + beam; the context must have been created with max_batch >= items x beams).
 *   cw_beam_begin    prompt [n_items][n_prompt] replicated over the beams, prompt positions forwarded.
 *   cw_beam_step     one decoder forward for every row + log_softmax + the logits processors (:3402-3403); per row the
 *                    n_cand (<= 64) best processed log-probabilities and their tokens, best first (-inf / -1 padded).
 *   cw_beam_advance  the caller chose, for every row, the row it descends from (same item) and its next token
 *                    (:3125-3170, :3480-3486): token history, self-attention cache ancestry and decoder input follow.
 *   cw_beam_finish   row_of_pos [n_items][L]: for every returned sequence and decoder input position, the row whose
 *                    forward pass produced it (HF's unrolled `beam_indices`, generation_whisper.py:262-303): the
 *                    alignment-head rows are gathered accordingly; cw_token_timestamps(n_items, L, ...) follows.   */
int32_t cw_beam_begin(cw_ctx* ctx, int32_t n_items, int32_t num_beams, const int32_t* prompt, int32_t n_prompt,
                      int32_t max_length, int32_t min_new_tokens);
int32_t cw_beam_step(cw_ctx* ctx, int32_t n_cand, float* cand_logprob, int32_t* cand_token);
int32_t cw_beam_advance(cw_ctx* ctx, const int32_t* parent, const int32_t* token);
int32_t cw_beam_finish(cw_ctx* ctx, int32_t n_items, int32_t L, const int32_t* row_of_pos);

/* Host half of the same search (running / finished hypotheses, length penalty, early-stopping heuristic:
 * TF/generation/utils.py:3147, 3173-3245, 3009-3053; float32 like HF), host-only C++: no cw_ctx, no GPU.  Per decoder step:
 *   cw_beam_step -> cw_beam_host_step (candidates in, parent / token out; 1 = go on, 0 = search over) -> cw_beam_advance.
 * cw_beam_host_result: best hypothesis per item -- sequences [n_items][max_length] (pad / eos filled), beam_indices
 * [n_items][max_length - n_prompt] (flat row of every generated position, -1 behind the end), its score.               */
typedef struct cw_beam_host cw_beam_host;
cw_beam_host* cw_beam_host_new(int32_t n_items, int32_t num_beams, int32_t n_prompt, int32_t max_length, int32_t vocab_size,
                               int32_t eos_token_id, int32_t pad_token_id, double length_penalty, int32_t early_stopping,
                               const int32_t* prompt /* [n_items][n_prompt] */);
int32_t cw_beam_host_step(cw_beam_host* s, const float* cand_logprob, const int32_t* cand_token /* [rows][2 * num_beams] */,
                          int32_t* parent, int32_t* token /* [rows] */);
int32_t cw_beam_host_result(const cw_beam_host* s, int64_t* sequences, int32_t* beam_indices, float* score);
/* The candidate log-probability (the value handed to cw_beam_host_step, before the running score is added) of every generated
 * token of the best hypothesis, followed along its ancestry: out [n_items][max_length - n_prompt], NaN behind the end.       */
int32_t cw_beam_host_token_logprobs(const cw_beam_host* s, float* out);
void cw_beam_host_free(cw_beam_host* s);

/* cw_token_timestamps: _extract_token_timestamps (generation_whisper.py:241-381) on the retained rows:
 * crop to num_frames[b]//2 encoder frames, drop the n_prompt prompt rows, z-score over tokens, median
 * filter, head mean, DTW, jump times.  L = rows retained = max(lengths) - 1.  ts_out [nb][L+1] seconds. */
int32_t cw_token_timestamps(cw_ctx* ctx, int32_t nb, int32_t L, int32_t n_prompt, const int32_t* num_frames,
                            float* ts_out);
/* Alignment scores: how sure the model is of WHEN a token was said.  With the switch on (default off) every run of the timestamp
 * stage -- cw_token_timestamps after a greedy, sampled or beam decode, cw_align_tokens, cw_align_score_tokens, every pass of
 * cw_transcribe / cw_transcribe_prompted; not cw_align_heads -- launches one more kernel behind its DTW, inside the
 * CW_STAGE_TIMESTAMPS timer, on the normalised alignment rows and the first frames the DTW just left on the device.  For token
 * row i of a sequence with n frames (the columns that reached the DTW), rows w[h][i][0 .. n-1] of the Ha alignment heads and
 * first frames fc[0 .. N-1] (fc[N] := n):
 *   lo = fc[i], hi = max(lo + 1, fc[i+1]), window = [max(0, lo - collar_frames), min(n, hi + collar_frames))
 *   T_h = sum_j w[h][i][j],  p_h[j] = w[h][i][j] / T_h,  pbar[j] = mean_h p_h[j]
 *   mass   = sum of pbar[j] over the window: the share of the heads' attention that lies where the path put the token
 *   spread = 0.02 * sqrt(sum_j pbar[j] (j - mu)^2) seconds, mu = sum_j pbar[j] j: how diffuse the attention is, path or no path
 * both NaN when n == 0, when a T_h is 0 or when fc[i] < 0.  Float64 sums in a fixed order (csrc/align.hip), rounded to f32 once:
 * a row's values are bit-identical from run to run and whatever else is in the batch.
 * cw_set_alignment_scores: CW_ERR_INVALID for a negative collar_frames; CW_ERR_STATE for switching it on, or changing the collar,
 * while a beam search is open (cw_beam_begin without cw_beam_finish; the next decode closes it).  Switching it off, and repeating
 * the setting in force, change nothing and are accepted in any state.  Allocates two
 * [max_batch][max_target_positions] f32 buffers on first use.  While off nothing is launched, allocated or copied, and every
 * other output is bit-identical either way.
 * cw_get_alignment_scores: those of the last timestamp stage, mass / spread [nb][L+1] in cw_token_timestamps' indexing (after
 * cw_align_tokens / cw_align_score_tokens: L = the longest row's n_ids - 1); NaN at prompt positions, in the eos slot and
 * behind a row's end.  CW_ERR_STATE while off, for more rows than were scored, or for an L below a row's own.
 * cw_get_transcribe_alignment_scores: those of the last cw_transcribe / cw_transcribe_prompted, carried through segment slicing
 * and eos stripping exactly as the token timestamps are: [B][cap] aligned with its `tokens` (NaN behind lens[i]).          */
int32_t cw_set_alignment_scores(cw_ctx* ctx, int32_t on, int32_t collar_frames);
int32_t cw_get_alignment_scores(cw_ctx* ctx, float* mass, float* spread /* [nb][L+1] */, int32_t nb, int32_t L);
int32_t cw_get_transcribe_alignment_scores(cw_ctx* ctx, float* mass, float* spread /* [B][cap] */, int32_t B, int32_t cap);

/* cw_align_tokens: forced alignment of known token sequences.  Encodes the nb resident feature items (cw_mel /
 * cw_set_features), runs one teacher-forced decoder forward of row b over ids[b][0 .. n_ids[b]-2] (the n_init init tokens
 * <|startoftranscript|><|lang|>[<|task|>], then the transcript; the last id, eos, is only predicted), records the alignment
 * heads' cross-attention at exactly the positions a finished greedy generation of the same sequence leaves them, and runs
 * the cw_token_timestamps stages on every row over its own n_ids[b] - 1 rows, so a row's result does not depend on the other
 * rows of the batch.  token_ts [nb][ids_stride]: entries 0 .. n_ids[b]-1 of row b in cw_token_timestamps' convention (the init
 * tokens 0, the eos the time of the token before it); the rest is not written.
 * On the 16-bit engines with the 16-bit cross cache the forward is one batched prefill (csrc/prefill.hip) that stops after the
 * last layer holding an alignment head; the f32 engine, the e4m3 cross cache and cw_set_option "align_prefill" = 0 run it
 * through the per-position decoder step (cw_decode with every generated token forced).
 * CW_ERR_INVALID, before anything is launched: nb outside 1 .. max_batch, an id outside the vocabulary, eos before a row's
 * last id, n_ids[b] outside n_init + 1 .. min(max_target_positions, ids_stride), num_frames[b] outside 0 .. 3000.        */
int32_t cw_align_tokens(cw_ctx* ctx, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                        const int32_t* n_ids, int32_t n_init, float* token_ts);
/* cw_align_prefill_runs: how many cw_align_tokens calls of this context ran their forward as the batched prefill.        */
int32_t cw_align_prefill_runs(cw_ctx* ctx);

/* cw_align_heads: cw_align_tokens for any set of decoder cross-attention heads at once -- what alignment-head selection needs.
 * Same inputs, checks, encoder pass and forward path as cw_align_tokens (the batched prefill on the 16-bit engines with the
 * 16-bit cross cache, else the forced per-position loop), but the n_heads heads (layers[k], heads[k]) are recorded instead of the
 * context's own: for the duration of the call the alignment outputs are a call-local buffer [nb][n_heads][rows][1500] f32 (rows =
 * the longest row's positions), and the prefill stops after the cross-attention of the highest requested layer.  The timestamp
 * stages then run on every (item, head) pair on its own (one head, no head mean), with the frame count of item b computed as
 * cw_align_tokens computes it.  token_ts [n_heads][nb][ids_stride] in request order: row (k, b) is bit-identical to what
 * cw_align_tokens writes for item b in a context whose only alignment head is (layers[k], heads[k]).
 * ref_begin / ref_end [nb][ids_stride] (seconds, NaN = no reference; both null: no similarity): reference interval of the
 * token at the same index.  similarity [n_heads][nb][ids_stride] (null allowed) then receives, for every text token with a
 * finite interval, the cosine between its normalised attention row a and the interval's target g over the item's frames:
 * g = 1 on frames f0 = floor(begin / 0.02) .. f1 - 1, f1 = max(f0 + 1, ceil(end / 0.02)), 1 - k / 5 on the k-th frame outside
 * either end (k = 1 .. 4), 0 elsewhere; with clip_frames >= 0, a counts as 0 outside [f0 - clip_frames, f1 + clip_frames).
 * NaN where undefined (init tokens, eos, no reference, a zero norm).  Computed on the device: the rows are never copied out.
 * On return, success or not, the context's own alignment heads are back in place and no alignment rows are retained
 * (cw_token_timestamps / cw_get_alignment are refused until the next decode).
 * CW_ERR_INVALID, before any device work: what cw_align_tokens refuses, n_heads < 1, a pair outside the decoder's layers x
 * heads, a pair given twice, exactly one of ref_begin / ref_end null, a capture above CW_ALIGN_HEADS_MAX_BYTES.            */
#define CW_ALIGN_HEADS_MAX_BYTES (8ull << 30)
int32_t cw_align_heads(cw_ctx* ctx, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                       const int32_t* n_ids, int32_t n_init, int32_t n_heads, const int32_t* layers, const int32_t* heads,
                       float* token_ts, const float* ref_begin, const float* ref_end, int32_t clip_frames, float* similarity);
/* cw_align_heads_times: wall milliseconds of the last cw_align_heads' parts, the stream drained between them: ms[0] forward,
 * [1] normalisation of the rows, [2] similarity (upload, kernel, download; 0 without references), [3] per-head timestamps,
 * [4] the similarity kernel alone (device events).  ms holds 5 floats.                                                       */
int32_t cw_align_heads_times(cw_ctx* ctx, float* ms);
/* cw_test_align_similarity: cw_align_heads' similarity kernel, through the same launcher, on caller-supplied normalised rows
 * attn [B][Ha][N][S] (S a multiple of 4), n_cols [B] <= S, ref_begin / ref_end [B][N] -> out [Ha][B][N].                   */
int32_t cw_test_align_similarity(cw_ctx* ctx, const float* attn, int32_t B, int32_t Ha, int32_t N, int32_t S,
                                 const int32_t* n_cols, const float* ref_begin, const float* ref_end, int32_t clip_frames,
                                 float* out);
/* cw_test_align_path_scores: the alignment-score kernel, through the timestamp stage's launcher, on caller-supplied rows
 * attn [B][Ha][N][S] (S a multiple of 4), n_cols [B] <= S, first_col [B][N] (<= S) -> mass / spread [B][N].                 */
int32_t cw_test_align_path_scores(cw_ctx* ctx, const float* attn, int32_t B, int32_t Ha, int32_t N, int32_t S,
                                  const int32_t* n_cols, const int32_t* first_col, int32_t collar_frames, float* mass,
                                  float* spread);

/* cw_score_tokens: teacher-forced log-probabilities of known token sequences.  rows = n_items * rows_per_item decoder rows,
 * row r scored against resident feature item r / rows_per_item (several candidate texts of one clip share its encoder pass).
 * ids rows are whole decoder inputs exactly as cw_align_tokens takes them (init tokens, text, eos).  Written at index k =
 * n_init .. n_ids[r]-1 of row r (the text tokens and the eos; nothing else is written): token_logprob = log p(ids[k] | audio,
 * ids[0 .. k-1]) over the raw logits -- no suppress lists, no timestamp rules, temperature 1 -- and top_id / top_logprob the
 * arg-max of the same distribution (lowest id on an exact tie).  Each [rows][ids_stride]; top_id / top_logprob may be null.
 * On the 16-bit engines with the 16-bit cross cache the forward is one batched prefill over every layer followed by the
 * scoring head (csrc/score.hip: final LayerNorm, vocabulary projection, log-softmax and gather fused; the logits are never
 * stored); the f32 engine, the e4m3 cross cache and cw_set_option "score_prefill" = 0 run the per-position decoder step with
 * every token forced.  CW_ERR_INVALID, before anything is launched: what cw_align_tokens refuses, rows_per_item < 1, rows
 * over max_batch, a null ids / n_ids / token_logprob.                                                                      */
int32_t cw_score_tokens(cw_ctx* ctx, int32_t n_items, int32_t rows_per_item, const int32_t* ids, int32_t ids_stride,
                        const int32_t* n_ids, int32_t n_init, float* token_logprob, int32_t* top_id, float* top_logprob);
/* cw_align_score_tokens: cw_align_tokens and cw_score_tokens (rows_per_item 1) of the same rows in one forward.  token_ts is
 * bit-identical to cw_align_tokens' (the alignment rows come from launches both forwards make alike), the scores to
 * cw_score_tokens'.                                                                                                        */
int32_t cw_align_score_tokens(cw_ctx* ctx, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                              const int32_t* n_ids, int32_t n_init, float* token_ts, float* token_logprob, int32_t* top_id,
                              float* top_logprob);
/* cw_align_cut_tokens: how much of an offered transcript was spoken inside the window, and the alignment of that part, in the
 * one forward of cw_align_score_tokens (same inputs, checks, encoder pass and forward path).  Row b offers N_b = n_ids[b] -
 * n_init - 1 text tokens.  Beside token_logprob the head reduces, at every scored position k = n_init .. n_ids[b]-1,
 *   stop_logprob[b][k] = logsumexp(logit[n], n in S) - logsumexp(all logits),  S = {eos} + {n >= timestamp_begin}:
 * the log-probability that the text stops before position k (after the last word a window holds, Whisper predicts the end of
 * text or a closing timestamp).  On the device, S_b[n] = sum_{i<n} token_logprob[b][n_init + i] + stop_logprob[b][n_init + n]
 * (float64, ascending) is the log-probability that exactly the first n tokens are the window's text; cut[b] = the n in
 * 0 .. N_b with cut_ok[b][n] != 0 of the largest S_b[n], the lowest on an exact tie, or N_b whatever the mask says where
 * force_all[b] != 0; cut_score[b] = that S_b[n] rounded once to f32.  cut_ok [nb][ids_stride] bytes indexed by n = tokens kept,
 * force_all [nb] bytes.  The timestamp stage then runs with row b shortened to n_init + cut[b] + 1 ids: token_ts[b] holds
 * entries 0 .. n_init + cut[b], exactly what cw_align_tokens writes for ids[b][0 .. n_init + cut[b] - 1] followed by eos (the
 * forward is causal, so a prefix's alignment rows do not depend on what follows; the z-score over tokens is taken over the
 * prefix).  token_logprob, top_id and top_logprob are bit-identical to cw_align_score_tokens', written with stop_logprob for
 * every k; alignment scores (cw_set_alignment_scores) cover the shortened rows.  CW_ERR_INVALID, before anything is launched:
 * what cw_align_score_tokens refuses, a null cut_ok / force_all / cut / cut_score / token_ts / token_logprob / stop_logprob, a
 * row with neither force_all nor a non-zero cut_ok[b][0 .. N_b]; CW_ERR_STATE without alignment heads.                      */
int32_t cw_align_cut_tokens(cw_ctx* ctx, int32_t nb, const int32_t* num_frames, const int32_t* ids, int32_t ids_stride,
                            const int32_t* n_ids, int32_t n_init, const uint8_t* cut_ok, const uint8_t* force_all, int32_t* cut,
                            float* cut_score, float* token_ts, float* token_logprob, float* stop_logprob, int32_t* top_id,
                            float* top_logprob);
/* cw_score_prefill_runs: how many scoring calls of this context ran their forward as the batched prefill.                  */
int32_t cw_score_prefill_runs(cw_ctx* ctx);
/* cw_set_score_top_logprobs: the k best alternatives of every teacher-forced position (0 = off, the default; 1 ..
 * CW_TOP_LOGPROBS_MAX), selected on the device inside the scoring forward of cw_score_tokens / cw_align_score_tokens /
 * cw_align_cut_tokens -- the [M][V] logits are still never stored.  With z[n], n < V, the f32 logits of a scored position as
 * the head computes them and lse the normaliser token_logprob uses there: candidates are the columns with z[n] > -inf (no
 * suppress lists, no timestamp rules, temperature 1; a NaN is none), ordered by value descending, id ascending on an exact
 * tie; rank j holds that column's id and z - lse, ranks at or past the number of candidates -1 / NaN.  Rank 0 is top_id /
 * top_logprob bit for bit, the target's entry (where it is among the k) token_logprob, and every other output of the call is
 * what it is with k = 0.  Independent of cw_set_token_logprobs / cw_set_top_logprobs (the free-running decode), and the
 * captured decode steps stay: the loop path reduces the step's logits behind the step.  CW_ERR_INVALID outside 0 .. 8.
 * cw_get_score_top_logprobs: after one of the three calls, with that call's rows and ids_stride: ids_out / lp_out
 * [rows][ids_stride][k], filled at indices n_init .. n_ids[r]-1 of row r, -1 / NaN elsewhere.  CW_ERR_STATE while off, for more
 * rows than the last call scored, for another stride, or when no call has run since the switch was set.                     */
int32_t cw_set_score_top_logprobs(cw_ctx* ctx, int32_t k);
int32_t cw_get_score_top_logprobs(cw_ctx* ctx, int32_t* ids_out, float* lp_out, int32_t rows, int32_t ids_stride);
/* cw_set_score_entropy: the predictive entropy (nats) of every teacher-forced position (default off), computed on the device
 * inside the scoring forward of cw_score_tokens / cw_align_score_tokens / cw_align_cut_tokens -- the [M][V] logits are still
 * never stored.  The definition is that of cw_set_token_entropy over z[n], n < V, the f32 logits of a scored position as the head
 * computes them: entropy = log S - Zc / S over the columns with z[n] > -inf; NaN where a z[n] is NaN or +inf.  The fused head keeps
 * Zc beside its (maximum, sum) pair per lane, merges the 16 lanes of a row, then the vocabulary splits in split order; the loop
 * path's row kernel takes it from the step's logits.  It can be combined with cw_set_score_top_logprobs and with the stop form of
 * cw_align_cut_tokens; every other output of the call is what it is with the switch off.
 * cw_get_score_entropy: after one of the three calls, with that call's rows and ids_stride: out [rows][ids_stride], filled at
 * indices n_init .. n_ids[r]-1 of row r, NaN elsewhere (indexing as cw_get_score_top_logprobs).  CW_ERR_STATE while off, for more
 * rows than the last call scored, for another stride, or when no call has run since the switch was set.                     */
int32_t cw_set_score_entropy(cw_ctx* ctx, int32_t on);
int32_t cw_get_score_entropy(cw_ctx* ctx, float* out, int32_t rows, int32_t ids_stride);

/* ---- stand-alone differential-test entry points for the alignment kernels ---------------------------- */
/* attn [B][Ha][N][M] -> mat [B][N][M] (z-score, median(width), head mean); n_cols[b] <= M columns used.  */
int32_t cw_align_matrix(cw_ctx* ctx, const float* attn, int32_t B, int32_t Ha, int32_t N, int32_t M,
                        const int32_t* n_cols, int32_t width, float* mat_out);
/* _dynamic_time_warping(-mat) (generation_whisper.py:64-115): text_idx/time_idx [N+M] forward order.    */
int32_t cw_dtw(cw_ctx* ctx, const float* mat, int32_t N, int32_t M, int32_t* text_idx, int32_t* time_idx,
               int32_t* path_len);
/* ---- seam 4: adjust_pauses_for_hf_pipeline_output (REF/utils.py:1-29) on word start/end arrays, in place */
int32_t cw_adjust_pauses(cw_ctx* ctx, double* start, double* end, int32_t W, double split_threshold);

/* ---- seam 3: tokenizer._decode_asr(..., return_timestamps="word") (TF/models/whisper/tokenization_whisper.py
 * :901-1406), host-only (no GPU): chunk-seam merge, word grouping, punctuation merge, 0.01 s rounding.
 * Vocabulary: byte-level BPE table.  blob/offsets[n_tokens+1]: raw bytes of each text token; kind[i]: 0 text,
 * 1 special (<|...|>), 2 other (timestamp tokens); lang_class[i] for specials: -1 not a language tag, 0 language
 * written with spaces, 1 language without spaces (zh/ja/th/lo/my/yue: split on unicode points, :1299-1304).      */
typedef struct cw_vocab cw_vocab;
typedef struct cw_collator cw_collator;
cw_vocab* cw_vocab_create(int32_t n_tokens, const uint8_t* blob, const int64_t* offsets, const int8_t* kind,
                          const int8_t* lang_class, int32_t eos, int32_t timestamp_begin, int32_t startofprev,
                          int32_t sot, int32_t default_lang_class);
void cw_vocab_destroy(cw_vocab* v);
cw_collator* cw_collate_begin(const cw_vocab* v, double time_precision);
/* mode 0 (default): word chunks (return_timestamps="word"); mode 1: one chunk per timestamp-delimited segment
 * (return_timestamps=True, :1060-1075): token_ts is ignored, a missing start/end comes back as NaN                   */
int32_t cw_collate_set_mode(cw_collator* c, int32_t mode);
/* one pipeline output (chunk) in audio order: tokens [n_tokens], token_ts [n_ts] seconds, stride in seconds     */
int32_t cw_collate_feed(cw_collator* c, const int64_t* tokens, int32_t n_tokens, const float* token_ts, int32_t n_ts,
                        int32_t has_stride, double chunk_len, double stride_left, double stride_right);
/* flushes leftovers; returns sizes: words, utf-8 bytes of the full text / of all word texts, warned = 1 when
 * Whisper did not predict an ending timestamp (:1112-1116)                                                       */
int32_t cw_collate_finish(cw_collator* c, int32_t* n_words, int64_t* text_bytes, int64_t* words_bytes, int32_t* warned);
int32_t cw_collate_get(cw_collator* c, uint8_t* text, double* starts, double* ends, int64_t* word_offsets /* [n+1] */,
                       uint8_t* words_blob);
/* The tokens behind every word of cw_collate_get: token_index [cw_collate_token_groups_total] holds, word after word, the
 * positions of the word's tokens in the concatenation of all fed token arrays; word k owns token_index[group_offsets[k] ..
 * group_offsets[k + 1]).                                                                                                   */
int64_t cw_collate_token_groups_total(cw_collator* c);
int32_t cw_collate_get_token_groups(cw_collator* c, int64_t* group_offsets /* [n+1] */, int32_t* token_index);
/* The language token in force for every chunk of cw_collate_get (-1: none), by the rules of _decode_asr(return_language=True):
 * a word carries the language token seen last when its segment is flushed (a segment merged across a chunk seam takes the later
 * window's); a segment chunk starts from the language seen last and takes a language token met while it is current.          */
int32_t cw_collate_get_languages(cw_collator* c, int32_t* lang_token /* [n_chunks] */);
void cw_collate_free(cw_collator* c);

/* ---- kernel-level hooks used by the parity tests (host f32 in/out, run in the context's dtype) -------- */
/* process-wide tuning knobs for the tests: "gemm256_min_tiles" = tile count from which the 256x256 GEMM is used */
/* 1 when the library carries the measured-and-rejected kernel variants (built with make EXTRA=-DCW_EXPERIMENTS). */
int32_t cw_has_experiments(void);
int32_t cw_test_set_option(const char* name, int32_t value);
int32_t cw_test_gemm(cw_ctx* ctx, int32_t M, int32_t N, int32_t K, const float* A, const float* W,
                     const float* bias, int32_t gelu, float* out);
/* e4m3 x e4m3 GEMM of the opt-in fp8 encoder mode (row-wise scales, v_mfma_scale_f32_16x16x128_f8f6f4): out = T(A W^T + bias) */
int32_t cw_test_gemm_fp8(cw_ctx* ctx, int32_t M, int32_t N, int32_t K, const float* A, const float* W, const float* bias,
                         int32_t gelu, float* out);
/* One launch of the encoder's tile-GEMM dispatcher with any of its epilogues and either A-operand form, parameters filled the
 * way cw_encode fills them.  Host f32 in / out; A, W and the 16-bit outputs are rounded to / returned from the context's dtype.
 *   epi     0 store, 1 GELU: out [M][ldo] (engine type);  2 f32 residual, 3 GELU + pos[m % T], 5 f32 store: out [M][ldo] f32;
 *           4 head split: N = 2 or 3 times d_model column groups -> out, out1 (, out2), each [M / T][H][S_pad][64] (engine type)
 *   conv    0: A [M][K] row-major.  1: implicit conv1d(k = 3, pad = 1) gather over time-major input rows A [n_rows][C_in]:
 *           row m = b * T_out + t of the operand is the concatenation over tap = 0, 1, 2 of input row
 *           row_off[b] + t * stride + tap - 1, or zeros unless 0 <= t * stride + tap - 1 < row_valid[b];  M = nb * T_out, K = 3 C_in
 *   resid   epi 2: [M][ldo], or null for the in-place form the engine uses (out holds the residual on entry)
 *   fp8     1: A and W are quantised row-wise (cw_test_rownorm mode 2's kernel) and multiplied by the e4m3 GEMM: 16-bit engines,
 *           plain A, epi 0 / 1 / 2 / 4, N % 256 == 0, K % 128 == 0
 * Every output buffer is in / out: its contents are uploaded before the launch and downloaded after it, so a sentinel the caller
 * wrote marks every element the kernel left alone.  Refused (CW_ERR_INVALID) before anything is launched: a null buffer the
 * epilogue needs, K % 64, ldo < N, a conv gather with C_in % 64, K != 3 C_in, M != nb * T_out, a stride other than 1 / 2 or a
 * window outside [0, n_rows), a head split with M % T, d_model % 64, H != d_model / 64, N not 2 or 3 times d_model or S_pad < T,
 * epi 3 without pos / T, and what the fp8 form does not take.                                                                */
typedef struct cw_test_gemm_epi_args {
    int32_t epi, fp8, M, N, K;
    int32_t conv, n_rows, T_out, C_in, stride, nb;
    const int32_t* row_off;   /* [nb] */
    const int32_t* row_valid; /* [nb] */
    const float* A;
    const float* W;           /* [N][K] */
    const float* bias;        /* [N] or null */
    const float* resid;
    const float* pos;         /* epi 3: [T][ldo] */
    int32_t ldo, T, S_pad, H, d_model;
    float* out;
    float* out1;
    float* out2;
} cw_test_gemm_epi_args;
int32_t cw_test_gemm_epi(cw_ctx* ctx, const cw_test_gemm_epi_args* args);
/* One launch of a row kernel on x [rows][d] (f32), gamma / beta [d].  mode 0: LayerNorm -> out [rows][d] (engine type, f32 on the
 * f32 engine; d % 4 == 0).  mode 1: LayerNorm -> e4m3 bytes out8 [rows][d] + scale [rows] (d % 4 == 0, d <= 2048).  mode 2: x
 * rounded to the engine's 16-bit type -> row-wise e4m3 quantisation, out8 + scale (d % 8 == 0; gamma / beta unused).  Modes 1 and
 * 2 belong to the 16-bit engines.  The outputs are in / out like those of cw_test_gemm_epi.                                    */
int32_t cw_test_rownorm(cw_ctx* ctx, int32_t mode, int32_t rows, int32_t d, const float* x, const float* gamma, const float* beta,
                        float* out, uint8_t* out8, float* scale);
/* The mel stage's own buffers as cw_mel / cw_mel_resident left them for items 0 .. B-1 (csrc/mel.hip).  Copies only: nothing is
 * launched and nothing is written on the device.  logspec [B][3000][n_mels] f32: log10(max(mel, 1e-10)) before the clip floor;
 * gmax [B]: the clip maximum, decoded from the ordered-uint form the atomicMax runs on; feats_tm [B][3000][n_mels]: the time-major
 * features conv1 reads, converted from the engine's activation type to f32.  Any of the three may be NULL.                       */
int32_t cw_test_mel_stages(cw_ctx* ctx, int32_t B, float* logspec, float* gmax, float* feats_tm);
int32_t cw_test_gemv(cw_ctx* ctx, int32_t Mb, int32_t N, int32_t K, const float* x, const float* W,
                     const float* bias, const float* ln_g, const float* ln_b, int32_t gelu, float* out);
/* One skinny-M decoder projection (17..64 rows; csrc/skinny.hip) on caller-supplied rows, 16-bit engines.  mode 0: LayerNorm
 * (no affine part) + projection through K-split planes and the finish launch; 1: the same through GELU; 2: residual rows
 * out += x16 W^T + bias by grid atomics.  nks = k-steps of 32 per block (0 = default), reps > 0 also times the launches on cold
 * weights: us[0] GEMM, us[1] finish (microseconds per launch). */
int32_t cw_test_skinny(cw_ctx* ctx, int32_t mode, int32_t Mb, int32_t N, int32_t K, const float* x, const float* W,
                       const float* bias, int32_t nks, int32_t reps, float* out, float* us);
/* One launch of the encoder self-attention: q (pre-scaled) / k / v [B][H][S][64] -> out [B][S][H*64].  The rows S .. S_pad-1 of K
 * and V are zero on the device, as in the engine; those of Q are zero, or NaN after cw_test_set_option("attn_poison_qpad", 1) (the
 * kernels never use them).  out is in / out like the outputs of cw_test_gemm_epi, and rows behind it are guarded: a write there is
 * CW_ERR_STATE.  Refused (CW_ERR_INVALID) before anything is launched: B, H or S < 1, a null buffer.                            */
int32_t cw_test_attention(cw_ctx* ctx, int32_t B, int32_t H, int32_t S, const float* q, const float* k,
                          const float* v, float* out /* [B][S][H*64] */);
/* One launch of the key-split cross-attention decode kernel (CW_ATT_SPLITS = 6 key splits): q [B][H*64] pre-scaled, k / v
 * [B / kv_div][H][S][64] (kv_div rows share one K/V: the hypotheses of an audio item under beam search).  Raw outputs:
 * part_o [6][B][H*64], part_ml [B][H][6][2] = (max, sum) per split; head `align_head` captured as the only alignment head:
 * align [B][S] = exp(s - max of its split), align_ml [B][6][2].                                                     */
#define CW_ATT_SPLITS 6
/* The scoring head (csrc/score.hip) on its own: x [M][D] f32, ln_g / ln_b [D], embed [V][D] (rounded to the engine's 16-bit
 * type), targets [M] in 0 .. V-1 -> logprob / top_id / top_logprob [M].  16-bit engines; D % 32 == 0.                      */
int32_t cw_test_score_head(cw_ctx* ctx, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                           const float* embed, const int32_t* targets, float* logprob, int32_t* top_id, float* top_logprob);
/* ... and its STOP form (cw_align_cut_tokens): also stop_logprob [M] over S = {eos} + {n >= timestamp_begin}, eos in 0 .. V-1,
 * timestamp_begin in 0 .. V (V: S = {eos}).  logprob / top_id / top_logprob are bit-identical to cw_test_score_head's.       */
int32_t cw_test_score_head_stop(cw_ctx* ctx, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                                const float* embed, const int32_t* targets, int32_t eos, int32_t timestamp_begin, float* logprob,
                                int32_t* top_id, float* top_logprob, float* stop_logprob);
/* The cut kernel of cw_align_cut_tokens on caller-supplied scores: logprob / stop_logprob / cut_ok [rows][stride], entries
 * 0 .. n_tok[r] of row r used (n_tok[r] < stride), force_all [rows] -> cut / cut_score [rows].  Any engine.  CW_ERR_INVALID for
 * a row that is neither forced nor allowed any cut.                                                                         */
int32_t cw_test_align_cut(cw_ctx* ctx, int32_t rows, int32_t stride, const int32_t* n_tok, const float* logprob,
                          const float* stop_logprob, const uint8_t* cut_ok, const uint8_t* force_all, int32_t* cut,
                          float* cut_score);
/* Times the scoring head at the context's geometry over M pseudo-random rows: unfused = 0 the fused kernels, 1 the same GEMM
 * writing f32 logits [M][V] plus a row-wise log-softmax pass, 2 the fused STOP form.  avg_ms per repetition (HIP events, one
 * warm-up).                                                                                                                */
int32_t cw_time_score_head(cw_ctx* ctx, int32_t M, int32_t unfused, int32_t iters, float* avg_ms);
/* The TOPK forms of the head (cw_set_score_top_logprobs), k = 1 .. CW_TOP_LOGPROBS_MAX: cw_test_score_head[_stop] plus alt_id /
 * alt_logprob [M][CW_TOP_LOGPROBS_MAX] (ranks >= k hold -1 / NaN).  logits_out non-null: [M][V], the same operands through the
 * head's logits-storing form -- the same MFMA sequence, so the very f32 numbers the fused form selected from.  The device
 * arrays carry guard rows behind row M - 1: a write there is CW_ERR_STATE.                                                  */
int32_t cw_test_score_head_top(cw_ctx* ctx, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                               const float* embed, const int32_t* targets, int32_t k, float* logprob, int32_t* top_id,
                               float* top_logprob, int32_t* alt_id, float* alt_logprob, float* logits_out);
int32_t cw_test_score_head_stop_top(cw_ctx* ctx, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g,
                                    const float* ln_b, const float* embed, const int32_t* targets, int32_t eos,
                                    int32_t timestamp_begin, int32_t k, float* logprob, int32_t* top_id, float* top_logprob,
                                    float* stop_logprob, int32_t* alt_id, float* alt_logprob, float* logits_out);
/* The loop path's row kernel in its TOPK form on caller-supplied f32 logits [rows][ldv] (ldv >= V), any engine: targets [rows]
 * (negative: none) -> logprob / top_id / top_logprob [rows], alt_id / alt_logprob [rows][CW_TOP_LOGPROBS_MAX]; stop_logprob
 * non-null: the STOP form over S = {eos} + {n >= timestamp_begin} as well.                                                  */
int32_t cw_test_score_rows_top(cw_ctx* ctx, int32_t rows, int32_t V, int32_t ldv, const float* logits, const int32_t* targets,
                               int32_t k, int32_t eos, int32_t timestamp_begin, float* logprob, int32_t* top_id,
                               float* top_logprob, float* stop_logprob, int32_t* alt_id, float* alt_logprob);
/* cw_time_score_head's fused forms (stop = 0 / 1) with k alternatives per row; k = 0 times the plain forms in the same loop.  */
int32_t cw_time_score_head_top(cw_ctx* ctx, int32_t M, int32_t k, int32_t stop, int32_t iters, float* avg_ms);
/* The ENT forms (cw_set_score_entropy).  cw_test_score_head_entropy: the head with entropy [M] beside its outputs; stop_logprob
 * non-null joins the STOP form (eos / timestamp_begin as cw_test_score_head_stop), k > 0 the TOPK form (alt_id / alt_logprob as
 * cw_test_score_head_top; NULL with k = 0); logits_out and the guard rows as there.  cw_test_score_rows_entropy: the row kernel
 * likewise, k = 0 .. CW_TOP_LOGPROBS_MAX.  cw_time_score_head_entropy: cw_time_score_head_top's loop with the ENT form on.   */
int32_t cw_test_score_head_entropy(cw_ctx* ctx, int32_t M, int32_t D, int32_t V, const float* x, const float* ln_g, const float* ln_b,
                                   const float* embed, const int32_t* targets, int32_t eos, int32_t timestamp_begin, int32_t k,
                                   float* logprob, int32_t* top_id, float* top_logprob, float* stop_logprob, int32_t* alt_id,
                                   float* alt_logprob, float* entropy, float* logits_out);
int32_t cw_test_score_rows_entropy(cw_ctx* ctx, int32_t rows, int32_t V, int32_t ldv, const float* logits, const int32_t* targets,
                                   int32_t k, int32_t eos, int32_t timestamp_begin, float* logprob, int32_t* top_id,
                                   float* top_logprob, float* stop_logprob, int32_t* alt_id, float* alt_logprob, float* entropy);
int32_t cw_time_score_head_entropy(cw_ctx* ctx, int32_t M, int32_t k, int32_t stop, int32_t iters, float* avg_ms);
/* Decoder prompt prefill kernels (16-bit engines) against a host reference: cw_test_prefill_gemm runs the prefill GEMM over
 * fragment-major packed W with epilogue mode 0 = 16-bit store, 2 = f32 residual add (out: residual in, result out), 3 = erf GELU
 * (K % 32 == 0, N % 16 == 0); cw_test_prefill_attention the flash attention of the prefill (causal over n_keys >= n_q keys, or
 * all n_keys keys of K/V row row / kv_div), no scale applied.                                                                 */
int32_t cw_test_prefill_gemm(cw_ctx* ctx, int32_t mode, int32_t M, int32_t N, int32_t K, const float* A, const float* W,
                             const float* bias, float* out);
int32_t cw_test_prefill_attention(cw_ctx* ctx, int32_t rows, int32_t n_q, int32_t H, int32_t cap, int32_t n_keys, int32_t causal,
                                  int32_t kv_div, const float* q, const float* k, const float* v, float* out);
/* cw_test_prefill_align_attention: the cross mode of the prefill attention with head align_head recording alignment rows (slot
 * 0): q [rows * n_q][H * 64], k / v [rows / kv_div][H][n_keys][64] -> out [rows * n_q][H * 64] and align [rows][n_q][n_keys],
 * the recorded rows after the alignment normalisation (softmax weights of that head).  16-bit engines only.                */
int32_t cw_test_prefill_align_attention(cw_ctx* ctx, int32_t rows, int32_t n_q, int32_t H, int32_t n_keys, int32_t kv_div,
                                        int32_t align_head, const float* q, const float* k, const float* v, float* out,
                                        float* align);
int32_t cw_test_cross_attention(cw_ctx* ctx, int32_t B, int32_t H, int32_t S, int32_t kv_div, const float* q, const float* k,
                                const float* v, int32_t align_head, float* part_o, float* part_ml, float* align,
                                float* align_ml);
/* The same launch and outputs with the query left unfinished, as the fused out-projection stage hands it over (16-bit engines):
 * qa, qb [B][H*64], qw, qbias [H*64] and pstats [ceil(B / 16)][n_pstats][16][2], the per-block (sum, sum of squares) planes of
 * gemv_stack_kernel; the kernel finishes q = rstd (qa + qb - mean qw) + qbias itself.  Dispatched as decode_step does: the
 * context's e4m3 cache (cw_set_option "cross_kv_fp8") -> cw_launch_attn_cross_split_fp8 on the quantised rows, else
 * cw_launch_attn_cross_split, which takes kv_div == 1 to the split kernel and kv_div > 1 to the beam-search matrix-core kernel.
 * part_o and part_ml are in / out.  Refused (CW_ERR_INVALID) before anything runs: the f32 engine, a null buffer, B outside
 * 1 .. 64, H, S or kv_div < 1, B % kv_div, a key split without a key, and whatever the launchers refuse (n_pstats outside
 * 1 .. 128, or 1 .. 96 under beam search; H > 20 or kv_div > 16; beam search on the e4m3 cache).                            */
int32_t cw_test_cross_attention_fused(cw_ctx* ctx, int32_t B, int32_t H, int32_t S, int32_t kv_div, const float* qa,
                                      const float* qb, const float* qw, const float* qbias, const float* pstats,
                                      int32_t n_pstats, const float* k, const float* v, int32_t align_head, float* part_o,
                                      float* part_ml, float* align, float* align_ml);
/* One launch of a load-time rewrite of the 16-bit decode step (16-bit engines), parameters as load_state_dict gives them.
 *   op 0  cw_launch_fold_layernorm: a = W [N][K], s = gamma [K], v = beta [K] -> out16 [N][K] = T(scale W diag(gamma)),
 *         c_out [N] += scale W beta
 *   op 1  cw_launch_fold_product:   a = A [N][J], s [J] or null, v = B [J][K]  -> out16 [N][K] = T((A diag(s) scale) B)
 *   op 2  cw_launch_fold_rowvec:    c_out [N] = (A diag(s) scale) v from a = A [N][J], s [J] or null, v [J];  w_out [N] = row sums
 *         of w16 [N][J] rounded to the engine's type.  Either output may be null, and a / s / v with c_out, w16 with w_out
 *   op 3  cw_launch_wfrag_pack:     a = W [N][K] rounded to the engine's type -> image [ceil(N / 16) * 16 * K], the raw 16-bit
 *         fragment-major image (pad rows included)
 * out16, c_out, w_out and image are in / out.  Refused (CW_ERR_INVALID) before any launch: the f32 engine, an unknown op, a size
 * < 1, a null buffer the op needs, and what the launcher refuses (op 0: K % 4; op 1: N % 64, K % 64, J % 16; op 3: K % 32).     */
typedef struct cw_test_fold_args {
    int32_t op, N, J, K;
    float scale;
    const float* a;
    const float* s;
    const float* v;
    const float* w16;
    float* out16;
    float* c_out;
    float* w_out;
    uint16_t* image;
} cw_test_fold_args;
int32_t cw_test_fold(cw_ctx* ctx, const cw_test_fold_args* args);
/* One cw_launch_gemv_stack call (csrc/decfuse.hip; 16-bit engines) with StackParams filled the way decode_step fills them: W
 * [sum n_tiles * 16][K] rounded to the engine's type (wpk = 1: packed by cw_launch_wfrag_pack first), Mb rows, the launch's nt
 * (0 = chosen by the launcher) and nseg <= 3 segments whose tile0 is the running sum of the earlier n_tiles.  Per segment: x
 * [Mb][K], bias / wsum [n_tiles * 16] or null, resid [Mb][n_tiles * 16] (epi 1), n_tiles, nt (0 = the launch's), epi 0 store / 1
 * residual grid / 2 accumulate, and the in / out buffers out, out2 (epi 1, optional) [Mb][n_tiles * 16] and pstats (epi 1,
 * optional) [ceil(Mb / 16)][pstats_blocks][16][2], pstats_blocks = ceil(n_tiles / effective nt).  Segments that name the same
 * `out` share one device buffer (the two accumulating halves of X2).  zero [zero_n4 * 4]: in / out, cleared by the launch.
 * The device copy of every pstats buffer is followed by guard elements: a write there is CW_ERR_STATE.  Refused (CW_ERR_INVALID)
 * before any launch: the f32 engine, a null buffer, Mb outside 1 .. 64, K % 128 or K > 1280, nseg outside 1 .. 3, nt outside
 * 0 .. 3, n_tiles < 1, an unknown epi, epi 1 without resid, wsum / out2 / pstats with an epilogue that does not use them,
 * shared `out` buffers of different sizes or epilogues other than 2, a pstats_blocks that is not the launch's block count of the
 * segment, zero_n4 < 1 or beyond 256 elements per block of the launch.                                                        */
typedef struct cw_test_stack_seg {
    const float* x;
    const float* bias;
    const float* wsum;
    const float* resid;
    int32_t n_tiles, nt, epi, pstats_blocks;
    float* out;
    float* out2;
    float* pstats;
} cw_test_stack_seg;
typedef struct cw_test_gemv_stack_args {
    int32_t Mb, K, nt, wpk, nseg;
    const float* W;
    cw_test_stack_seg seg[3];
    float* zero;
    int32_t zero_n4;
} cw_test_gemv_stack_args;
int32_t cw_test_gemv_stack(cw_ctx* ctx, const cw_test_gemv_stack_args* args);
/* One call of a launcher of the decode GEMV dispatcher (csrc/gemm.hip) with the arguments decode_step / gemv_ln give it.  Host f32
 * in / out; W and every 16-bit operand are rounded to the context's type; wpk = 1: W is packed by cw_launch_wfrag_pack first.
 *   op 0  cw_launch_gemv: x [Mb][K] (x16 = 1: uploaded as 16-bit rows), W [N][K], bias [N] or null, ln_g / ln_b [K] (both null: no
 *         LayerNorm; ln_b null: the folded form).  epi 1: out [Mb][ldo] 16-bit GELU rows;  2: out [Mb][ldo] = resid + grid(acc +
 *         bias), resid [Mb][ldo], or inplace = 1: out holds the residual on entry and resid == outf (the K-split form);  5 / 7: out
 *         [Mb][ldo] f32 store / GELU;  6: N = 3 d_model, out = q [Mb][d_model], k / v appended to sk / sv [Mb][H][cap][64] at row
 *         pos[b];  8: out [Mb][N] = the 16-bit fragment-major GELU rows (ldo = N), returned un-permuted.  part_o [6][Mb][K] + part_ml
 *         [Mb][H][6][2]: the activations are the combination of the key-split partials (plane = Mb K; x unused).  frag_in = 1: the
 *         producer form -- the hook writes the rounded rows of x fragment-major (frag_index) into the scratch and passes x = null.
 *         The scratch (64 rows) is the hook's own and is passed exactly when gemv_ln passes one (Mb <= 16 or wpk).
 *   op 1  cw_launch_rows_combine: part_o, part_ml -> out [Mb][K], the 16-bit fragment-major rows un-permuted; with pstats
 *         [ceil(Mb / 16)][n_pstats][16][2] also cvec [Mb] = the row sums of the planes' first components over K.
 *   op 2  cw_launch_gemv_own: x = the rounded activation rows a [Mb][K] (written fragment-major by the hook), W [N][K], bias, out
 *         [Mb][N] the residual in place, cvec_in [Mb] -> out, y [Mb][N] (the 16-bit fragment-major rows x_new - c un-permuted) and
 *         stats [N / (16 nt)][64][2] per-block (sum y, sum y^2); nt, the launcher's cw_gemv_own_nt, is reported in *nt.
 *   op 3  cw_launch_gemv_lna: x = y [Mb][K] rounded (fragment-major by the hook), stats_in [n_stats][64][2], wsum [N], W [N][K], bias
 *         -> out [Mb][N], the 16-bit fragment-major GELU rows un-permuted.
 * Every output (out, sk, sv, y, stats, cvec) is in / out: uploaded before the launch and downloaded after it, so a sentinel marks
 * what the kernel left alone.  *frag_tail_ok = 1 when the pad rows Mb .. of every fragment-major output kept their fill.  Every
 * device output is followed by guard elements: a write there is CW_ERR_STATE.  Refused (CW_ERR_INVALID) before the launcher is
 * called: the f32 engine for everything but op 0 with epi 2 / 5 / 6 / 7 and no LayerNorm / combine / wpk / x16 / frag_in, an unknown
 * op or epi, a null buffer the form needs, a size < 1, Mb > 64, K % 128 or K > 5120, N > 65536, ldo < N (epi 8: ldo != N), a combine
 * with H 64 != K or in front of a LayerNorm, inplace or resid with an epilogue other than 2, epi 6 with d_model % 64, N != 3
 * d_model, H 64 != d_model, cap < 1 or a pos[b] outside [0, cap), n_pstats outside 1 .. 256, n_stats < 1; and whatever the launcher
 * itself refuses, reported as its refusal.                                                                                       */
typedef struct cw_test_gemv_epi_args {
    int32_t op, epi, Mb, N, K, ldo, wpk, x16, inplace, frag_in;
    int32_t H, cap, d_model, n_pstats, n_stats;
    const float* x;
    const float* W;
    const float* bias;
    const float* ln_g;
    const float* ln_b;
    const float* resid;
    const float* part_o;
    const float* part_ml;
    const float* pstats;
    const int32_t* pos;
    const float* cvec_in;
    const float* stats_in;
    const float* wsum;
    float* out;
    float* sk;
    float* sv;
    float* y;
    float* stats;
    float* cvec;
    int32_t* nt;           /* out (op 2), may be null */
    int32_t* frag_tail_ok; /* out, may be null */
} cw_test_gemv_epi_args;
int32_t cw_test_gemv_epi(cw_ctx* ctx, const cw_test_gemv_epi_args* args);
/* One launch of the decode self-attention dispatcher (cw_launch_attn_decode: attn_decode_kernel / attn_decode_anc_kernel) with
 * the parameters decode_step gives it: q [B][H*64] pre-scaled, k / v [B / kv_div][H][cap][64], pos [B] (n_keys = 0: row b
 * attends over its pos[b] + 1 keys; n_keys > 0: over n_keys keys, pos[b] = alignment row), anc [B][cap] or NULL (key t of row
 * b in cache row anc[b][t]), short_hist = the host's <= 64-key hint.  out_frag = 1: the 16-bit fragment-major output,
 * returned un-permuted in out [B][H*64] (*frag_tail_ok = 1 when its padding rows B.. were left untouched).  align_head >= 0
 * (fixed n_keys only): that head captured as the only alignment slot into align [B][align_rows][n_keys] (in / out).
 * Rejected before any launch: n_keys > cap, pos[b] outside [0, cap), anc[b][t <= pos[b]] outside [0, B), anc with
 * kv_div > 1, a fixed n_keys or alignment capture.                                                                  */
int32_t cw_test_self_attention(cw_ctx* ctx, int32_t B, int32_t H, int32_t cap, int32_t kv_div, const float* q, const float* k,
                               const float* v, const int32_t* pos, int32_t n_keys, const int32_t* anc, int32_t short_hist,
                               int32_t out_frag, int32_t align_head, int32_t align_rows, float* out, float* align,
                               int32_t* frag_tail_ok);
/* Beam-search state of rows 0..rows-1 after cw_beam_begin / cw_beam_advance: ids [rows][max_target_positions], anc
 * [rows][max_target_positions] (cache row of every key position), pos [rows].                                       */
int32_t cw_test_beam_state(cw_ctx* ctx, int32_t rows, int32_t* ids, int32_t* anc, int32_t* pos);
/* One launch of the beam-search candidate selection as cw_beam_step launches it (log-softmax of the raw row, the logits
 * processors on it, the n_cand best (value, token) pairs per row in (value desc, token asc) order) on caller-supplied rows: logits
 * [nb][vocab], ids [nb][t].  The pad columns of the logits rows hold +75 during the call, the candidate buffers are filled with
 * 0xff bytes and the slice records with 1e30 beforehand.  cand_val / cand_id [max_batch * 64]: the whole candidate buffers
 * afterwards, [nb][n_cand] written.  The kernel form follows cw_test_set_option("beam_topk_1block").  Refused before any launch:
 * a null pointer, nb outside 1 .. min(max_batch, 64), n_cand outside 1 .. 64, n_prompt < 1, t outside n_prompt ..
 * max_target_positions - 1, a negative min_new_tokens, an id outside the vocabulary, an open beam search (its state would be
 * overwritten).                                                                                                             */
int32_t cw_test_beam_topk(cw_ctx* ctx, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                          int32_t min_new_tokens, int32_t n_cand, float* cand_val, int32_t* cand_id);
/* The decoder input rows of the next step as the device holds them, x [rows][d_model].  Read-only.                  */
int32_t cw_test_beam_x(cw_ctx* ctx, int32_t rows, float* x);
/* What the last decoder forward left on the device (differential tests of the decode step's launch plans).  what 0: the
 * cross-query x term of the last layer that ran, out [rows][d_model] f32 (fused layers only); what 1 / 2: rows 0 .. n_pos - 1
 * of the self-attention key / value cache of `layer`, out [rows][heads][n_pos][64] in the engine's element type; what 3: one
 * int32, 1 when a forward of `rows` rows computes the x term in the q/k/v launch (the two-segment fused stage).            */
int32_t cw_test_decode_state(cw_ctx* ctx, int32_t what, int32_t layer, int32_t rows, int32_t n_pos, void* out);
/* One launch of the fused logits processors + greedy choice (MinNewTokensLength, SuppressTokensAtBegin, SuppressTokens,
 * WhisperTimeStamp: TF/generation/logits_process.py:203-260, 1816-2047; argmax TF/generation/utils.py:2925) on
 * caller-supplied rows: logits [nb][vocab], ids [nb][t] = prompt + tokens generated so far; choice_out [nb] = token for
 * sequence index t.  Uses the lists installed by cw_set_generation.                                               */
int32_t cw_test_sample(cw_ctx* ctx, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                       int32_t min_new_tokens, int32_t max_length, int32_t* choice_out);
/* The same two launches under cw_set_sampling(temperature, seed, row_streams, nb) for this call only (the context's own
 * setting is put back).  Refused before any launch: a null pointer, nb outside 1 .. min(max_batch, 64), an id outside the
 * vocabulary, t outside n_prompt .. max_target_positions - 1, max_length outside n_prompt + 1 .. max_target_positions, a
 * negative min_new_tokens, a temperature cw_set_sampling refuses, a positive temperature without row_streams.            */
int32_t cw_test_sample_seeded(cw_ctx* ctx, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                              int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                              const uint64_t* row_streams, int32_t* choice_out);
/* cw_test_sample_seeded with the per-token log-probability store on for this call: lp_out [nb] = the value stored for sequence
 * index t.  forced_tok [nb] (NULL: none; -1: row not forced) is written at t instead of the choice; choice_out stays the
 * un-forced choice, as cw_decode's argmax_out.                                                                             */
int32_t cw_test_sample_logprobs(cw_ctx* ctx, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                                int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                                const uint64_t* row_streams, const int32_t* forced_tok, int32_t* choice_out, float* lp_out);
/* ... and with cw_set_top_logprobs(k) on for this call as well: top_id_out / top_lp_out [nb][k] = the alternatives stored for
 * sequence index t.  The pad columns of the logits rows (vocab_size .. the padded width) hold +75 during the call, so a kernel
 * that counted them would list them.  The context's own settings are restored afterwards.                                   */
int32_t cw_test_sample_top_logprobs(cw_ctx* ctx, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                                    int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                                    const uint64_t* row_streams, const int32_t* forced_tok, int32_t k, int32_t* choice_out,
                                    float* lp_out, int32_t* top_id_out, float* top_lp_out);
/* cw_test_sample_logprobs with cw_set_token_entropy on for this call as well: ent_out [nb] = the entropy stored for sequence
 * index t.  k = 0 .. CW_TOP_LOGPROBS_MAX: with k > 0 the alternatives ride along as in cw_test_sample_top_logprobs (top_id_out /
 * top_lp_out [nb][k]; NULL is accepted for k = 0).  The pad columns of the logits rows hold +75 during the call.  The context's
 * own settings are restored afterwards.                                                                                       */
int32_t cw_test_sample_entropy(cw_ctx* ctx, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                               int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                               const uint64_t* row_streams, const int32_t* forced_tok, int32_t k, int32_t* choice_out,
                               float* lp_out, float* ent_out, int32_t* top_id_out, float* top_lp_out);
/* ... and with a cw_set_sequence_bias table for this call only (n_seq == 0: none), the context's own table put back
 * afterwards.  proc_lp_out [nb] = the processed-score log-probability term of the token written at t, i.e. what the step adds to
 * the sum behind cw_get_avg_logprobs (0 where it adds nothing).                                                              */
int32_t cw_test_sample_biased(cw_ctx* ctx, int32_t nb, const float* logits, const int32_t* ids, int32_t t, int32_t n_prompt,
                              int32_t min_new_tokens, int32_t max_length, float temperature, uint64_t seed,
                              const uint64_t* row_streams, const int32_t* forced_tok, int32_t k, int32_t n_seq,
                              const int32_t* seq_tokens, const int32_t* seq_lengths, const float* seq_bias, int32_t* choice_out,
                              float* lp_out, int32_t* top_id_out, float* top_lp_out, float* proc_lp_out);

/* ---- measurement -------------------------------------------------------------------------------------- */
#define CW_STAGE_MEL 0
#define CW_STAGE_ENCODER 1
#define CW_STAGE_CROSS_KV 2
#define CW_STAGE_DECODE 3
#define CW_STAGE_TIMESTAMPS 4
#define CW_N_STAGES 5
/* Accumulated HIP-event time per stage (ms) and number of timed invocations since the last reset.        */
int32_t cw_stage_times(cw_ctx* ctx, float* ms /* [CW_N_STAGES] */, int32_t* calls /* [CW_N_STAGES] */, int32_t reset);
/* Times `iters` back-to-back launches of one decode-step kernel on the context's stream with HIP events:
 * which = 0 decode GEMV (fc1 of decoder layer 0, LN fused), 1 cross-attention decode (layer 0).
 * Returns average ms per launch and the algorithmic bytes one launch must move.                          */
int32_t cw_time_kernel(cw_ctx* ctx, int32_t which, int32_t nb, int32_t iters, float* avg_ms, double* algo_bytes);
/* Times ONE launch of the decoder layer exactly as the decode step issues it for `nb` greedy rows (the step's own launch code with
 * the step's arguments; the layers are cycled so that every launch streams its operands from HBM).  stage = index of the launch
 * inside the layer, 0 .. *n_stages - 1 (the count depends on rows, dtype and cache mode); stage = -1 times the whole layer.
 * Returns average ms per launch, the algorithmic bytes it must move, and its kind (cw_decode_stage_name).  Measurement aid of
 * bench.py's roofline block: the reference has no counterpart (it times the pipeline call, /root/reference/transcribe.py:33). */
int32_t cw_time_decode_stage(cw_ctx* ctx, int32_t nb, int32_t stage, int32_t iters, float* avg_ms, double* algo_bytes,
                             int32_t* kind, int32_t* n_stages);
const char* cw_decode_stage_name(int32_t kind);
/* Kernel launches behind stage `stage` of the layer last enumerated by cw_time_decode_stage (2 at 17..64 rows where a preparation
 * launch precedes the GEMV); 0 for an unknown stage. */
int32_t cw_decode_stage_launches(cw_ctx* ctx, int32_t stage);
/* Number of calls this context repeated on the launch-per-stage decoder kernels because blocks of one launch waited for each other
 * in vain (only when the GPU is shared with other work; 0 in normal operation).  After the first one the context stays on those
 * kernels; results are identical either way. */
int32_t cw_handoff_fallbacks(cw_ctx* ctx);
/* ... of which cw_decode did not start over: the decoder kernels record the position of the first forward that ran on a missed
 * hand-off, the host sees it with the one-step lag of its "rows still running" read, rebuilds the sampler's per-row state from the
 * token ids (/root/reference has no counterpart; the state is that of transformers' WhisperTimeStampLogitsProcessor +
 * stopping criteria, generation_whisper.py / logits_process.py:1933-2048) and resumes at that position.  The whole call is
 * repeated instead while a logprob threshold is set (its running sums cannot be rebuilt from ids) or cw_set_token_logprobs is on. */
int32_t cw_handoff_resumes(cw_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
