"""Thin object wrapper over the C ABI: one ``Engine`` = one ``cw_ctx`` on one GPU.

Host side of seam 2 of SURVEY.md section 8b: owns the context, uploads weights, and exposes the device
stages (mel / encode / decode / token timestamps) with numpy host buffers.  No arithmetic of the
hot path happens in Python.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native as N

_GemvEpiArgs = N.GemvEpiArgs     # (test_gemv_epi has a parameter named N)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32))


@dataclasses.dataclass
class ModelSpec:
    """The fields of WhisperConfig / generation_config the path reads."""
    d_model: int
    n_heads: int
    ffn_dim: int
    enc_layers: int
    dec_layers: int
    n_mels: int
    vocab_size: int
    max_target_positions: int = 448
    median_filter_width: int = 7
    alignment_heads: Sequence[Sequence[int]] = ()
    eos_token_id: int = 0
    pad_token_id: int = 0
    decoder_start_token_id: int = 0
    no_timestamps_token_id: int = 0
    max_initial_timestamp_index: Optional[int] = 50
    suppress_tokens: Sequence[int] = ()
    begin_suppress_tokens: Sequence[int] = ()
    lang_to_id: Dict[str, int] = dataclasses.field(default_factory=dict)
    task_to_id: Dict[str, int] = dataclasses.field(default_factory=dict)
    max_length: int = 448
    # generation_config defaults that seed the decoder prompt (generation_whisper.py:1488-1525)
    forced_decoder_ids: Optional[Sequence[Sequence[Optional[int]]]] = None
    language: Optional[str] = None
    task: Optional[str] = None
    # top_k / top_p / min_p / typical_p / repetition_penalty of the checkpoint's generation_config where they are set to
    # something that acts: a sampling call is refused then (temperature is the only warper the sampler implements)
    sampling_warpers: Dict[str, float] = dataclasses.field(default_factory=dict)

    @property
    def timestamp_begin(self) -> int:
        return self.no_timestamps_token_id + 1


class EngineError(RuntimeError):
    pass


class Engine:
    def __init__(self, spec: ModelSpec, dtype: str = "bf16", max_batch: int = 16, device: int = 0,
                 cross_kv_dtype: Optional[str] = None, encoder_gemm_dtype: Optional[str] = None):
        """``dtype``: "f32" (parity engine), "bf16" or "f16" (the 16-bit MFMA engine in bfloat16 / IEEE binary16).
        ``cross_kv_dtype="fp8"`` (16-bit engines only): the decode step streams an OCP e4m3 copy of the cross-attention
        cache, half the bytes of its dominant stream -- an accuracy-gated performance mode, not the parity path.
        ``encoder_gemm_dtype="fp8"`` (16-bit engines only; BASELINE configs[3]): the encoder's qkv / fc1 / fc2 projections and
        the cross-K/V projection run as e4m3 x e4m3 MFMA GEMMs with row-wise scales (weights quantised once after loading,
        activations by the LayerNorm that produces them) -- likewise accuracy-gated, not the parity path.  ``"fp8:fc1"`` (any subset of
        qkv / fc1 / fc2 / cross_kv joined by "+") quantises only those; "fp8:fc1" together with ``cross_kv_dtype="fp8"`` is the
        largest subset that reproduces every reference clip of the batch-64 workload (profiles/r04_fp8_sweep.txt)."""
        self.lib = N.load()
        self.spec = spec
        self.dtype = dtype
        self.max_batch = int(max_batch)
        if not spec.alignment_heads:
            raise ValueError("Model generation config has no `alignment_heads`, token-level timestamps not available.")
        al = _i32([h[0] for h in spec.alignment_heads])
        ah = _i32([h[1] for h in spec.alignment_heads])
        desc = N.ModelDesc(
            d_model=spec.d_model, n_heads=spec.n_heads, ffn_dim=spec.ffn_dim, enc_layers=spec.enc_layers,
            dec_layers=spec.dec_layers, n_mels=spec.n_mels, vocab_size=spec.vocab_size,
            max_target_positions=spec.max_target_positions, median_filter_width=spec.median_filter_width,
            dtype={"f32": N.CW_DTYPE_F32, "fp32": N.CW_DTYPE_F32, "bf16": N.CW_DTYPE_BF16, "f16": N.CW_DTYPE_F16, "fp16": N.CW_DTYPE_F16}[dtype],
            max_batch=self.max_batch, n_align=len(al),
            align_layers=al.ctypes.data_as(C.POINTER(C.c_int32)), align_heads=ah.ctypes.data_as(C.POINTER(C.c_int32)))
        self.ctx = self.lib.cw_create(C.byref(desc), int(device))
        if not self.ctx:
            raise EngineError("cw_create failed: " + (self.lib.cw_last_error(None) or b"?").decode())
        sup, bsup = _i32(list(spec.suppress_tokens)), _i32(list(spec.begin_suppress_tokens))
        cfg = N.GenCfg(
            eos_token_id=spec.eos_token_id, pad_token_id=spec.pad_token_id,
            no_timestamps_token_id=spec.no_timestamps_token_id,
            max_initial_timestamp_index=-1 if spec.max_initial_timestamp_index is None else spec.max_initial_timestamp_index,
            suppress_tokens=sup.ctypes.data_as(C.POINTER(C.c_int32)), n_suppress=len(sup),
            begin_suppress_tokens=bsup.ctypes.data_as(C.POINTER(C.c_int32)), n_begin_suppress=len(bsup))
        self._chk(self.lib.cw_set_generation(self.ctx, C.byref(cfg)))
        self._capture = None
        self.alignment_scores_on = False                # what set_alignment_scores last set (generation.set_alignment_scores reads it)
        if cross_kv_dtype not in (None, "bf16", "f32", "fp8"):
            raise ValueError(f"cross_kv_dtype must be None or 'fp8', got {cross_kv_dtype!r}")
        if cross_kv_dtype == "fp8":
            self._chk(self.lib.cw_set_option(self.ctx, b"cross_kv_fp8", 1))
        sub = encoder_gemm_dtype[4:] if isinstance(encoder_gemm_dtype, str) and encoder_gemm_dtype.startswith("fp8:") else None
        if sub is not None and (not sub or any(t not in ("qkv", "fc1", "fc2", "cross_kv") for t in sub.split("+"))):
            raise ValueError(f"encoder_gemm_dtype {encoder_gemm_dtype!r}: the subset after 'fp8:' is qkv / fc1 / fc2 / cross_kv joined by '+'")
        if sub is None and encoder_gemm_dtype not in (None, "bf16", "f16", "f32", "fp8"):
            raise ValueError(f"encoder_gemm_dtype must be None, 'fp8' or 'fp8:<subset>', got {encoder_gemm_dtype!r}")
        self._enc_fp8 = sub if sub is not None else (encoder_gemm_dtype == "fp8")

    # ------------------------------------------------------------------
    def _chk(self, rc: int):
        if rc != 0:
            raise EngineError(f"native call failed ({rc}): " + (self.lib.cw_last_error(self.ctx) or b"?").decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.cw_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self.lib.cw_sync(self.ctx))

    # ------------------------------------------------------------------ weights
    def load_tensor(self, name: str, array: np.ndarray):
        a = np.ascontiguousarray(array, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        self._chk(self.lib.cw_load_tensor(self.ctx, name.encode(), _ptr(a), shape, a.ndim))

    def load_state_dict(self, weights: Dict[str, np.ndarray]):
        """Uploads every tensor, then fails loudly (naming the absent tensors) if the checkpoint was incomplete."""
        for k, v in weights.items():
            self.load_tensor(k, v)
        self.check_weights()
        if getattr(self, "_enc_fp8", False):
            self.set_encoder_gemm_fp8(self._enc_fp8)

    _ENC8_BITS = {"qkv": 1, "fc1": 2, "fc2": 4, "cross_kv": 8}

    def set_encoder_gemm_fp8(self, on, mask: Optional[int] = None):
        """(Re)build the e4m3 copies of the resident encoder / cross-K/V weights and switch the encoder GEMMs to them, or back.
        ``on``: True (or the legacy int 1) = every GEMM, False / 0 = none; a str of names out of "qkv", "fc1", "fc2", "cross_kv"
        joined by "+" = that subset.  ``mask`` (keyword) gives the subset as bits instead: 1 q/k/v, 2 fc1, 4 fc2, 8 cross-K/V
        projection.  "fc1" (together with the e4m3 cross-attention cache) is the largest subset that reproduces every reference
        clip of the batch-64 workload (profiles/r04_fp8_sweep.txt: 64 / 64; "fc1+fc2" is at 62-63 / 64)."""
        if mask is not None:
            if isinstance(mask, bool) or not 0 <= int(mask) <= 15:
                raise ValueError(f"mask must be a bit mask in 0..15 (1 q/k/v, 2 fc1, 4 fc2, 8 cross-K/V), not {mask!r}")
            value = 16 + int(mask) if int(mask) > 0 else 0
        elif isinstance(on, str):
            names = [t for t in on.split("+") if t]
            unknown = [t for t in names if t not in self._ENC8_BITS]
            if unknown or not names:
                raise ValueError(f"unknown encoder GEMM name(s) {unknown or on!r}: choose from {sorted(self._ENC8_BITS)} joined by '+'")
            value = 16 + sum(self._ENC8_BITS[t] for t in set(names))
        elif isinstance(on, (bool, np.bool_)) or on in (0, 1):
            value = 1 if on else 0
        else:
            raise ValueError(f"set_encoder_gemm_fp8({on!r}): pass True / False, a '+'-joined name list, or mask=<bits>")
        self._chk(self.lib.cw_set_option(self.ctx, b"encoder_gemm_fp8", value))

    def check_weights(self):
        self._chk(self.lib.cw_check_weights(self.ctx))

    # ------------------------------------------------------------------ stages
    def mel(self, clips: List[np.ndarray], return_features: bool = False):
        """clips: list of 1-D float32 arrays (each <= 30 s).  Returns (features or None, n_frames)."""
        B = len(clips)
        ns = _i32([len(c) for c in clips])
        pcm = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float32) for c in clips])) if B else np.zeros(0, np.float32)
        feats = np.empty((B, self.spec.n_mels, N.N_FRAMES), dtype=np.float32) if return_features else None
        nf = np.zeros(B, dtype=np.int32)
        self._chk(self.lib.cw_mel(self.ctx, _ptr(pcm), B, _ptr(ns), _ptr(feats), _ptr(nf)))
        return feats, nf

    def upload_pcm(self, clips: List[np.ndarray]):
        ns = _i32([len(c) for c in clips])
        pcm = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float32) for c in clips]))
        self._chk(self.lib.cw_upload_pcm(self.ctx, _ptr(pcm), len(clips), _ptr(ns)))
        return (ns + 159) // 160

    def mel_resident(self, B: int):
        self._chk(self.lib.cw_mel_resident(self.ctx, B))

    def set_features(self, feats: np.ndarray):
        f = np.ascontiguousarray(feats, dtype=np.float32)
        self._chk(self.lib.cw_set_features(self.ctx, _ptr(f), f.shape[0]))

    def encode(self, item, seek, n_frames):
        item, seek, n_frames = _i32(item), _i32(seek), _i32(n_frames)
        self._chk(self.lib.cw_encode(self.ctx, len(item), _ptr(item), _ptr(seek), _ptr(n_frames)))

    def encoder_output(self, nb: int) -> np.ndarray:
        out = np.empty((nb, N.N_CTX, self.spec.d_model), dtype=np.float32)
        self._chk(self.lib.cw_get_encoder_output(self.ctx, _ptr(out), nb))
        return out

    def decode(self, prompt: np.ndarray, max_length: int, min_new_tokens: int = 0,
               forced: Optional[np.ndarray] = None, want_argmax: bool = False, row_active=None):
        """``row_active`` (cw_decode_rows): rows with 0 start finished; their ids and log-probability sums on the device stay
        what the previous decode left, their ``lens`` entry is 0 and their ``seqs`` row is what the device held."""
        if row_active is not None:
            return self._decode_rows(prompt, max_length, min_new_tokens, forced, want_argmax, row_active)
        prompt = _i32(prompt)
        nb, n_prompt = prompt.shape
        tgt = self.spec.max_target_positions
        seqs = np.zeros((nb, tgt), dtype=np.int32)
        lens = np.zeros(nb, dtype=np.int32)
        amax = np.zeros((nb, tgt), dtype=np.int32) if want_argmax else None
        f = None
        if forced is not None:
            f = np.full((nb, tgt), -1, dtype=np.int32)
            f[:, :forced.shape[1]] = forced
        self._chk(self.lib.cw_decode(self.ctx, nb, _ptr(prompt), n_prompt, int(max_length), int(min_new_tokens),
                                     _ptr(f), _ptr(seqs), _ptr(lens), _ptr(amax)))
        return seqs, lens, amax

    def _decode_rows(self, prompt, max_length, min_new_tokens, forced, want_argmax, row_active):
        prompt = _i32(prompt)
        nb, n_prompt = prompt.shape
        act = _i32(row_active)
        if act.shape != (nb,):
            raise ValueError(f"row_active must hold one entry per row ({nb}), got shape {act.shape}")
        tgt = self.spec.max_target_positions
        seqs = np.zeros((nb, tgt), dtype=np.int32)
        lens = np.zeros(nb, dtype=np.int32)
        amax = np.zeros((nb, tgt), dtype=np.int32) if want_argmax else None
        f = None
        if forced is not None:
            f = np.full((nb, tgt), -1, dtype=np.int32)
            f[:, :forced.shape[1]] = forced
        self._chk(self.lib.cw_decode_rows(self.ctx, nb, _ptr(prompt), n_prompt, int(max_length), int(min_new_tokens),
                                          _ptr(f), _ptr(act), _ptr(seqs), _ptr(lens), _ptr(amax)))
        return seqs, lens, amax

    def set_sampling(self, temperature: float = 0.0, seed: int = 0, row_streams=None):
        """Seeded Gumbel-max sampling for the coming ``decode`` calls (``cw_set_sampling``): ``row_streams`` holds one 64-bit
        stream id per row.  Temperature 0 or no streams: greedy."""
        if row_streams is None or not float(temperature) > 0.0:
            if not float(temperature) >= 0.0:
                raise ValueError(f"temperature must be finite and >= 0, not {temperature!r}")
            self._chk(self.lib.cw_set_sampling(self.ctx, 0.0, 0, None, 0))
            return
        rs = np.ascontiguousarray(row_streams, dtype=np.uint64)
        self._chk(self.lib.cw_set_sampling(self.ctx, float(temperature), int(seed) & (2 ** 64 - 1), _ptr(rs), int(rs.shape[0])))

    def set_thresholds(self, logprob_threshold: Optional[float] = None, no_speech_threshold: Optional[float] = None):
        """Deterministic half of generate_with_fallback (``cw_set_thresholds``); None = unset."""
        nan = float("nan")
        self._chk(self.lib.cw_set_thresholds(self.ctx, nan if logprob_threshold is None else float(logprob_threshold),
                                             nan if no_speech_threshold is None else float(no_speech_threshold)))

    def no_speech_probs(self, nb: int, sot: int) -> np.ndarray:
        out = np.zeros(nb, np.float32)
        self._chk(self.lib.cw_no_speech_probs(self.ctx, nb, int(sot), _ptr(out)))
        return out

    def detect_language(self, nb: int, lang_ids=None, no_speech: bool = True, sot: Optional[int] = None):
        """Language identification over the ``nb`` encoded windows (``cw_detect_language``): one decoder step on
        <|startoftranscript|>, then one kernel on the logits where they lie.  ``lang_ids``: the candidate language tokens
        (default: every value of ``spec.lang_to_id``, ascending).  Returns ``(ids [nb] int32, probs [nb][n_lang] float32 in
        the order of lang_ids, no_speech [nb] float32 or None)``: the softmax over the candidates alone, and the probability
        of the no-speech token over the whole vocabulary."""
        lids = _i32(sorted(set(self.spec.lang_to_id.values())) if lang_ids is None else lang_ids).reshape(-1)
        best = np.zeros(nb, np.int32)
        prob = np.zeros((nb, max(len(lids), 1)), np.float32)
        ns = np.zeros(nb, np.float32) if no_speech else None
        sot = self.spec.decoder_start_token_id if sot is None else sot
        self._chk(self.lib.cw_detect_language(self.ctx, int(nb), int(sot), _ptr(lids), len(lids), _ptr(best), _ptr(prob), _ptr(ns)))
        return best, prob[:, :len(lids)], ns

    def test_language_probs(self, logits: np.ndarray, lang_ids, nospeech_token: int = -1):
        """cw_test_language_probs: the kernel of ``detect_language`` on caller-supplied rows logits [nb][vocab] ->
        (ids, probs, no_speech); the pad columns of the device buffer hold +75 during the call."""
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        if lg.ndim != 2 or lg.shape[1] != self.spec.vocab_size:
            raise ValueError("test_language_probs: logits must be [nb][vocab_size]")
        nb = lg.shape[0]
        lids = _i32(lang_ids).reshape(-1)
        best = np.zeros(nb, np.int32)
        prob = np.zeros((nb, max(len(lids), 1)), np.float32)
        ns = np.zeros(nb, np.float32)
        self._chk(self.lib.cw_test_language_probs(self.ctx, _ptr(lg), nb, _ptr(lids), len(lids), int(nospeech_token),
                                                  _ptr(best), _ptr(prob), _ptr(ns)))
        return best, prob[:, :len(lids)], ns

    def transcribe_languages(self, B: int):
        """(language token int32 [B], detection probability float32 [B], NaN where forced) of the last ``transcribe``
        (``cw_get_transcribe_languages``)."""
        tok = np.zeros(B, np.int32)
        prob = np.zeros(B, np.float32)
        self._chk(self.lib.cw_get_transcribe_languages(self.ctx, _ptr(tok), _ptr(prob), int(B)))
        return tok, prob

    def avg_logprobs(self, nb: int) -> np.ndarray:
        out = np.zeros(nb, np.float32)
        self._chk(self.lib.cw_get_avg_logprobs(self.ctx, _ptr(out), nb))
        return out

    def set_token_logprobs(self, on: bool):
        """Per-token log-probabilities of the free-running decode (``cw_set_token_logprobs``); off by default.  Switching them
        off switches ``set_top_logprobs`` off as well."""
        self._chk(self.lib.cw_set_token_logprobs(self.ctx, 1 if on else 0))
        if not on:
            self._top_k = 0

    def token_logprobs(self, nb: int) -> np.ndarray:
        """[nb, max_target_positions] float32 aligned with the last ``decode``'s sequences: ``logits[tok] -
        logsumexp(logits[:vocab])`` on the raw logits of the step that wrote each token; NaN at prompt positions, behind a
        row's end and for rows never decoded (``cw_get_token_logprobs``)."""
        out = np.empty((nb, self.spec.max_target_positions), np.float32)
        self._chk(self.lib.cw_get_token_logprobs(self.ctx, _ptr(out), nb))
        return out

    def transcribe_token_logprobs(self, lens) -> List[np.ndarray]:
        """The values of the last ``transcribe``, one float32 array per item aligned with its tokens (``lens`` = their
        counts; ``cw_get_transcribe_token_logprobs``)."""
        nb = len(lens)
        cap = max(1, max((int(n) for n in lens), default=1))
        out = np.empty((nb, cap), np.float32)
        self._chk(self.lib.cw_get_transcribe_token_logprobs(self.ctx, _ptr(out), nb, cap))
        return [out[i, :int(n)].copy() for i, n in enumerate(lens)]

    def set_top_logprobs(self, k: int):
        """The ``k`` (0 = off, at most 8) best raw logits of every decode step next to the token log-probabilities
        (``cw_set_top_logprobs``); needs ``set_token_logprobs(True)``."""
        self._chk(self.lib.cw_set_top_logprobs(self.ctx, int(k)))
        self._top_k = int(k)

    def set_token_entropy(self, on: bool):
        """Predictive entropy (nats) of the raw next-token distribution of every decode step, next to the token log-probabilities
        (``cw_set_token_entropy``); off by default, needs ``set_token_logprobs(True)``.  Greedy and sampled decoding only."""
        self._chk(self.lib.cw_set_token_entropy(self.ctx, 1 if on else 0))

    def token_entropy(self, nb: int) -> np.ndarray:
        """[nb, max_target_positions] float32 aligned with the last ``decode``'s sequences: ``log S - Zc / S`` over the raw logits
        of the step that wrote each token, whichever token that was; NaN wherever ``token_logprobs`` holds NaN, and at a step
        whose logits hold a NaN or +inf (``cw_get_token_entropy``)."""
        out = np.empty((nb, self.spec.max_target_positions), np.float32)
        self._chk(self.lib.cw_get_token_entropy(self.ctx, _ptr(out), nb))
        return out

    def transcribe_token_entropy(self, lens) -> List[np.ndarray]:
        """The values of the last ``transcribe``, one float32 array per item aligned with its tokens (``lens`` = their
        counts; ``cw_get_transcribe_token_entropy``)."""
        nb = len(lens)
        cap = max(1, max((int(n) for n in lens), default=1))
        out = np.empty((nb, cap), np.float32)
        self._chk(self.lib.cw_get_transcribe_token_entropy(self.ctx, _ptr(out), nb, cap))
        return [out[i, :int(n)].copy() for i, n in enumerate(lens)]

    def set_sequence_bias(self, table):
        """Phrase boosting in the sampler kernels (``cw_set_sequence_bias``): ``table`` is a sequence of ``(token ids, bias)``
        pairs -- at most 256 distinct sequences of 1 .. 16 ids, finite biases -- with the semantics of transformers'
        SequenceBiasLogitsProcessor; None or an empty one switches it off.  Greedy and sampled decoding only."""
        table = list(table) if table is not None else []
        if not table:
            self._chk(self.lib.cw_set_sequence_bias(self.ctx, 0, None, None, None))
            return
        toks = _i32([t for ids, _ in table for t in ids])
        lens = _i32([len(ids) for ids, _ in table])
        bias = np.ascontiguousarray([b for _, b in table], np.float32)
        self._chk(self.lib.cw_set_sequence_bias(self.ctx, len(table), _ptr(toks), _ptr(lens), _ptr(bias)))

    def clear_sequence_bias(self):
        self.set_sequence_bias(None)

    def top_logprobs(self, nb: int):
        """(ids int32, logprobs float32), both [nb, max_target_positions, k], aligned with the last ``decode``'s sequences: the
        k best raw logits of the step that wrote each position, best first, ties to the lower id; -1 / NaN beyond the number
        of finite logits and wherever ``token_logprobs`` holds NaN (``cw_get_top_logprobs``)."""
        k = max(1, getattr(self, "_top_k", 0))
        ids = np.empty((nb, self.spec.max_target_positions, k), np.int32)
        lp = np.empty((nb, self.spec.max_target_positions, k), np.float32)
        self._chk(self.lib.cw_get_top_logprobs(self.ctx, _ptr(ids), _ptr(lp), nb))
        return ids, lp

    def transcribe_top_logprobs(self, lens):
        """The alternatives of the last ``transcribe``: (ids, logprobs), each one [n_tok][k] array per item aligned with its
        tokens (``lens`` = their counts; ``cw_get_transcribe_top_logprobs``)."""
        nb = len(lens)
        k = max(1, getattr(self, "_top_k", 0))
        cap = max(1, max((int(n) for n in lens), default=1))
        ids = np.empty((nb, cap, k), np.int32)
        lp = np.empty((nb, cap, k), np.float32)
        self._chk(self.lib.cw_get_transcribe_top_logprobs(self.ctx, _ptr(ids), _ptr(lp), nb, cap))
        return ([ids[i, :int(n)].copy() for i, n in enumerate(lens)], [lp[i, :int(n)].copy() for i, n in enumerate(lens)])

    def set_alignment_scores(self, on: bool, collar_frames: int = 0):
        """Alignment scores of every timestamp stage (``cw_set_alignment_scores``); off by default.  ``collar_frames`` >= 0
        widens every token's window of path frames by that many 20 ms frames on either side.  Switching it on (or changing the
        collar) is refused while a beam search is open; switching it off never is."""
        self._chk(self.lib.cw_set_alignment_scores(self.ctx, 1 if on else 0, int(collar_frames)))
        self.alignment_scores_on = bool(on)

    def alignment_scores(self, nb: int, L: int):
        """(mass, spread), both [nb, L + 1] float32 in ``token_timestamps``' indexing, of the last timestamp stage: the share of
        the alignment heads' attention inside the frames the DTW path gave each token, and the attention's spread in seconds; NaN
        at prompt positions, in the eos slot and behind a row's end (``cw_get_alignment_scores``)."""
        mass = np.empty((nb, L + 1), np.float32)
        spread = np.empty((nb, L + 1), np.float32)
        self._chk(self.lib.cw_get_alignment_scores(self.ctx, _ptr(mass), _ptr(spread), nb, L))
        return mass, spread

    def transcribe_alignment_scores(self, lens):
        """The alignment scores of the last ``transcribe``: (mass, spread), each one float32 array per item aligned with its
        tokens (``lens`` = their counts; ``cw_get_transcribe_alignment_scores``)."""
        nb = len(lens)
        cap = max(1, max((int(n) for n in lens), default=1))
        mass = np.empty((nb, cap), np.float32)
        spread = np.empty((nb, cap), np.float32)
        self._chk(self.lib.cw_get_transcribe_alignment_scores(self.ctx, _ptr(mass), _ptr(spread), nb, cap))
        return ([mass[i, :int(n)].copy() for i, n in enumerate(lens)], [spread[i, :int(n)].copy() for i, n in enumerate(lens)])

    def test_align_path_scores(self, attn, n_cols, first_col, collar_frames: int):
        """cw_test_align_path_scores: the alignment-score kernel on rows attn [B][Ha][N][S] (S a multiple of 4), n_cols [B],
        first_col [B][N] -> (mass, spread), both [B][N]."""
        a = np.ascontiguousarray(attn, dtype=np.float32)
        if a.ndim != 4:
            raise ValueError("test_align_path_scores: attn must be [B][Ha][N][S]")
        B, Ha, Nn, S = a.shape
        nc, fc = _i32(n_cols), _i32(first_col)
        if nc.shape != (B,) or fc.shape != (B, Nn):
            raise ValueError("test_align_path_scores: shapes do not agree")
        mass = np.zeros((B, Nn), dtype=np.float32)
        spread = np.zeros((B, Nn), dtype=np.float32)
        self._chk(self.lib.cw_test_align_path_scores(self.ctx, _ptr(a), B, Ha, Nn, S, _ptr(nc), _ptr(fc), int(collar_frames),
                                                     _ptr(mass), _ptr(spread)))
        return mass, spread

    def last_logits(self, nb: int) -> np.ndarray:
        out = np.empty((nb, self.spec.vocab_size), dtype=np.float32)
        self._chk(self.lib.cw_get_logits(self.ctx, _ptr(out), nb))
        return out

    def capture_logits(self, nb: int, max_steps: int) -> np.ndarray:
        self._capture = np.zeros((max_steps, nb, self.spec.vocab_size), dtype=np.float32)
        self._chk(self.lib.cw_set_logits_capture(self.ctx, _ptr(self._capture), max_steps))
        return self._capture

    def stop_capture(self):
        self._chk(self.lib.cw_set_logits_capture(self.ctx, None, 0))
        self._capture = None

    def alignment(self, nb: int, L: int) -> np.ndarray:
        out = np.empty((nb, len(self.spec.alignment_heads), L, N.N_CTX), dtype=np.float32)
        self._chk(self.lib.cw_get_alignment(self.ctx, _ptr(out), nb, L))
        return out

    def ingest(self, raw, fmt: int, channels: int, n_frames: int, sr_in: int, sr_out: int = 16000,
               normalise: bool = False) -> np.ndarray:
        """cw_ingest: interleaved sample frames (bytes or a C-contiguous array) -> mono float32 at ``sr_out``."""
        buf = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.ascontiguousarray(raw)
        n_out = int(self.lib.cw_resampled_length(int(n_frames), int(sr_in), int(sr_out)))
        out = np.empty(n_out, dtype=np.float32)
        self._chk(self.lib.cw_ingest(self.ctx, buf.ctypes.data_as(C.c_void_p), int(fmt), int(channels), int(n_frames),
                                     int(sr_in), int(sr_out), 1 if normalise else 0, _ptr(out)))
        return out

    def transcribe(self, nb: int, num_frames, *, sot: int, language_token: int = -1, task_token: int = -1,
                   max_new_tokens: int = -1, min_new_tokens: int = 0, max_length: int = 448, lang_ids=None, prefix=None):
        """Native seek loop (cw_transcribe) over the nb resident feature items: returns (tokens, timestamps, passes),
        the per-item concatenated segment tokens (int64) and absolute token timestamps (float32).  ``prefix``: decoder
        prompt ids (``prompt_ids``, starting with <|startofprev|>) put in front of every window's init tokens
        (cw_transcribe_prompted)."""
        nf = _i32(num_frames)
        pre = _i32(prefix if prefix is not None else [])
        lids = _i32(lang_ids if lang_ids is not None else [])
        cfg = N.TranscribeCfg(sot, language_token, task_token, max_new_tokens, min_new_tokens, max_length,
                              lids.ctypes.data_as(C.POINTER(C.c_int32)), len(lids))
        # a 30 s window can be re-decoded at most once per 0.02 s of progress; 4 full-length passes is far above
        # what the seek loop can emit before running out of frames with real timestamps, and the call fails loudly
        # (never truncates) if an item exceeds it
        cap = 4 * self.spec.max_target_positions
        while True:
            toks = np.zeros((nb, cap), dtype=np.int32)
            ts = np.zeros((nb, cap), dtype=np.float32)
            lens = np.zeros(nb, dtype=np.int32)
            passes = C.c_int32(0)
            if len(pre):
                rc = self.lib.cw_transcribe_prompted(self.ctx, nb, _ptr(nf), C.byref(cfg), _ptr(pre), len(pre), _ptr(toks),
                                                     _ptr(ts), _ptr(lens), cap, C.byref(passes))
            else:
                rc = self.lib.cw_transcribe(self.ctx, nb, _ptr(nf), C.byref(cfg), _ptr(toks), _ptr(ts), _ptr(lens), cap,
                                            C.byref(passes))
            if rc != 0 and b"capacity" in (self.lib.cw_last_error(self.ctx) or b"") and cap < (1 << 20):
                cap *= 4
                continue
            self._chk(rc)
            break
        return ([toks[i, :lens[i]].astype(np.int64) for i in range(nb)], [ts[i, :lens[i]].copy() for i in range(nb)],
                int(passes.value))

    def align_tokens(self, num_frames, ids, n_init: int) -> List[np.ndarray]:
        """Forced alignment (cw_align_tokens) of the resident feature items 0 .. len(ids)-1: ``ids[b]`` is row b's whole
        sequence, the ``n_init`` init tokens, the transcript and eos.  Returns one float32 array of len(ids[b]) token
        timestamps per row (cw_token_timestamps' convention)."""
        nb = len(ids)
        n = _i32([len(r) for r in ids])
        stride = max(1, int(n.max()) if nb else 1)
        table = np.zeros((nb, stride), dtype=np.int32)
        for b, r in enumerate(ids):
            r = np.asarray(r, dtype=np.int64)
            if r.size and (r.min() < 0 or r.max() >= self.spec.vocab_size):    # before the int32 table could wrap them
                raise ValueError(f"row {b}: token id outside the vocabulary (0 .. {self.spec.vocab_size - 1})")
            table[b, :len(r)] = r
        nf = _i32(num_frames)
        ts = np.zeros((nb, stride), dtype=np.float32)
        self._chk(self.lib.cw_align_tokens(self.ctx, nb, _ptr(nf), _ptr(table), stride, _ptr(n), int(n_init), _ptr(ts)))
        return [ts[b, :n[b]].copy() for b in range(nb)]

    def align_heads(self, num_frames, ids, n_init: int, heads, ref=None, clip_frames: int = 200):
        """Per-head forced alignment (cw_align_heads) of the resident feature items 0 .. len(ids)-1.  ``ids`` as
        ``align_tokens`` takes them; ``heads`` a list of distinct (layer, head) pairs of the decoder.  Returns per head, in the
        order given, what ``align_tokens`` would return with that head as the only alignment head: a list over the heads of
        lists over the rows of float32 arrays of len(ids[b]).  ``ref=(begin, end)``, per row one array of len(ids[b]) seconds
        (NaN: no reference): also returns the similarity of every token's attention row to its interval, in the same shape
        (NaN where undefined), with the row counted as 0 further than ``clip_frames`` frames from the interval (< 0: no
        clipping)."""
        nb = len(ids)
        hd = np.asarray(heads, dtype=np.int64)
        if hd.ndim != 2 or hd.shape[1] != 2 or hd.shape[0] < 1:
            raise ValueError("heads must be a non-empty list of (layer, head) pairs")
        n, stride, table = self._token_table(ids)
        nf = _i32(num_frames)
        nh = hd.shape[0]
        layers, hh = _i32(hd[:, 0]), _i32(hd[:, 1])
        ts = np.zeros((nh, nb, stride), dtype=np.float32)
        rb = re = sim = None
        if ref is not None:
            begin, end = ref
            if len(begin) != nb or len(end) != nb:
                raise ValueError(f"ref holds {len(begin)} / {len(end)} rows for {nb} rows of ids")
            rb = np.full((nb, stride), np.nan, dtype=np.float32)
            re = np.full((nb, stride), np.nan, dtype=np.float32)
            for b in range(nb):
                if len(begin[b]) != n[b] or len(end[b]) != n[b]:
                    raise ValueError(f"ref row {b} holds {len(begin[b])} / {len(end[b])} entries for {n[b]} ids")
                rb[b, :n[b]] = begin[b]
                re[b, :n[b]] = end[b]
            sim = np.zeros((nh, nb, stride), dtype=np.float32)
        self._chk(self.lib.cw_align_heads(self.ctx, nb, _ptr(nf), _ptr(table), stride, _ptr(n), int(n_init), nh, _ptr(layers),
                                          _ptr(hh), _ptr(ts), _ptr(rb), _ptr(re), int(clip_frames), _ptr(sim)))
        out = [[ts[k, b, :n[b]].copy() for b in range(nb)] for k in range(nh)]
        if sim is None:
            return out
        return out, [[sim[k, b, :n[b]].copy() for b in range(nb)] for k in range(nh)]

    def align_heads_times(self):
        """cw_align_heads_times: milliseconds of the last ``align_heads`` call's forward, normalisation, similarity and
        per-head timestamps, and of the similarity kernel alone."""
        ms = np.zeros(5, dtype=np.float32)
        self._chk(self.lib.cw_align_heads_times(self.ctx, _ptr(ms)))
        return {"forward": float(ms[0]), "normalize": float(ms[1]), "similarity": float(ms[2]), "timestamps": float(ms[3]),
                "similarity_kernel": float(ms[4])}

    def test_align_similarity(self, attn, n_cols, ref_begin, ref_end, clip_frames: int) -> np.ndarray:
        """cw_test_align_similarity: the similarity kernel of ``align_heads`` on normalised rows attn [B][Ha][N][S] (S a multiple
        of 4), n_cols [B], ref_begin / ref_end [B][N] seconds -> [Ha][B][N]."""
        a = np.ascontiguousarray(attn, dtype=np.float32)
        if a.ndim != 4:
            raise ValueError("test_align_similarity: attn must be [B][Ha][N][S]")
        B, Ha, Nn, S = a.shape
        nc = _i32(n_cols)
        rb = np.ascontiguousarray(ref_begin, dtype=np.float32)
        re = np.ascontiguousarray(ref_end, dtype=np.float32)
        if nc.shape != (B,) or rb.shape != (B, Nn) or re.shape != (B, Nn):
            raise ValueError("test_align_similarity: shapes do not agree")
        out = np.zeros((Ha, B, Nn), dtype=np.float32)
        self._chk(self.lib.cw_test_align_similarity(self.ctx, _ptr(a), B, Ha, Nn, S, _ptr(nc), _ptr(rb), _ptr(re), int(clip_frames),
                                                    _ptr(out)))
        return out

    def align_prefill_runs(self) -> int:
        """cw_align_prefill_runs: align_tokens calls of this engine whose forward ran as the batched prefill."""
        return int(self.lib.cw_align_prefill_runs(self.ctx))

    def set_align_prefill(self, on: bool):
        """cw_set_option "align_prefill": 0 runs cw_align_tokens' forward through the per-position decoder step."""
        self._chk(self.lib.cw_set_option(self.ctx, b"align_prefill", 1 if on else 0))

    def _token_table(self, ids):
        nb = len(ids)
        n = _i32([len(r) for r in ids])
        stride = max(1, int(n.max()) if nb else 1)
        table = np.zeros((nb, stride), dtype=np.int32)
        for b, r in enumerate(ids):
            r = np.asarray(r, dtype=np.int64)
            if r.size and (r.min() < 0 or r.max() >= self.spec.vocab_size):    # before the int32 table could wrap them
                raise ValueError(f"row {b}: token id outside the vocabulary (0 .. {self.spec.vocab_size - 1})")
            table[b, :len(r)] = r
        return n, stride, table

    def set_score_top_logprobs(self, k: int):
        """cw_set_score_top_logprobs: the k best alternatives (0 = off, 1 .. 8) of every position the scoring calls score."""
        self._chk(self.lib.cw_set_score_top_logprobs(self.ctx, int(k)))

    def _with_score_top(self, k, call, nr, stride, n, n_init):
        """Runs ``call`` (one of the scoring calls) with ``cw_set_score_top_logprobs(k)`` on around it -- off again afterwards,
        also when the call raises -- and returns its alternatives per row: (ids int64 [n][k], logprobs float32 [n][k])."""
        k = int(k)
        if not 1 <= k <= 8:
            raise ValueError(f"top_logprobs must be an integer in 0 .. 8, got {k!r}")
        self.set_score_top_logprobs(k)
        try:
            call()
            ai = np.zeros((nr, stride, k), dtype=np.int32)
            al = np.zeros((nr, stride, k), dtype=np.float32)
            self._chk(self.lib.cw_get_score_top_logprobs(self.ctx, _ptr(ai), _ptr(al), nr, stride))
        finally:
            self.set_score_top_logprobs(0)
        i0 = int(n_init)
        return ([ai[b, i0:n[b]].astype(np.int64) for b in range(nr)], [al[b, i0:n[b]].copy() for b in range(nr)])

    def set_score_entropy(self, on: bool):
        """cw_set_score_entropy: the predictive entropy (nats) of every position the scoring calls score; off by default."""
        self._chk(self.lib.cw_set_score_entropy(self.ctx, 1 if on else 0))

    def score_entropy(self, nr: int, stride: int) -> np.ndarray:
        """cw_get_score_entropy: [nr, stride] float32 of the last scoring call (its rows and ids stride), NaN where nothing was
        scored."""
        out = np.zeros((int(nr), int(stride)), dtype=np.float32)
        self._chk(self.lib.cw_get_score_entropy(self.ctx, _ptr(out), int(nr), int(stride)))
        return out

    def _with_score_extras(self, top_logprobs, entropy, call, nr, stride, n, n_init):
        """Runs ``call`` (one of the scoring calls) under ``top_logprobs`` (``_with_score_top``) and / or with
        ``cw_set_score_entropy`` on around it -- off again afterwards, also when the call raises.  Returns the extra entries of
        the call's result: the alternatives (ids, logprobs) when ``top_logprobs``, then the entropies per row (float32 [n]) when
        ``entropy``."""
        if not entropy:
            return self._with_score_top(top_logprobs, call, nr, stride, n, n_init) if top_logprobs else call() or ()
        self.set_score_entropy(True)
        try:
            alts = self._with_score_top(top_logprobs, call, nr, stride, n, n_init) if top_logprobs else call() or ()
            en = self.score_entropy(nr, stride)
        finally:
            self.set_score_entropy(False)
        i0 = int(n_init)
        return tuple(alts) + ([en[b, i0:n[b]].copy() for b in range(nr)],)

    def score_tokens(self, rows, n_init: int, rows_per_item: int = 1, top_logprobs: int = 0, entropy: bool = False):
        """Teacher-forced log-probabilities (cw_score_tokens): ``rows[r]`` is a whole decoder input (``n_init`` init tokens,
        transcript, eos), scored against resident feature item r // rows_per_item.  Returns (logprob, top_id, top_logprob):
        per row one array over its text tokens and the eos (len(rows[r]) - n_init entries) -- log p(token | audio, tokens
        before it) over the raw logits, and the arg-max id of the same distribution with its log-probability.
        ``top_logprobs=k`` (1 .. 8): two more entries, per row the ids [n][k] and log-probabilities [n][k] of the k best
        tokens of every scored position, best first, ties to the lower id, -1 / NaN past the candidates
        (``cw_set_score_top_logprobs``).  ``entropy=True``: one more entry behind those, per row the predictive entropy (nats,
        float32) of every scored position's distribution (``cw_set_score_entropy``)."""
        nr = len(rows)
        rpi = int(rows_per_item)
        if rpi >= 1 and nr % rpi:
            raise ValueError(f"{nr} rows are not a multiple of rows_per_item={rpi}")
        n, stride, table = self._token_table(rows)
        lp = np.zeros((nr, stride), dtype=np.float32)
        ti = np.zeros((nr, stride), dtype=np.int32)
        tl = np.zeros((nr, stride), dtype=np.float32)
        def call():
            self._chk(self.lib.cw_score_tokens(self.ctx, nr // rpi if rpi >= 1 else nr, rpi, _ptr(table), stride, _ptr(n), int(n_init),
                                               _ptr(lp), _ptr(ti), _ptr(tl)))
        alts = self._with_score_extras(top_logprobs, entropy, call, nr, stride, n, n_init)
        k = int(n_init)
        return ([lp[b, k:n[b]].copy() for b in range(nr)], [ti[b, k:n[b]].astype(np.int64) for b in range(nr)],
                [tl[b, k:n[b]].copy() for b in range(nr)]) + tuple(alts)

    def align_score_tokens(self, num_frames, ids, n_init: int, top_logprobs: int = 0, entropy: bool = False):
        """cw_align_score_tokens: ``align_tokens`` and ``score_tokens`` (one row per item) of the same rows in one forward.
        Returns (timestamps as align_tokens, logprob, top_id, top_logprob as score_tokens[, with ``top_logprobs=k`` its
        alternative ids and log-probabilities][, with ``entropy=True`` the positions' entropies])."""
        nb = len(ids)
        n, stride, table = self._token_table(ids)
        nf = _i32(num_frames)
        ts = np.zeros((nb, stride), dtype=np.float32)
        lp = np.zeros((nb, stride), dtype=np.float32)
        ti = np.zeros((nb, stride), dtype=np.int32)
        tl = np.zeros((nb, stride), dtype=np.float32)
        def call():
            self._chk(self.lib.cw_align_score_tokens(self.ctx, nb, _ptr(nf), _ptr(table), stride, _ptr(n), int(n_init), _ptr(ts),
                                                     _ptr(lp), _ptr(ti), _ptr(tl)))
        alts = self._with_score_extras(top_logprobs, entropy, call, nb, stride, n, n_init)
        k = int(n_init)
        return ([ts[b, :n[b]].copy() for b in range(nb)], [lp[b, k:n[b]].copy() for b in range(nb)],
                [ti[b, k:n[b]].astype(np.int64) for b in range(nb)], [tl[b, k:n[b]].copy() for b in range(nb)]) + tuple(alts)

    def align_cut_tokens(self, num_frames, ids, n_init: int, cut_ok, force_all, top_logprobs: int = 0, entropy: bool = False):
        """cw_align_cut_tokens: how much of each offered transcript was spoken inside its window, and the alignment of that part,
        in the one forward of ``align_score_tokens``.  ``ids`` as ``align_tokens`` takes them (row b offers N_b = len(ids[b]) -
        n_init - 1 text tokens); ``cut_ok[b]``: N_b + 1 flags, entry n allowing "keep the first n tokens"; ``force_all[b]``: keep
        all N_b whatever the flags say.  Returns (cut [nb] int64, cut_score [nb] float32, timestamps: per row n_init + cut[b] + 1
        entries, what ``align_tokens`` gives for the kept prefix followed by eos, logprob / stop_logprob / top_id / top_logprob: per
        row len(ids[b]) - n_init entries as ``score_tokens`` returns them).  stop_logprob[k] is the log-probability that the
        text stops before position k (eos or any timestamp token); cut maximises sum(logprob[:n]) + stop_logprob[n] over the
        allowed n, the lowest n on an exact tie.  ``top_logprobs=k``: two more entries, the alternatives as ``score_tokens``
        returns them (every offered position, not the kept prefix only).  ``entropy=True``: one more entry behind those, the
        positions' entropies as ``score_tokens`` returns them."""
        nb = len(ids)
        n, stride, table = self._token_table(ids)
        if len(cut_ok) != nb or len(force_all) != nb:
            raise ValueError(f"cut_ok / force_all hold {len(cut_ok)} / {len(force_all)} rows for {nb} rows of ids")
        k = int(n_init)
        ok = np.zeros((nb, stride), dtype=np.uint8)
        for b in range(nb):
            m = np.asarray(cut_ok[b]).astype(bool)
            if m.shape != (max(0, int(n[b]) - k),):
                raise ValueError(f"cut_ok[{b}] holds {m.shape} flags for {int(n[b]) - k - 1} text tokens (one per count 0 .. N)")
            ok[b, :len(m)] = m
        force = np.ascontiguousarray(np.asarray(force_all).astype(bool), dtype=np.uint8)
        nf = _i32(num_frames)
        cut = np.zeros(nb, dtype=np.int32)
        score = np.zeros(nb, dtype=np.float32)
        ts = np.zeros((nb, stride), dtype=np.float32)
        lp = np.zeros((nb, stride), dtype=np.float32)
        sl = np.zeros((nb, stride), dtype=np.float32)
        ti = np.zeros((nb, stride), dtype=np.int32)
        tl = np.zeros((nb, stride), dtype=np.float32)
        def call():
            self._chk(self.lib.cw_align_cut_tokens(self.ctx, nb, _ptr(nf), _ptr(table), stride, _ptr(n), k, _ptr(ok), _ptr(force),
                                                   _ptr(cut), _ptr(score), _ptr(ts), _ptr(lp), _ptr(sl), _ptr(ti), _ptr(tl)))
        alts = self._with_score_extras(top_logprobs, entropy, call, nb, stride, n, k)
        return (cut.astype(np.int64), score, [ts[b, :k + cut[b] + 1].copy() for b in range(nb)],
                [lp[b, k:n[b]].copy() for b in range(nb)], [sl[b, k:n[b]].copy() for b in range(nb)],
                [ti[b, k:n[b]].astype(np.int64) for b in range(nb)], [tl[b, k:n[b]].copy() for b in range(nb)]) + tuple(alts)

    def test_score_head_stop(self, x, ln_g, ln_b, embed, targets, eos: int, timestamp_begin: int):
        """cw_test_score_head_stop: ``test_score_head`` through the STOP form of the head -> (logprob, top_id, top_logprob,
        stop_logprob) [M], stop_logprob over S = {eos} + {n >= timestamp_begin}."""
        x = np.ascontiguousarray(x, np.float32)
        embed = np.ascontiguousarray(embed, np.float32)
        g = np.ascontiguousarray(ln_g, np.float32)
        b = np.ascontiguousarray(ln_b, np.float32)
        t = _i32(targets)
        M, D = x.shape
        V = embed.shape[0]
        if embed.shape[1] != D or g.shape != (D,) or b.shape != (D,) or t.shape != (M,):
            raise ValueError("test_score_head_stop: shapes do not agree")
        lp = np.zeros(M, np.float32)
        ti = np.zeros(M, np.int32)
        tl = np.zeros(M, np.float32)
        sl = np.zeros(M, np.float32)
        self._chk(self.lib.cw_test_score_head_stop(self.ctx, M, D, V, _ptr(x), _ptr(g), _ptr(b), _ptr(embed), _ptr(t), int(eos),
                                                   int(timestamp_begin), _ptr(lp), _ptr(ti), _ptr(tl), _ptr(sl)))
        return lp, ti, tl, sl

    def test_align_cut(self, logprob, stop_logprob, cut_ok, force_all):
        """cw_test_align_cut: the cut kernel on caller-supplied scores.  Per row r ``logprob[r]`` / ``stop_logprob[r]`` /
        ``cut_ok[r]`` hold N_r + 1 entries (N_r text tokens; the last logprob is the eos's); ``force_all`` [rows] ->
        (cut [rows] int64, cut_score [rows] float32)."""
        rows = len(logprob)
        if not (len(stop_logprob) == len(cut_ok) == len(force_all) == rows):
            raise ValueError("test_align_cut: row counts do not agree")
        n_tok = _i32([len(r) - 1 for r in logprob])
        stride = max(1, int(n_tok.max()) + 1 if rows else 1)
        lp = np.zeros((rows, stride), np.float32)
        sl = np.zeros((rows, stride), np.float32)
        ok = np.zeros((rows, stride), np.uint8)
        for r in range(rows):
            m = int(n_tok[r]) + 1
            if m < 1 or len(stop_logprob[r]) != m or len(cut_ok[r]) != m:
                raise ValueError(f"test_align_cut: row {r} needs the same non-zero number of logprob / stop_logprob / cut_ok entries")
            lp[r, :m] = logprob[r]
            sl[r, :m] = stop_logprob[r]
            ok[r, :m] = np.asarray(cut_ok[r]).astype(bool)
        force = np.ascontiguousarray(np.asarray(force_all).astype(bool), dtype=np.uint8)
        cut = np.zeros(rows, np.int32)
        score = np.zeros(rows, np.float32)
        self._chk(self.lib.cw_test_align_cut(self.ctx, rows, stride, _ptr(n_tok), _ptr(lp), _ptr(sl), _ptr(ok), _ptr(force),
                                             _ptr(cut), _ptr(score)))
        return cut.astype(np.int64), score

    def score_prefill_runs(self) -> int:
        """cw_score_prefill_runs: scoring calls of this engine whose forward ran as the batched prefill."""
        return int(self.lib.cw_score_prefill_runs(self.ctx))

    def set_score_prefill(self, on: bool):
        """cw_set_option "score_prefill": 0 runs the scoring forward through the per-position decoder step."""
        self._chk(self.lib.cw_set_option(self.ctx, b"score_prefill", 1 if on else 0))

    def test_score_head(self, x, ln_g, ln_b, embed, targets):
        """cw_test_score_head: x [M][D], ln_g / ln_b [D], embed [V][D], targets [M] -> (logprob, top_id, top_logprob) [M]."""
        x = np.ascontiguousarray(x, np.float32)
        embed = np.ascontiguousarray(embed, np.float32)
        g = np.ascontiguousarray(ln_g, np.float32)
        b = np.ascontiguousarray(ln_b, np.float32)
        t = _i32(targets)
        M, D = x.shape
        V = embed.shape[0]
        if embed.shape[1] != D or g.shape != (D,) or b.shape != (D,) or t.shape != (M,):
            raise ValueError("test_score_head: shapes do not agree")
        lp = np.zeros(M, np.float32)
        ti = np.zeros(M, np.int32)
        tl = np.zeros(M, np.float32)
        self._chk(self.lib.cw_test_score_head(self.ctx, M, D, V, _ptr(x), _ptr(g), _ptr(b), _ptr(embed), _ptr(t), _ptr(lp),
                                              _ptr(ti), _ptr(tl)))
        return lp, ti, tl

    def test_score_head_top(self, x, ln_g, ln_b, embed, targets, k: int, want_logits: bool = False, stop=None):
        """cw_test_score_head_top (``stop`` = (eos, timestamp_begin): cw_test_score_head_stop_top): the TOPK form of the head ->
        dict with logprob / top_id / top_logprob [M], alt_id / alt_logprob [M][8] (ranks >= k: -1 / NaN)[, stop_logprob [M]][,
        logits [M][V]: the same operands through the logits-storing form]."""
        x = np.ascontiguousarray(x, np.float32)
        embed = np.ascontiguousarray(embed, np.float32)
        g = np.ascontiguousarray(ln_g, np.float32)
        b = np.ascontiguousarray(ln_b, np.float32)
        t = _i32(targets)
        M, D = x.shape
        V = embed.shape[0]
        if embed.shape[1] != D or g.shape != (D,) or b.shape != (D,) or t.shape != (M,):
            raise ValueError("test_score_head_top: shapes do not agree")
        out = {"logprob": np.zeros(M, np.float32), "top_id": np.zeros(M, np.int32), "top_logprob": np.zeros(M, np.float32),
               "alt_id": np.full((M, 8), -7, np.int32), "alt_logprob": np.full((M, 8), 7.0, np.float32)}
        lg = np.full((M, V), 7.0, np.float32) if want_logits else None
        if stop is None:
            self._chk(self.lib.cw_test_score_head_top(self.ctx, M, D, V, _ptr(x), _ptr(g), _ptr(b), _ptr(embed), _ptr(t), int(k),
                                                      _ptr(out["logprob"]), _ptr(out["top_id"]), _ptr(out["top_logprob"]),
                                                      _ptr(out["alt_id"]), _ptr(out["alt_logprob"]), _ptr(lg) if want_logits else None))
        else:
            out["stop_logprob"] = np.zeros(M, np.float32)
            self._chk(self.lib.cw_test_score_head_stop_top(self.ctx, M, D, V, _ptr(x), _ptr(g), _ptr(b), _ptr(embed), _ptr(t),
                                                           int(stop[0]), int(stop[1]), int(k), _ptr(out["logprob"]),
                                                           _ptr(out["top_id"]), _ptr(out["top_logprob"]), _ptr(out["stop_logprob"]),
                                                           _ptr(out["alt_id"]), _ptr(out["alt_logprob"]),
                                                           _ptr(lg) if want_logits else None))
        if want_logits:
            out["logits"] = lg
        return out

    def test_score_rows_top(self, logits, V: int, targets, k: int, stop=None):
        """cw_test_score_rows_top: the loop path's row kernel (TOPK form) over f32 ``logits`` [rows][ldv], columns 0 .. V-1 ->
        dict as ``test_score_head_top`` (``stop`` = (eos, timestamp_begin): the STOP form, with stop_logprob)."""
        lg = np.ascontiguousarray(logits, np.float32)
        rows, ldv = lg.shape
        t = _i32(targets)
        if t.shape != (rows,):
            raise ValueError("test_score_rows_top: shapes do not agree")
        out = {"logprob": np.zeros(rows, np.float32), "top_id": np.zeros(rows, np.int32), "top_logprob": np.zeros(rows, np.float32),
               "alt_id": np.full((rows, 8), -7, np.int32), "alt_logprob": np.full((rows, 8), 7.0, np.float32)}
        if stop is not None:
            out["stop_logprob"] = np.zeros(rows, np.float32)
        self._chk(self.lib.cw_test_score_rows_top(self.ctx, rows, int(V), ldv, _ptr(lg), _ptr(t), int(k),
                                                  int(stop[0]) if stop is not None else 0, int(stop[1]) if stop is not None else 0,
                                                  _ptr(out["logprob"]), _ptr(out["top_id"]), _ptr(out["top_logprob"]),
                                                  _ptr(out["stop_logprob"]) if stop is not None else None, _ptr(out["alt_id"]),
                                                  _ptr(out["alt_logprob"])))
        return out

    def test_score_head_entropy(self, x, ln_g, ln_b, embed, targets, k: int = 0, want_logits: bool = False, stop=None):
        """cw_test_score_head_entropy: the ENT form of the head, alone or joined with TOPK (``k`` > 0) and / or STOP (``stop`` =
        (eos, timestamp_begin)) -> dict as ``test_score_head_top`` plus entropy [M] (alt_id / alt_logprob only with ``k`` > 0)."""
        x = np.ascontiguousarray(x, np.float32)
        embed = np.ascontiguousarray(embed, np.float32)
        g = np.ascontiguousarray(ln_g, np.float32)
        b = np.ascontiguousarray(ln_b, np.float32)
        t = _i32(targets)
        M, D = x.shape
        V = embed.shape[0]
        if embed.shape[1] != D or g.shape != (D,) or b.shape != (D,) or t.shape != (M,):
            raise ValueError("test_score_head_entropy: shapes do not agree")
        out = {"logprob": np.zeros(M, np.float32), "top_id": np.zeros(M, np.int32), "top_logprob": np.zeros(M, np.float32),
               "entropy": np.full(M, 7.0, np.float32)}
        if int(k) > 0:
            out["alt_id"], out["alt_logprob"] = np.full((M, 8), -7, np.int32), np.full((M, 8), 7.0, np.float32)
        if stop is not None:
            out["stop_logprob"] = np.zeros(M, np.float32)
        lg = np.full((M, V), 7.0, np.float32) if want_logits else None
        self._chk(self.lib.cw_test_score_head_entropy(
            self.ctx, M, D, V, _ptr(x), _ptr(g), _ptr(b), _ptr(embed), _ptr(t), int(stop[0]) if stop is not None else 0,
            int(stop[1]) if stop is not None else 0, int(k), _ptr(out["logprob"]), _ptr(out["top_id"]), _ptr(out["top_logprob"]),
            _ptr(out.get("stop_logprob")), _ptr(out.get("alt_id")), _ptr(out.get("alt_logprob")), _ptr(out["entropy"]), _ptr(lg)))
        if want_logits:
            out["logits"] = lg
        return out

    def test_score_rows_entropy(self, logits, V: int, targets, k: int = 0, stop=None):
        """cw_test_score_rows_entropy: the loop path's row kernel (ENT form, with TOPK when ``k`` > 0 and STOP when ``stop``) over
        f32 ``logits`` [rows][ldv], columns 0 .. V-1 -> dict as ``test_score_rows_top`` plus entropy [rows]."""
        lg = np.ascontiguousarray(logits, np.float32)
        rows, ldv = lg.shape
        t = _i32(targets)
        if t.shape != (rows,):
            raise ValueError("test_score_rows_entropy: shapes do not agree")
        out = {"logprob": np.zeros(rows, np.float32), "top_id": np.zeros(rows, np.int32), "top_logprob": np.zeros(rows, np.float32),
               "entropy": np.full(rows, 7.0, np.float32)}
        if int(k) > 0:
            out["alt_id"], out["alt_logprob"] = np.full((rows, 8), -7, np.int32), np.full((rows, 8), 7.0, np.float32)
        if stop is not None:
            out["stop_logprob"] = np.zeros(rows, np.float32)
        self._chk(self.lib.cw_test_score_rows_entropy(
            self.ctx, rows, int(V), ldv, _ptr(lg), _ptr(t), int(k), int(stop[0]) if stop is not None else 0,
            int(stop[1]) if stop is not None else 0, _ptr(out["logprob"]), _ptr(out["top_id"]), _ptr(out["top_logprob"]),
            _ptr(out.get("stop_logprob")), _ptr(out.get("alt_id")), _ptr(out.get("alt_logprob")), _ptr(out["entropy"])))
        return out

    def time_score_head_entropy(self, M: int, k: int = 0, stop: bool = False, iters: int = 10) -> float:
        """cw_time_score_head_entropy: ``time_score_head_top`` with the ENT form on."""
        ms = C.c_float(0.0)
        self._chk(self.lib.cw_time_score_head_entropy(self.ctx, int(M), int(k), 1 if stop else 0, int(iters), C.byref(ms)))
        return float(ms.value)

    def time_score_head_top(self, M: int, k: int, stop: bool = False, iters: int = 10) -> float:
        """cw_time_score_head_top: ms per run of the fused head (``stop``: its STOP form) with k alternatives per row (0: none)."""
        ms = C.c_float(0.0)
        self._chk(self.lib.cw_time_score_head_top(self.ctx, int(M), int(k), 1 if stop else 0, int(iters), C.byref(ms)))
        return float(ms.value)

    def time_score_head(self, M: int, unfused: bool = False, iters: int = 10, stop: bool = False) -> float:
        """cw_time_score_head: ms per run of the scoring head over M rows at this engine's geometry (fused, or the unfused form
        that stores f32 logits and reduces them row by row; ``stop``: the fused STOP form of ``align_cut_tokens``)."""
        ms = C.c_float(0.0)
        self._chk(self.lib.cw_time_score_head(self.ctx, int(M), 2 if stop else (1 if unfused else 0), int(iters), C.byref(ms)))
        return float(ms.value)

    # ------------------------------------------------------------------ beam search (device half; host half: generation.beam_search)
    def beam_begin(self, prompt: np.ndarray, num_beams: int, max_length: int, min_new_tokens: int = 0):
        prompt = _i32(prompt)
        n_items, n_prompt = prompt.shape
        self._beam_rows = n_items * int(num_beams)
        self._chk(self.lib.cw_beam_begin(self.ctx, n_items, int(num_beams), _ptr(prompt), n_prompt, int(max_length),
                                         int(min_new_tokens)))

    def beam_step(self, n_cand: int):
        """-> (log-probabilities [rows, n_cand] float32 best first, tokens [rows, n_cand] int32; -inf / -1 padded)."""
        vals = np.empty((self._beam_rows, n_cand), dtype=np.float32)
        toks = np.empty((self._beam_rows, n_cand), dtype=np.int32)
        self._chk(self.lib.cw_beam_step(self.ctx, int(n_cand), _ptr(vals), _ptr(toks)))
        return vals, toks

    def beam_advance(self, parent, token):
        parent, token = _i32(parent), _i32(token)
        self._chk(self.lib.cw_beam_advance(self.ctx, _ptr(parent), _ptr(token)))

    def beam_finish(self, row_of_pos: np.ndarray):
        r = _i32(row_of_pos)
        self._chk(self.lib.cw_beam_finish(self.ctx, r.shape[0], r.shape[1], _ptr(r)))

    def token_timestamps(self, nb: int, L: int, n_prompt: int, num_frames) -> np.ndarray:
        nf = _i32(num_frames)
        out = np.zeros((nb, L + 1), dtype=np.float32)
        self._chk(self.lib.cw_token_timestamps(self.ctx, nb, L, n_prompt, _ptr(nf), _ptr(out)))
        return out

    # ------------------------------------------------------------------ stand-alone kernels
    def align_matrix(self, attn: np.ndarray, n_cols, width: int) -> np.ndarray:
        a = np.ascontiguousarray(attn, dtype=np.float32)
        B, Ha, Nn, M = a.shape
        nc = _i32(n_cols)
        out = np.zeros((B, Nn, M), dtype=np.float32)
        self._chk(self.lib.cw_align_matrix(self.ctx, _ptr(a), B, Ha, Nn, M, _ptr(nc), width, _ptr(out)))
        return out

    def dtw(self, mat: np.ndarray):
        m = np.ascontiguousarray(mat, dtype=np.float32)
        Nn, M = m.shape
        ti = np.zeros(Nn + M + 2, dtype=np.int32)
        tj = np.zeros(Nn + M + 2, dtype=np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.cw_dtw(self.ctx, _ptr(m), Nn, M, _ptr(ti), _ptr(tj), C.byref(n)))
        return ti[:n.value].copy(), tj[:n.value].copy()

    def adjust_pauses(self, start: np.ndarray, end: np.ndarray, thr: float):
        s = np.ascontiguousarray(start, dtype=np.float64).copy()
        e = np.ascontiguousarray(end, dtype=np.float64).copy()
        self._chk(self.lib.cw_adjust_pauses(self.ctx, _ptr(s), _ptr(e), len(s), float(thr)))
        return s, e

    def test_gemm(self, A, W, bias=None, gelu=False):
        A = np.ascontiguousarray(A, np.float32); W = np.ascontiguousarray(W, np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        out = np.zeros((A.shape[0], W.shape[0]), np.float32)
        self._chk(self.lib.cw_test_gemm(self.ctx, A.shape[0], W.shape[0], A.shape[1], _ptr(A), _ptr(W), _ptr(b), int(gelu), _ptr(out)))
        return out

    def test_gemm_fp8(self, A, W, bias=None, gelu=False):
        """A W^T (+ bias, optional GELU) through the e4m3 GEMM of the opt-in fp8 encoder mode (row-wise scales of both operands)."""
        A = np.ascontiguousarray(A, np.float32); W = np.ascontiguousarray(W, np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        out = np.zeros((A.shape[0], W.shape[0]), np.float32)
        self._chk(self.lib.cw_test_gemm_fp8(self.ctx, A.shape[0], W.shape[0], A.shape[1], _ptr(A), _ptr(W), _ptr(b), int(gelu), _ptr(out)))
        return out

    def test_gemm_epi(self, epi, A, W, bias=None, *, out, out1=None, out2=None, conv=None, resid=None, pos=None, ldo=0, T=0,
                      S_pad=0, H=0, d_model=0, fp8=False, M=None, K=None):
        """One launch of the encoder GEMM dispatcher with epilogue `epi` (cw_test_gemm_epi).  A [M][K], or with
        conv = (T_out, stride, row_off, row_valid) the time-major input rows [n_rows][C_in] of the implicit conv1d gather;
        W [N][K].  out (head split: out, out1, out2) are float32 arrays holding the caller's sentinel; they are overwritten in
        place with what the device holds after the launch and `out` is returned.  M / K override the operand's own shape (the
        refusal tests)."""
        A = np.ascontiguousarray(A, np.float32); W = np.ascontiguousarray(W, np.float32)
        keep = [A, W]
        a = N.GemmEpiArgs()
        a.epi, a.fp8, a.N = int(epi), int(bool(fp8)), W.shape[0]
        if conv is None:
            a.conv, a.M, a.K = 0, A.shape[0], A.shape[1]
        else:
            T_out, stride, row_off, row_valid = conv
            ro, rv = _i32(row_off), _i32(row_valid)
            keep += [ro, rv]
            a.conv, a.n_rows, a.C_in, a.T_out, a.stride, a.nb = 1, A.shape[0], A.shape[1], int(T_out), int(stride), len(ro)
            a.row_off, a.row_valid = _ptr(ro), _ptr(rv)
            a.M, a.K = len(ro) * int(T_out), 3 * A.shape[1]
        if M is not None:
            a.M = int(M)
        if K is not None:
            a.K = int(K)
        a.A, a.W = _ptr(A), _ptr(W)
        for name, t in (("bias", bias), ("resid", resid), ("pos", pos)):
            if t is not None:
                t = np.ascontiguousarray(t, np.float32)
                keep.append(t)
                setattr(a, name, _ptr(t))
        a.ldo, a.T, a.S_pad, a.H, a.d_model = int(ldo), int(T), int(S_pad), int(H), int(d_model)
        for name, t in (("out", out), ("out1", out1), ("out2", out2)):
            if t is not None:
                assert t.dtype == np.float32 and t.flags["C_CONTIGUOUS"] and t.flags["WRITEABLE"]
                setattr(a, name, _ptr(t))
        self._chk(self.lib.cw_test_gemm_epi(self.ctx, C.byref(a)))
        return out

    def test_rownorm(self, mode, x, gamma=None, beta=None, *, out=None, out8=None, scale=None):
        """One launch of a row kernel (cw_test_rownorm): mode 0 LayerNorm -> out [rows][d] float32; mode 1 LayerNorm -> e4m3
        bytes out8 [rows][d] (uint8) + scale [rows]; mode 2 row-wise e4m3 quantisation of x rounded to the 16-bit type.  The
        output arrays are in / out (sentinel in, device contents out); missing ones are created zero-filled.  Returns out, or
        (out8, scale)."""
        x = np.ascontiguousarray(x, np.float32)
        rows, d = x.shape
        g = None if gamma is None else np.ascontiguousarray(gamma, np.float32)
        b = None if beta is None else np.ascontiguousarray(beta, np.float32)
        if mode == 0:
            out = np.zeros((rows, d), np.float32) if out is None else out
            assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        else:
            out8 = np.zeros((rows, d), np.uint8) if out8 is None else out8
            scale = np.zeros(rows, np.float32) if scale is None else scale
            assert out8.dtype == np.uint8 and scale.dtype == np.float32 and out8.flags["C_CONTIGUOUS"]
        self._chk(self.lib.cw_test_rownorm(self.ctx, int(mode), rows, d, _ptr(x), _ptr(g), _ptr(b), _ptr(out), _ptr(out8), _ptr(scale)))
        return out if mode == 0 else (out8, scale)

    def test_mel_stages(self, B: int):
        """The mel stage's buffers after mel / mel_resident over B items (cw_test_mel_stages; copies only): logspec [B][3000]
        [n_mels] (log10 before the clip floor), gmax [B] (the decoded clip maximum) and feats_tm [B][3000][n_mels] (the time-major
        features conv1 reads, engine type -> float32)."""
        B = int(B)
        raw = np.empty((B, N.N_FRAMES, self.spec.n_mels), np.float32)
        gmax = np.empty(B, np.float32)
        tm = np.empty((B, N.N_FRAMES, self.spec.n_mels), np.float32)
        self._chk(self.lib.cw_test_mel_stages(self.ctx, B, _ptr(raw), _ptr(gmax), _ptr(tm)))
        return raw, gmax, tm

    def test_gemv(self, x, W, bias=None, ln=None, gelu=False):
        x = np.ascontiguousarray(x, np.float32); W = np.ascontiguousarray(W, np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        g = be = None
        if ln is not None:
            g, be = (np.ascontiguousarray(t, np.float32) for t in ln)
        out = np.zeros((x.shape[0], W.shape[0]), np.float32)
        self._chk(self.lib.cw_test_gemv(self.ctx, x.shape[0], W.shape[0], x.shape[1], _ptr(x), _ptr(W), _ptr(b),
                                        _ptr(g), _ptr(be), int(gelu), _ptr(out)))
        return out

    def test_skinny(self, mode, x, W, bias=None, out0=None, nks=0, reps=0):
        """One skinny-M decoder projection (cw_test_skinny, 17..64 rows).  mode 0: LayerNorm (no affine) + projection, 1: + GELU
        (16-bit result), 2: out0 + x16 W^T + bias on the residual grid.  Returns (out, (gemm_us, finish_us))."""
        x = np.ascontiguousarray(x, np.float32); W = np.ascontiguousarray(W, np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        out = np.zeros((x.shape[0], W.shape[0]), np.float32) if out0 is None else np.ascontiguousarray(out0, np.float32).copy()
        us = np.zeros(2, np.float32)
        self._chk(self.lib.cw_test_skinny(self.ctx, int(mode), x.shape[0], W.shape[0], x.shape[1], _ptr(x), _ptr(W), _ptr(b),
                                          int(nks), int(reps), _ptr(out), _ptr(us)))
        return out, (float(us[0]), float(us[1]))

    def test_attention(self, q, k, v, out0=None):
        """cw_test_attention: q / k / v [B][H][S][64] -> [B][S][H*64].  out0: what the output buffer holds before the launch (a
        sentinel shows every element the kernel did not write); zeros when omitted."""
        q, k, v = (np.ascontiguousarray(t, np.float32) for t in (q, k, v))
        B, H, S, _ = q.shape
        out = np.zeros((B, S, H * 64), np.float32) if out0 is None else np.ascontiguousarray(out0, np.float32).copy()
        assert out.shape == (B, S, H * 64), out.shape
        self._chk(self.lib.cw_test_attention(self.ctx, B, H, S, _ptr(q), _ptr(k), _ptr(v), _ptr(out)))
        return out

    def set_prompt_prefix(self, n: int):
        """cw_set_option "prompt_prefix": the coming decode / beam_begin inputs start with n prompt_ids (0: none) -- what lets
        the prefill engage; cw_transcribe_prompted sets it itself."""
        self._chk(self.lib.cw_set_option(self.ctx, b"prompt_prefix", int(n)))

    def set_prompt_prefill(self, on: bool):
        """cw_set_option "prompt_prefill": 0 runs the prompt positions of a prompt_ids call through the per-position step."""
        self._chk(self.lib.cw_set_option(self.ctx, b"prompt_prefill", 1 if on else 0))

    def test_prefill_gemm(self, mode, A, W, bias=None, resid=None):
        """cw_test_prefill_gemm: mode 0 store / 2 residual (returns resid + A W^T + bias) / 3 GELU, W [N][K] packed on device."""
        A, W = (np.ascontiguousarray(t, np.float32) for t in (A, W))
        M, K = A.shape
        N = W.shape[0]
        out = (np.ascontiguousarray(resid, np.float32).copy() if resid is not None else np.zeros((M, N), np.float32))
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        self._chk(self.lib.cw_test_prefill_gemm(self.ctx, int(mode), M, N, K, _ptr(A), _ptr(W), _ptr(b), _ptr(out)))
        return out

    def test_prefill_attention(self, q, k, v, n_keys, causal, kv_div=1):
        """cw_test_prefill_attention: q [rows][n_q][H*64], k / v [rows / kv_div][H][cap][64] -> [rows][n_q][H*64]."""
        q, k, v = (np.ascontiguousarray(t, np.float32) for t in (q, k, v))
        rows, n_q, D = q.shape
        H, cap = k.shape[1], k.shape[2]
        out = np.zeros_like(q)
        self._chk(self.lib.cw_test_prefill_attention(self.ctx, rows, n_q, H, cap, int(n_keys), 1 if causal else 0, int(kv_div),
                                                     _ptr(q), _ptr(k), _ptr(v), _ptr(out)))
        return out

    def test_prefill_align_attention(self, q, k, v, kv_div=1, align_head=0):
        """cw_test_prefill_align_attention: q [rows][n_q][H*64], k / v [rows / kv_div][H][n_keys][64] -> (out [rows][n_q][H*64],
        align [rows][n_q][n_keys]: head align_head's recorded rows, normalised)."""
        q, k, v = (np.ascontiguousarray(t, np.float32) for t in (q, k, v))
        rows, n_q, _ = q.shape
        H, n_keys = k.shape[1], k.shape[2]
        out = np.zeros_like(q)
        align = np.zeros((rows, n_q, n_keys), np.float32)
        self._chk(self.lib.cw_test_prefill_align_attention(self.ctx, rows, n_q, H, n_keys, int(kv_div), int(align_head),
                                                           _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(align)))
        return out, align

    def test_cross_attention(self, q, k, v, kv_div=1, align_head=0):
        """One launch of the key-split cross-attention decode kernel (cw_test_cross_attention): q [B][H][64] pre-scaled,
        k / v [B / kv_div][H][S][64].  Returns (out [B][H*64], align [B][S]) with the six splits combined on the host."""
        q, k, v = (np.ascontiguousarray(t, np.float32) for t in (q, k, v))
        B, H, _ = q.shape
        S = k.shape[2]
        NS = 6
        po = np.zeros((NS, B, H * 64), np.float32); ml = np.zeros((B, H, NS, 2), np.float32)
        al = np.zeros((B, S), np.float32); aml = np.zeros((B, NS, 2), np.float32)
        self._chk(self.lib.cw_test_cross_attention(self.ctx, B, H, S, int(kv_div), _ptr(q), _ptr(k), _ptr(v), int(align_head),
                                                   _ptr(po), _ptr(ml), _ptr(al), _ptr(aml)))
        m = ml[..., 0].astype(np.float64); l = ml[..., 1].astype(np.float64)
        M = m.max(-1, keepdims=True)
        w = np.exp(m - M)                                            # [B][H][NS]
        o = (po.astype(np.float64).reshape(NS, B, H, 64) * w.transpose(2, 0, 1)[..., None]).sum(0) / (l * w).sum(-1)[..., None]
        per = (S + NS - 1) // NS
        am = aml[..., 0].astype(np.float64); a_l = aml[..., 1].astype(np.float64)
        AM = am.max(-1, keepdims=True); aw = np.exp(am - AM)
        scale = np.repeat(aw, per, axis=1)[:, :S] / (a_l * aw).sum(-1, keepdims=True)
        return o.reshape(B, H * 64), al.astype(np.float64) * scale

    def test_cross_attention_raw(self, q, k, v, kv_div=1, align_head=0):
        """cw_test_cross_attention without the host combine: q [B][H*64] -> (part_o [6][B][H*64], part_ml [B][H][6][2])."""
        q, k, v = (np.ascontiguousarray(t, np.float32) for t in (q, k, v))
        B, H, S, NS = q.shape[0], k.shape[1], k.shape[2], 6
        po = np.zeros((NS, B, H * 64), np.float32); ml = np.zeros((B, H, NS, 2), np.float32)
        al = np.zeros((B, S), np.float32); aml = np.zeros((B, NS, 2), np.float32)
        self._chk(self.lib.cw_test_cross_attention(self.ctx, B, H, S, int(kv_div), _ptr(q), _ptr(k), _ptr(v), int(align_head),
                                                   _ptr(po), _ptr(ml), _ptr(al), _ptr(aml)))
        return po, ml

    def test_cross_attention_fused(self, qa, qb, qw, qbias, pstats, k, v, kv_div=1, align_head=0, n_pstats=None, fill=0.0):
        """cw_test_cross_attention_fused: qa / qb [B][H*64], qw / qbias [H*64], pstats [ceil(B/16)][n_pstats][16][2], k / v
        [B / kv_div][H][S][64] -> (part_o [6][B][H*64], part_ml [B][H][6][2]), which hold `fill` before the launch."""
        qa, qb, qw, qbias, pstats, k, v = (np.ascontiguousarray(t, np.float32) for t in (qa, qb, qw, qbias, pstats, k, v))
        B, H, S, NS = qa.shape[0], k.shape[1], k.shape[2], 6
        n_pstats = pstats.shape[1] if n_pstats is None else int(n_pstats)
        assert qa.shape == qb.shape == (B, H * 64) and qw.shape == qbias.shape == (H * 64,)
        assert pstats.size == ((B + 15) // 16) * n_pstats * 32 or n_pstats < 1 or n_pstats > 128, pstats.shape
        po = np.full((NS, B, H * 64), fill, np.float32); ml = np.full((B, H, NS, 2), fill, np.float32)
        al = np.zeros((B, S), np.float32); aml = np.zeros((B, NS, 2), np.float32)
        self._chk(self.lib.cw_test_cross_attention_fused(self.ctx, B, H, S, int(kv_div), _ptr(qa), _ptr(qb), _ptr(qw), _ptr(qbias),
                                                         _ptr(pstats), n_pstats, _ptr(k), _ptr(v), int(align_head), _ptr(po),
                                                         _ptr(ml), _ptr(al), _ptr(aml)))
        return po, ml

    def test_fold(self, op, *, n, j=0, k=0, scale=1.0, a=None, s=None, v=None, w16=None, out16=None, c_out=None, w_out=None,
                  image=None):
        """One load-time rewrite (cw_test_fold; op 0 fold_layernorm, 1 fold_product, 2 fold_rowvec, 3 wfrag_pack).  The inputs
        a / s / v / w16 are float32 arrays (or None); out16 / c_out / w_out (float32) and image (uint16) are in / out: they are
        overwritten in place with what the device holds after the launch."""
        keep = []
        args = N.FoldArgs()
        args.op, args.N, args.J, args.K, args.scale = int(op), int(n), int(j), int(k), float(scale)
        for name, t in (("a", a), ("s", s), ("v", v), ("w16", w16)):
            if t is not None:
                t = np.ascontiguousarray(t, np.float32)
                keep.append(t)
                setattr(args, name, _ptr(t))
        for name, t, dt in (("out16", out16, np.float32), ("c_out", c_out, np.float32), ("w_out", w_out, np.float32),
                            ("image", image, np.uint16)):
            if t is not None:
                assert t.dtype == dt and t.flags["C_CONTIGUOUS"] and t.flags["WRITEABLE"], name
                setattr(args, name, _ptr(t))
        self._chk(self.lib.cw_test_fold(self.ctx, C.byref(args)))

    def test_gemv_stack(self, W, segs, *, Mb, K, nt=0, wpk=False, zero=None):
        """One cw_launch_gemv_stack call (cw_test_gemv_stack).  W [sum n_tiles * 16][K]; segs: up to three dicts with x [Mb][K],
        n_tiles, epi, optional bias / wsum / resid / nt, and the in / out float32 arrays out, out2, pstats ([groups][blocks][16][2];
        its second dimension is passed on as the caller's block count), which are overwritten in place; `zero` likewise (a float32
        array of a multiple of four elements)."""
        W = np.ascontiguousarray(W, np.float32)
        keep = [W]
        a = N.GemvStackArgs()
        a.Mb, a.K, a.nt, a.wpk, a.nseg, a.W = int(Mb), int(K), int(nt), int(bool(wpk)), len(segs), _ptr(W)
        assert len(segs) <= 3
        for i, sg in enumerate(segs):
            q = a.seg[i]
            for name in ("x", "bias", "wsum", "resid"):
                t = sg.get(name)
                if t is not None:
                    t = np.ascontiguousarray(t, np.float32)
                    keep.append(t)
                    setattr(q, name, _ptr(t))
            q.n_tiles, q.nt, q.epi = int(sg["n_tiles"]), int(sg.get("nt", 0)), int(sg["epi"])
            for name in ("out", "out2", "pstats"):
                t = sg.get(name)
                if t is not None:
                    assert t.dtype == np.float32 and t.flags["C_CONTIGUOUS"] and t.flags["WRITEABLE"], name
                    setattr(q, name, _ptr(t))
            if sg.get("pstats") is not None:
                q.pstats_blocks = int(sg.get("pstats_blocks", sg["pstats"].shape[1]))
        if zero is not None:
            assert zero.dtype == np.float32 and zero.flags["C_CONTIGUOUS"] and zero.size % 4 == 0
            a.zero, a.zero_n4 = _ptr(zero), zero.size // 4
        self._chk(self.lib.cw_test_gemv_stack(self.ctx, C.byref(a)))

    def test_gemv_epi(self, *, op=0, epi=0, Mb, N, K, W=None, ldo=None, wpk=False, x16=False, inplace=False, frag_in=False, H=0, cap=0,
                      d_model=0, x=None, bias=None, ln_g=None, ln_b=None, resid=None, part_o=None, part_ml=None, pstats=None,
                      n_pstats=0, pos=None, cvec_in=None, stats_in=None, n_stats=0, wsum=None, out=None, sk=None, sv=None, y=None,
                      stats=None, cvec=None):
        """One call of a launcher of the decode GEMV dispatcher (cw_test_gemv_epi; include/crisperwhisper.h describes the forms).
        The in / out float32 arrays out, sk, sv, y, stats and cvec are overwritten in place.  Returns {"nt", "frag_tail_ok"}."""
        a = _GemvEpiArgs()
        keep = []
        a.op, a.epi, a.Mb, a.N, a.K = int(op), int(epi), int(Mb), int(N), int(K)
        a.ldo = int(N if ldo is None else ldo)
        a.wpk, a.x16, a.inplace, a.frag_in = int(bool(wpk)), int(bool(x16)), int(bool(inplace)), int(bool(frag_in))
        a.H, a.cap, a.d_model, a.n_pstats, a.n_stats = int(H), int(cap), int(d_model), int(n_pstats), int(n_stats)
        for name, t in (("x", x), ("W", W), ("bias", bias), ("ln_g", ln_g), ("ln_b", ln_b), ("resid", resid), ("part_o", part_o),
                        ("part_ml", part_ml), ("pstats", pstats), ("cvec_in", cvec_in), ("stats_in", stats_in), ("wsum", wsum)):
            if t is not None:
                t = np.ascontiguousarray(t, np.float32)
                keep.append(t)
                setattr(a, name, _ptr(t))
        if pos is not None:
            pos = _i32(pos)
            a.pos = _ptr(pos)
        for name, t in (("out", out), ("sk", sk), ("sv", sv), ("y", y), ("stats", stats), ("cvec", cvec)):
            if t is not None:
                assert t.dtype == np.float32 and t.flags["C_CONTIGUOUS"] and t.flags["WRITEABLE"], name
                setattr(a, name, _ptr(t))
        nt, tail = np.zeros(1, np.int32), np.zeros(1, np.int32)
        a.nt, a.frag_tail_ok = _ptr(nt), _ptr(tail)
        self._chk(self.lib.cw_test_gemv_epi(self.ctx, C.byref(a)))
        return {"nt": int(nt[0]), "frag_tail_ok": bool(tail[0])}

    def test_self_attention(self, q, k, v, pos, n_keys=0, anc=None, kv_div=1, short_hist=False, out_frag=False,
                            align_head=-1, align_rows=0, align_init=None):
        """One launch of the decode self-attention dispatcher (cw_test_self_attention): q [B][H*64] pre-scaled, k / v
        [B / kv_div][H][cap][64], pos [B]; n_keys = 0: pos[b] + 1 keys per row, else that many (pos[b] = alignment row);
        anc [B][cap] or None.  Returns out [B][H*64]; with out_frag also whether the fragment buffer's padding rows stayed
        untouched; with align_head >= 0 also align [B][align_rows][n_keys] (starting from align_init, default zeros)."""
        q, k, v = (np.ascontiguousarray(t, np.float32) for t in (q, k, v))
        B = q.shape[0]
        H, cap = k.shape[1], k.shape[2]
        pos = _i32(pos)
        a = None if anc is None else _i32(anc)
        out = np.zeros((B, H * 64), np.float32)
        al = None
        if align_head >= 0:
            al = (np.zeros((B, align_rows, n_keys), np.float32) if align_init is None
                  else np.ascontiguousarray(align_init, np.float32).copy())
        tail = np.zeros(1, np.int32)
        self._chk(self.lib.cw_test_self_attention(self.ctx, B, H, cap, int(kv_div), _ptr(q), _ptr(k), _ptr(v), _ptr(pos),
                                                  int(n_keys), _ptr(a), 1 if short_hist else 0, 1 if out_frag else 0,
                                                  int(align_head), int(align_rows), _ptr(out), _ptr(al), _ptr(tail)))
        res = (out,)
        if out_frag:
            res += (bool(tail[0]),)
        if align_head >= 0:
            res += (al,)
        return res[0] if len(res) == 1 else res

    def test_beam_state(self, rows: int):
        """(ids, anc, pos) of the first `rows` beam rows as the device holds them (cw_test_beam_state)."""
        tgt = self.spec.max_target_positions
        ids = np.zeros((rows, tgt), np.int32); anc = np.zeros((rows, tgt), np.int32); pos = np.zeros(rows, np.int32)
        self._chk(self.lib.cw_test_beam_state(self.ctx, int(rows), _ptr(ids), _ptr(anc), _ptr(pos)))
        return ids, anc, pos

    def test_beam_topk(self, logits: np.ndarray, ids: np.ndarray, n_prompt: int, n_cand: int, min_new_tokens: int = 0):
        """One launch of the beam-search candidate selection on caller rows (cw_test_beam_topk): returns (values [nb][n_cand] f32,
        tokens [nb][n_cand] int32, untouched) where ``untouched`` says that everything behind the nb * n_cand written entries of
        the device's candidate buffers still holds the 0xff bytes the hook put there."""
        lg = np.ascontiguousarray(logits, np.float32)
        ids = _i32(ids)
        if ids.ndim != 2 or lg.shape != (ids.shape[0], self.spec.vocab_size):
            raise ValueError(f"logits must be [nb][{self.spec.vocab_size}] and ids [nb][t], got {lg.shape} and {ids.shape}")
        nb, t = ids.shape
        val = np.zeros(self.max_batch * 64, np.float32)
        tok = np.zeros(self.max_batch * 64, np.int32)
        self._chk(self.lib.cw_test_beam_topk(self.ctx, nb, _ptr(lg), _ptr(ids), t, int(n_prompt), int(min_new_tokens), int(n_cand),
                                             _ptr(val), _ptr(tok)))
        n = nb * int(n_cand)
        untouched = bool(np.all(val[n:].view(np.uint32) == 0xffffffff) and np.all(tok[n:] == -1))
        return val[:n].reshape(nb, n_cand).copy(), tok[:n].reshape(nb, n_cand).copy(), untouched

    def test_beam_x(self, rows: int) -> np.ndarray:
        """The decoder input rows of the next step as the device holds them, [rows][d_model] (cw_test_beam_x)."""
        x = np.zeros((int(rows), self.spec.d_model), np.float32)
        self._chk(self.lib.cw_test_beam_x(self.ctx, int(rows), _ptr(x)))
        return x

    def test_decode_state(self, what: str, rows: int, layer: int = 0, n_pos: int = 1) -> np.ndarray:
        """What the last decoder forward left on the device (cw_test_decode_state): ``"qa"`` the cross-query x term of the last
        layer, [rows][d_model] f32; ``"k"`` / ``"v"`` the first n_pos self-attention cache rows of a layer, raw element bits;
        ``"xq_plan"``: [1] int32, whether ``rows`` rows take the x term in the q/k/v launch."""
        code = {"qa": 0, "k": 1, "v": 2, "xq_plan": 3}[what]
        if code == 3:
            out = np.zeros(1, np.int32)
        elif code == 0:
            out = np.zeros((int(rows), self.spec.d_model), np.float32)
        else:
            out = np.zeros((int(rows), self.spec.n_heads, int(n_pos), 64), np.float32 if self.dtype == "f32" else np.uint16)
        self._chk(self.lib.cw_test_decode_state(self.ctx, code, int(layer), int(rows), int(n_pos), _ptr(out)))
        return out

    def test_sample(self, logits: np.ndarray, ids: np.ndarray, n_prompt: int, min_new_tokens: int = 0,
                    max_length: Optional[int] = None) -> np.ndarray:
        """One launch of the fused logits processors + greedy choice on caller rows (cw_test_sample)."""
        lg = np.ascontiguousarray(logits, np.float32)
        ids = _i32(ids)
        nb, t = ids.shape
        out = np.zeros(nb, np.int32)
        self._chk(self.lib.cw_test_sample(self.ctx, nb, _ptr(lg), _ptr(ids), t, int(n_prompt), int(min_new_tokens),
                                          int(max_length or self.spec.max_target_positions), _ptr(out)))
        return out

    def test_sample_seeded(self, logits: np.ndarray, ids: np.ndarray, n_prompt: int, temperature: float, seed: int,
                           row_streams, min_new_tokens: int = 0, max_length: Optional[int] = None) -> np.ndarray:
        """The same two launches under a sampling setting of their own (cw_test_sample_seeded)."""
        lg = np.ascontiguousarray(logits, np.float32)
        ids = _i32(ids)
        nb, t = ids.shape
        if lg.shape != (nb, self.spec.vocab_size):
            raise ValueError(f"logits must be [{nb}][{self.spec.vocab_size}], got {lg.shape}")
        rs = None if row_streams is None else np.ascontiguousarray(row_streams, dtype=np.uint64)
        if rs is not None and rs.shape != (nb,):
            raise ValueError(f"row_streams must hold one id per row ({nb}), got shape {rs.shape}")
        out = np.zeros(nb, np.int32)
        self._chk(self.lib.cw_test_sample_seeded(self.ctx, nb, _ptr(lg), _ptr(ids), t, int(n_prompt), int(min_new_tokens),
                                                 int(max_length or self.spec.max_target_positions), float(temperature),
                                                 int(seed) & (2 ** 64 - 1), _ptr(rs), _ptr(out)))
        return out

    def test_sample_logprobs(self, logits: np.ndarray, ids: np.ndarray, n_prompt: int, temperature: float = 0.0, seed: int = 0,
                             row_streams=None, forced=None, min_new_tokens: int = 0, max_length: Optional[int] = None):
        """``test_sample_seeded`` with the per-token log-probability store on (cw_test_sample_logprobs): returns (choice [nb],
        logprob [nb] of the token written at index t).  ``forced`` [nb] (-1: not forced) is written instead of the choice."""
        lg = np.ascontiguousarray(logits, np.float32)
        ids = _i32(ids)
        nb, t = ids.shape
        if lg.shape != (nb, self.spec.vocab_size):
            raise ValueError(f"logits must be [{nb}][{self.spec.vocab_size}], got {lg.shape}")
        rs = None if row_streams is None else np.ascontiguousarray(row_streams, dtype=np.uint64)
        if rs is not None and rs.shape != (nb,):
            raise ValueError(f"row_streams must hold one id per row ({nb}), got shape {rs.shape}")
        fr = None if forced is None else _i32(forced)
        if fr is not None and fr.shape != (nb,):
            raise ValueError(f"forced must hold one token per row ({nb}), got shape {fr.shape}")
        out = np.zeros(nb, np.int32)
        lp = np.zeros(nb, np.float32)
        self._chk(self.lib.cw_test_sample_logprobs(self.ctx, nb, _ptr(lg), _ptr(ids), t, int(n_prompt), int(min_new_tokens),
                                                   int(max_length or self.spec.max_target_positions), float(temperature),
                                                   int(seed) & (2 ** 64 - 1), _ptr(rs), _ptr(fr), _ptr(out), _ptr(lp)))
        return out, lp

    def test_sample_top_logprobs(self, logits: np.ndarray, ids: np.ndarray, n_prompt: int, k: int, temperature: float = 0.0,
                                 seed: int = 0, row_streams=None, forced=None, min_new_tokens: int = 0,
                                 max_length: Optional[int] = None):
        """``test_sample_logprobs`` with ``set_top_logprobs(k)`` on for the call (cw_test_sample_top_logprobs): returns (choice
        [nb], logprob [nb], top ids [nb][k], top logprobs [nb][k]) of index t."""
        lg = np.ascontiguousarray(logits, np.float32)
        ids = _i32(ids)
        nb, t = ids.shape
        if lg.shape != (nb, self.spec.vocab_size):
            raise ValueError(f"logits must be [{nb}][{self.spec.vocab_size}], got {lg.shape}")
        if not 1 <= int(k) <= 8:
            raise ValueError(f"k must be in 1 .. 8, got {k}")
        rs = None if row_streams is None else np.ascontiguousarray(row_streams, dtype=np.uint64)
        if rs is not None and rs.shape != (nb,):
            raise ValueError(f"row_streams must hold one id per row ({nb}), got shape {rs.shape}")
        fr = None if forced is None else _i32(forced)
        if fr is not None and fr.shape != (nb,):
            raise ValueError(f"forced must hold one token per row ({nb}), got shape {fr.shape}")
        out = np.zeros(nb, np.int32)
        lp = np.zeros(nb, np.float32)
        top_id = np.zeros((nb, int(k)), np.int32)
        top_lp = np.zeros((nb, int(k)), np.float32)
        self._chk(self.lib.cw_test_sample_top_logprobs(self.ctx, nb, _ptr(lg), _ptr(ids), t, int(n_prompt), int(min_new_tokens),
                                                       int(max_length or self.spec.max_target_positions), float(temperature),
                                                       int(seed) & (2 ** 64 - 1), _ptr(rs), _ptr(fr), int(k), _ptr(out), _ptr(lp),
                                                       _ptr(top_id), _ptr(top_lp)))
        return out, lp, top_id, top_lp

    def test_sample_entropy(self, logits: np.ndarray, ids: np.ndarray, n_prompt: int, k: int = 0, temperature: float = 0.0,
                            seed: int = 0, row_streams=None, forced=None, min_new_tokens: int = 0,
                            max_length: Optional[int] = None):
        """``test_sample_logprobs`` with ``set_token_entropy(True)`` on for the call (cw_test_sample_entropy): returns (choice
        [nb], logprob [nb], entropy [nb]) of index t, and with ``k`` > 0 also (top ids [nb][k], top logprobs [nb][k])."""
        lg = np.ascontiguousarray(logits, np.float32)
        ids = _i32(ids)
        nb, t = ids.shape
        if lg.shape != (nb, self.spec.vocab_size):
            raise ValueError(f"logits must be [{nb}][{self.spec.vocab_size}], got {lg.shape}")
        if not 0 <= int(k) <= 8:
            raise ValueError(f"k must be in 0 .. 8, got {k}")
        rs = None if row_streams is None else np.ascontiguousarray(row_streams, dtype=np.uint64)
        if rs is not None and rs.shape != (nb,):
            raise ValueError(f"row_streams must hold one id per row ({nb}), got shape {rs.shape}")
        fr = None if forced is None else _i32(forced)
        if fr is not None and fr.shape != (nb,):
            raise ValueError(f"forced must hold one token per row ({nb}), got shape {fr.shape}")
        out = np.zeros(nb, np.int32)
        lp = np.zeros(nb, np.float32)
        ent = np.zeros(nb, np.float32)
        top_id = np.zeros((nb, max(1, int(k))), np.int32)
        top_lp = np.zeros((nb, max(1, int(k))), np.float32)
        self._chk(self.lib.cw_test_sample_entropy(self.ctx, nb, _ptr(lg), _ptr(ids), t, int(n_prompt), int(min_new_tokens),
                                                  int(max_length or self.spec.max_target_positions), float(temperature),
                                                  int(seed) & (2 ** 64 - 1), _ptr(rs), _ptr(fr), int(k), _ptr(out), _ptr(lp),
                                                  _ptr(ent), _ptr(top_id), _ptr(top_lp)))
        return (out, lp, ent, top_id, top_lp) if int(k) > 0 else (out, lp, ent)

    def test_sample_biased(self, logits: np.ndarray, ids: np.ndarray, n_prompt: int, k: int, table=None, temperature: float = 0.0,
                           seed: int = 0, row_streams=None, forced=None, min_new_tokens: int = 0,
                           max_length: Optional[int] = None):
        """``test_sample_top_logprobs`` under a ``set_sequence_bias`` table for this call only (cw_test_sample_biased; ``table``
        None or empty: none): returns (choice [nb], logprob [nb], top ids [nb][k], top logprobs [nb][k], processed-score
        log-probability term [nb]) of index t."""
        lg = np.ascontiguousarray(logits, np.float32)
        ids = _i32(ids)
        nb, t = ids.shape
        if lg.shape != (nb, self.spec.vocab_size):
            raise ValueError(f"logits must be [{nb}][{self.spec.vocab_size}], got {lg.shape}")
        if not 1 <= int(k) <= 8:
            raise ValueError(f"k must be in 1 .. 8, got {k}")
        rs = None if row_streams is None else np.ascontiguousarray(row_streams, dtype=np.uint64)
        if rs is not None and rs.shape != (nb,):
            raise ValueError(f"row_streams must hold one id per row ({nb}), got shape {rs.shape}")
        fr = None if forced is None else _i32(forced)
        if fr is not None and fr.shape != (nb,):
            raise ValueError(f"forced must hold one token per row ({nb}), got shape {fr.shape}")
        table = list(table) if table is not None else []
        toks = _i32([t_ for s, _ in table for t_ in s]) if table else None
        lens = _i32([len(s) for s, _ in table]) if table else None
        bias = np.ascontiguousarray([b for _, b in table], np.float32) if table else None
        out = np.zeros(nb, np.int32)
        lp = np.zeros(nb, np.float32)
        top_id = np.zeros((nb, int(k)), np.int32)
        top_lp = np.zeros((nb, int(k)), np.float32)
        proc = np.zeros(nb, np.float32)
        self._chk(self.lib.cw_test_sample_biased(self.ctx, nb, _ptr(lg), _ptr(ids), t, int(n_prompt), int(min_new_tokens),
                                                 int(max_length or self.spec.max_target_positions), float(temperature),
                                                 int(seed) & (2 ** 64 - 1), _ptr(rs), _ptr(fr), int(k), len(table), _ptr(toks),
                                                 _ptr(lens), _ptr(bias), _ptr(out), _ptr(lp), _ptr(top_id), _ptr(top_lp),
                                                 _ptr(proc)))
        return out, lp, top_id, top_lp, proc

    # ------------------------------------------------------------------ measurement
    def stage_times(self, reset: bool = False):
        ms = np.zeros(len(N.STAGES), np.float32)
        calls = np.zeros(len(N.STAGES), np.int32)
        self._chk(self.lib.cw_stage_times(self.ctx, _ptr(ms), _ptr(calls), int(reset)))
        return {s: (float(ms[i]), int(calls[i])) for i, s in enumerate(N.STAGES)}

    def time_kernel(self, which: int, nb: int, iters: int):
        ms = C.c_float(0.0)
        by = C.c_double(0.0)
        self._chk(self.lib.cw_time_kernel(self.ctx, which, nb, iters, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def time_decode_stages(self, nb: int, iters: int):
        """Every launch of the decoder layer as the decode step issues it for `nb` greedy rows, timed one at a time (HIP events on
        the engine's stream, layers cycled): [{"stage", "kernel", "avg_ms", "algo_bytes"}], plus the whole layer as stage -1."""
        out = []
        ms, by, kind, ns = C.c_float(0.0), C.c_double(0.0), C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.cw_time_decode_stage(self.ctx, nb, -1, iters, C.byref(ms), C.byref(by), C.byref(kind), C.byref(ns)))
        out.append({"stage": -1, "kernel": "whole decoder layer (all launches)", "avg_ms": ms.value, "algo_bytes": by.value})
        for s in range(ns.value):
            self._chk(self.lib.cw_time_decode_stage(self.ctx, nb, s, iters, C.byref(ms), C.byref(by), C.byref(kind), C.byref(ns)))
            out.append({"stage": s, "kernel": self.lib.cw_decode_stage_name(kind.value).decode(), "avg_ms": ms.value, "algo_bytes": by.value,
                        "launches": int(self.lib.cw_decode_stage_launches(self.ctx, s))})
        return out
