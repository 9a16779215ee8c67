"""Host control flow of ``WhisperGenerationMixin.generate`` for the word-timestamp path.

Mirrors (call surface, argument meaning, error behaviour) the parts of
TF/models/whisper/generation_whisper.py the reference pipeline reaches with
``return_timestamps="word"`` and ``num_beams=1``: init tokens (:1455-1608, explicit language/task),
the seek loop (:785-903) with batch shrinking (:1814-1829), window slicing (:1831-1852), padding and
eos stripping (:1060-1082), ``_retrieve_segment`` (:1977-2074) and the final assembly (:936-968 as
consumed by TF/pipelines/automatic_speech_recognition.py:529-540).  All tensor work is delegated to
the device through ``Engine``; this module only decides *what* to run next from the decoded ids.
"""
from __future__ import annotations

import dataclasses
import math
import zlib
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from ._native import N_FRAMES
from .engine import Engine

TIME_PRECISION = 0.02          # seconds per encoder frame (30 / 1500)
INPUT_STRIDE = 2               # conv1.stride * conv2.stride
TOP_LOGPROBS_MAX = 8           # CW_TOP_LOGPROBS_MAX: alternatives per token (generate(top_logprobs=k))
SEQUENCE_BIAS_MAX = 256        # CW_SEQUENCE_BIAS_MAX: sequences per table (generate(sequence_bias=...))
SEQUENCE_BIAS_MAX_LEN = 16     # CW_SEQUENCE_BIAS_MAX_LEN: tokens per sequence
LANG_IDS_MAX = 128             # CW_LANG_IDS_MAX: candidate languages of one detection (Engine.detect_language)


@dataclasses.dataclass
class Segment:
    tokens: np.ndarray             # int64
    token_timestamps: np.ndarray   # float32, absolute seconds within the 30 s chunk
    idxs: tuple
    token_logprobs: Optional[np.ndarray] = None   # float32, one per token (generate(return_token_logprobs=True))
    top_ids: Optional[np.ndarray] = None          # int32 [n_tok][k]: the k best raw logits of each token's step (generate(top_logprobs=k))
    top_logprobs: Optional[np.ndarray] = None     # float32 [n_tok][k]: their log-probabilities (-1 / NaN: fewer than k candidates)
    alignment_scores: Optional[np.ndarray] = None   # float32, one per token: attention mass on the DTW path (generate(return_alignment_scores=True))
    alignment_spreads: Optional[np.ndarray] = None  # float32, one per token: spread of the attention in seconds
    token_entropy: Optional[np.ndarray] = None      # float32, one per token: entropy of its step's raw distribution (generate(return_token_entropy=True))


def detect_language(engine: Engine, n_items: int) -> np.ndarray:
    """``WhisperGenerationMixin.detect_language`` (:1610-1673): one decoder step on <|startoftranscript|>
    over the already-encoded windows, argmax restricted to the language tokens.  Returns [n_items] ids.
    (HF runs a second encoder pass for this; the native path reuses the encoder output of the first
    seek iteration, which covers the same 3000-frame window.)"""
    return detect_language_probs(engine, n_items)[0]


def detect_language_probs(engine: Engine, n_items: int, lang_ids=None):
    """``detect_language`` with the probability of the winner: ([n_items] int64 ids, [n_items] float32 probabilities -- the
    softmax over the candidate language tokens alone, as Whisper's own detect_language computes it).  ``lang_ids``: the
    candidates (default: every language of the generation config).  The device engine does this in one kernel on the logits
    where they lie (``Engine.detect_language``); an engine double without it goes through ``decode`` + ``last_logits``."""
    spec = engine.spec
    if not spec.lang_to_id:
        raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
    lang_ids = np.array(sorted(set(spec.lang_to_id.values()) if lang_ids is None else set(int(t) for t in lang_ids)), dtype=np.int64)
    if hasattr(engine, "detect_language"):
        best, prob, _ = engine.detect_language(n_items, lang_ids, no_speech=False)
        best = np.asarray(best, np.int64)
        col = np.searchsorted(lang_ids, best)
        return best, np.asarray(prob, np.float32)[np.arange(n_items), col]
    prompt = np.full((n_items, 1), spec.decoder_start_token_id, dtype=np.int32)
    engine.decode(prompt, max_length=2)
    logits = engine.last_logits(n_items)
    cand = np.asarray(logits)[:, lang_ids]
    win = np.argmax(cand, axis=-1)
    c64 = cand.astype(np.float64)
    e = np.exp(c64 - c64.max(axis=-1, keepdims=True))
    return lang_ids[win], (e[np.arange(n_items), win] / e.sum(axis=-1)).astype(np.float32)


def check_language_candidates(spec, candidates):
    """``language_candidates``: the languages auto-detection may answer with, in any form ``language_to_id`` accepts ('<|en|>',
    'en', 'english'); at least one, no language twice.  Returns their token ids, ascending; None for None."""
    if candidates is None:
        return None
    if isinstance(candidates, (str, bytes)) or not hasattr(candidates, "__len__"):
        raise ValueError(f"language_candidates is a list of languages, got {candidates!r}")
    if len(candidates) == 0:
        raise ValueError("language_candidates needs at least one language")
    if not spec.lang_to_id:
        raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
    ids = []
    for c in candidates:
        if not isinstance(c, str):
            raise ValueError(f"language_candidates holds {c!r}: every entry is a language name, code or <|tag|>")
        t = language_to_id(spec, c)
        if t in ids:
            raise ValueError(f"language_candidates lists {c!r} twice")
        ids.append(t)
    return sorted(ids)


def language_to_id(spec, language: str) -> int:
    """``language_to_id`` of ``_retrieve_init_tokens`` (:1466-1486): '<|en|>', 'en' and 'english' (any case) all work."""
    from .languages import TO_LANGUAGE_CODE
    language = language.lower()
    if language in spec.lang_to_id:
        tag = language
    elif language in TO_LANGUAGE_CODE:
        tag = f"<|{TO_LANGUAGE_CODE[language]}|>"
    elif language in TO_LANGUAGE_CODE.values():
        tag = f"<|{language}|>"
    else:
        is_code = len(language) == 2
        raise ValueError(f"Unsupported language: {language}. Language should be one of:"
                         f" {list(TO_LANGUAGE_CODE.values()) if is_code else list(TO_LANGUAGE_CODE.keys())}.")
    if tag not in spec.lang_to_id:
        raise ValueError(f"{tag} is not supported by this specific model as it is not in the "
                         "`generation_config.lang_to_id`. (You should just add it to the generation config)")
    return spec.lang_to_id[tag]


def resolve_prompt(spec, language: Optional[str], task: Optional[str]):
    """``_retrieve_init_tokens`` (:1455-1608) for ``return_timestamps=True``: the decoder prompt as a list whose slot 1
    is ``None`` when the language has to be detected per item.  ``language`` / ``task`` are the call's generate_kwargs;
    the generation config's own ``language`` / ``task`` are their defaults, and when both are unset the (deprecated but
    still shipped) ``forced_decoder_ids`` of the checkpoint seed the prompt, e.g. [[1, None], [2, <|transcribe|>]]."""
    from .languages import TASK_IDS
    task = task if task is not None else getattr(spec, "task", None)
    language = language if language is not None else getattr(spec, "language", None)
    if isinstance(language, (list, tuple)):
        raise ValueError("per-item language lists are not supported on the native path: pass one language or None")
    init: List[Optional[int]] = [spec.decoder_start_token_id]
    if task is None and language is None:
        forced = getattr(spec, "forced_decoder_ids", None)
        if forced is not None:
            forced = [list(f) for f in forced]
            if forced and forced[0][0] == 1:
                i = 1
                while forced and forced[0][0] == i:
                    init.append(forced[0][1])
                    forced = forced[1:]
                    i += 1
                if forced:
                    raise ValueError(f"You are using token ids in `forced_decoder_ids` that do not seem to correctly follow "
                                     f"the prompt pattern of Whisper. Make sure that {forced} has an entry for all "
                                     f"indices >= 1 and < {forced[0][0]}.")
    lang_undefined = len(init) <= 1 or init[1] is None
    lang_id: Optional[int] = None
    detect = False
    if language is not None:
        lang_id = language_to_id(spec, language)
    elif spec.lang_to_id and lang_undefined:
        detect = True
    if lang_id is not None or detect:
        if len(init) > 1:
            init[1] = None if detect else lang_id
        else:
            init.append(None if detect else lang_id)
    if task is not None:
        if task not in TASK_IDS or task not in spec.task_to_id:
            raise ValueError(f"The `{task}` task is not supported. The task should be one of `{TASK_IDS}`")
        init.append(spec.task_to_id[task])
    elif language is not None and spec.task_to_id:
        if not any(t in init for t in spec.task_to_id.values()):
            init.append(spec.task_to_id["transcribe"])
    if init[-1] == spec.no_timestamps_token_id:          # return_timestamps=True drops a trailing <|notimestamps|>
        init = init[:-1]
    head, rest = init[:2], [t for t in init[2:] if t is not None]
    if len(head) == 2 and head[1] is None and not detect:
        head = head[:1]                                    # a None language nobody fills in is dropped like any None
    return head + rest, detect


def init_tokens(spec, language: Optional[str], task: Optional[str], lang_id: Optional[int] = None,
                prompt_ids=None) -> List[int]:
    """<|startoftranscript|><|lang|><|task|> (no <|notimestamps|>: return_timestamps=True); ``lang_id`` fills the
    language slot when it has to be detected.  ``prompt_ids`` (``processor.get_prompt_ids(text)``: <|startofprev|> p1 .. pk)
    go in front: the decoder input of generation_whisper.py:1909-1913."""
    toks, detect = resolve_prompt(spec, language, task)
    if detect:
        if lang_id is None:
            raise ValueError("language is None and no detected language id was supplied")
        toks = [toks[0], int(lang_id)] + toks[2:]
    pre = [] if prompt_ids is None else [int(t) for t in check_prompt_ids(spec, prompt_ids)]
    return pre + [int(t) for t in toks]


def check_prompt_ids(spec, prompt_ids) -> np.ndarray:
    """``prompt_ids`` as generate accepts them -- a 1-D integer list, numpy array or torch tensor of token ids in [0, vocab)
    -- as an int64 array; anything else raises."""
    if hasattr(prompt_ids, "detach") and hasattr(prompt_ids, "cpu"):      # torch.Tensor
        prompt_ids = prompt_ids.detach().cpu().numpy()
    if not isinstance(prompt_ids, (list, tuple, np.ndarray)):
        raise ValueError(f"prompt_ids must be a 1-D list, numpy array or torch tensor of token ids, got {type(prompt_ids).__name__}")
    if isinstance(prompt_ids, (list, tuple)) and not all(isinstance(t, (int, np.integer)) and not isinstance(t, bool)
                                                         for t in prompt_ids):
        raise ValueError("prompt_ids must hold integer token ids")
    a = np.asarray(prompt_ids)
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"prompt_ids must be a non-empty 1-D sequence of token ids (shape {a.shape})")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"prompt_ids must hold integer token ids (dtype {a.dtype})")
    if int(a.min()) < 0 or int(a.max()) >= spec.vocab_size:
        raise ValueError(f"prompt_ids must lie in [0, {spec.vocab_size}) (got {int(a.min())} .. {int(a.max())})")
    return a.astype(np.int64)


def check_prompt_length(spec, n_input: int, max_new_tokens: Optional[int]) -> None:
    """The length check of ``_set_max_new_tokens_and_length`` (generation_whisper.py:1920-1930) for a decoder input of
    ``n_input`` ids (prompt + init tokens)."""
    m = max_new_tokens if max_new_tokens is not None else 0
    tgt = spec.max_target_positions
    if m + n_input > tgt:
        raise ValueError(
            f"The length of `decoder_input_ids`, including special start tokens, prompt tokens, and previous tokens, is {n_input}, "
            f" and `max_new_tokens` is {m}. Thus, the combined length of "
            f"`decoder_input_ids` and `max_new_tokens` is: {m + n_input}. This exceeds the "
            f"`max_target_positions` of the Whisper model: {tgt}. "
            "You should either reduce the length of your prompt, or reduce the value of `max_new_tokens`, "
            f"so that their combined length is less than {tgt}.")


def prompted_max_length(spec, n_input: int, max_new_tokens: Optional[int]) -> int:
    """max_length of a generate call whose decoder input (``n_input`` ids) carries prompt_ids (:1932-1946)."""
    check_prompt_length(spec, n_input, max_new_tokens)
    tgt = spec.max_target_positions
    if max_new_tokens is not None:
        out = n_input + int(max_new_tokens)
    else:
        out = min(int(spec.max_length) + min(tgt // 2 - 1, n_input), tgt)
    if out <= n_input:
        raise ValueError(f"max_length {out} leaves no room to generate after the {n_input} decoder input ids (prompt + init "
                         f"tokens): pass max_new_tokens or a shorter prompt")
    return out


def split_segments(seq: np.ndarray, token_ts: np.ndarray, time_offset: float, timestamp_begin: int,
                   seek_num_frames: int, idx_offset: int, token_lp: Optional[np.ndarray] = None, token_top=None, token_align=None,
                   token_ent: Optional[np.ndarray] = None):
    """Slice one decoded window at paired timestamp tokens; returns (segments, frames to advance).  ``token_lp`` (per-token
    log-probabilities of the row, indexed like ``token_ts``), ``token_top`` (the row's (ids [T][k], log-probabilities [T][k])
    alternatives, indexed alike), ``token_align`` (the row's (mass, spread) alignment scores, indexed alike) and ``token_ent`` (the
    row's token entropies, indexed alike) are cut by the same index ranges."""
    def en(a, b):
        return None if token_ent is None else np.asarray(token_ent[a:b], dtype=np.float32).copy()

    def al(a, b):
        if token_align is None:
            return None, None
        return np.asarray(token_align[0][a:b], dtype=np.float32).copy(), np.asarray(token_align[1][a:b], dtype=np.float32).copy()

    def lp(a, b):
        return None if token_lp is None else np.asarray(token_lp[a:b], dtype=np.float32).copy()

    def top(a, b):
        if token_top is None:
            return None, None
        return np.asarray(token_top[0][a:b], dtype=np.int32).copy(), np.asarray(token_top[1][a:b], dtype=np.float32).copy()
    is_ts = seq >= timestamp_begin
    single_ending = len(seq) >= 2 and (not is_ts[-2]) and bool(is_ts[-1])
    if len(seq) == 1:
        single_ending = False                                   # tolist() == [True] != [False, True]
    pair_ends = np.nonzero(is_ts[:-1] & is_ts[1:])[0] + 1
    off32 = np.float32(time_offset)
    out: List[Segment] = []
    if len(pair_ends):
        cuts = pair_ends.tolist()
        if single_ending:
            cuts.append(len(seq))
        else:
            cuts[-1] += 1
        prev = 0
        for cut in cuts:
            out.append(Segment(seq[prev:cut], (token_ts[idx_offset + prev: idx_offset + cut] + off32).astype(np.float32),
                               (idx_offset + prev, idx_offset + cut), lp(idx_offset + prev, idx_offset + cut),
                               *top(idx_offset + prev, idx_offset + cut), *al(idx_offset + prev, idx_offset + cut),
                               en(idx_offset + prev, idx_offset + cut)))
            prev = cut
        if single_ending:
            advance = seek_num_frames
        else:
            advance = (int(seq[prev - 2]) - timestamp_begin) * INPUT_STRIDE
    else:
        out.append(Segment(seq, (token_ts[idx_offset: idx_offset + len(seq)] + off32).astype(np.float32),
                           (idx_offset, idx_offset + len(seq)), lp(idx_offset, idx_offset + len(seq)),
                           *top(idx_offset, idx_offset + len(seq)), *al(idx_offset, idx_offset + len(seq)),
                           en(idx_offset, idx_offset + len(seq))))
        advance = seek_num_frames
    return out, advance


def _topk_desc(values: np.ndarray, k: int) -> np.ndarray:
    """Indices of the k largest entries per row, largest first, ties towards the lower index (torch.topk on CPU)."""
    order = np.argsort(-values, axis=-1, kind="stable")
    return order[..., :k]


def _beam_search_native_host(engine, prompt, max_length, min_new_tokens, K, length_penalty, early_stopping):
    """The search loop over the native host half (csrc/beamhost.cpp): per decoder step one `cw_beam_step`, one
    `cw_beam_host_step` (candidates in, parent / token out) and one `cw_beam_advance`.  -> (sequences [B, max_length] int64,
    beam_indices [B, max_length - n_prompt] int32, scores [B] float32) of the best hypothesis per item."""
    import ctypes as C
    from . import _native
    lib = _native.load()
    spec = engine.spec
    pr = np.ascontiguousarray(prompt, dtype=np.int32)
    B, n_prompt = pr.shape
    st = lib.cw_beam_host_new(B, K, n_prompt, int(max_length), int(spec.vocab_size), int(spec.eos_token_id),
                              int(spec.pad_token_id or 0), float(length_penalty), 1 if early_stopping is True else 0,
                              pr.ctypes.data_as(C.c_void_p))
    if not st:
        raise ValueError(f"beam search: invalid geometry (items {B}, beams {K}, prompt {n_prompt}, max_length {max_length})")
    try:
        parent = np.empty(B * K, np.int32); token = np.empty(B * K, np.int32)
        engine.beam_begin(prompt, K, max_length, min_new_tokens)
        while True:
            vals, toks = engine.beam_step(2 * K)
            vals = np.ascontiguousarray(vals, dtype=np.float32); toks = np.ascontiguousarray(toks, dtype=np.int32)
            rc = lib.cw_beam_host_step(st, vals.ctypes.data_as(C.c_void_p), toks.ctypes.data_as(C.c_void_p),
                                       parent.ctypes.data_as(C.c_void_p), token.ctypes.data_as(C.c_void_p))
            if rc < 0:
                raise RuntimeError(f"cw_beam_host_step failed ({rc})")
            if rc == 0:
                break
            engine.beam_advance(parent, token)
        seqs = np.empty((B, max_length), np.int64); bi = np.empty((B, max_length - n_prompt), np.int32)
        sc = np.empty(B, np.float32)
        rc = lib.cw_beam_host_result(st, seqs.ctypes.data_as(C.c_void_p), bi.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"cw_beam_host_result failed ({rc})")
        tl = np.empty((B, max_length - n_prompt), np.float32)
        rc = lib.cw_beam_host_token_logprobs(st, tl.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise RuntimeError(f"cw_beam_host_token_logprobs failed ({rc})")
        return seqs, bi, sc, tl
    finally:
        lib.cw_beam_host_free(st)


def beam_search(engine: Engine, prompt: np.ndarray, max_length: int, min_new_tokens: int, num_beams: int,
                length_penalty: float = 1.0, early_stopping=False, native_host: Optional[bool] = None,
                return_token_logprobs: bool = False):
    """Host half of ``GenerationMixin._beam_search`` (TF/generation/utils.py:3208-3520) -- running / finished
    hypotheses, length penalty, the early-stopping heuristic (:3009-3053), all in float32 like HF -- over the device half
    (``Engine.beam_begin / beam_step / beam_advance / beam_finish``: decoder forwards on items x beams rows, log-softmax +
    logits processors, per-row best candidates, cache ancestry).  Deterministic beam search only (``do_sample=False``).

    Returns (sequences [B, n_prompt + max_generated] int64 padded with pad_token_id, beam_indices [B, max_generated]
    int32 flat row indices or -1, L = decoder input positions whose alignment rows were gathered for the returned
    sequences; ``engine.token_timestamps(B, L, n_prompt, ...)`` is valid afterwards).

    ``native_host`` (default True): the bookkeeping of every step runs in ``csrc/beamhost.cpp`` (one C call per step instead
    of ~45 numpy calls, 0.23 ms per step at 8 items x 5 beams); ``False`` keeps the numpy statement below, which
    ``tests/test_beam_host.py`` holds bit-equal to the native one on random candidate streams.

    ``return_token_logprobs=True`` appends a fifth value: [B, max_generated] float32, for every generated token of the
    returned hypothesis the candidate log-probability it was chosen with (``log_softmax`` of the raw logits of its step: a
    masked candidate is never chosen, so processed and raw value coincide), followed along the ancestry; NaN behind the end."""
    if early_stopping is not True and early_stopping is not False:
        # transformers also knows "never" (a third stopping heuristic, generation/utils.py:3042-3053); it is not implemented
        # here and must not be mistaken for False
        raise ValueError(f"early_stopping={early_stopping!r}: only True / False are implemented")
    spec = engine.spec
    f32 = np.float32
    prompt = np.asarray(prompt, dtype=np.int64)
    B, n_prompt = prompt.shape
    K, V = int(num_beams), spec.vocab_size
    if native_host is None or native_host:
        seqs, bi, sc, tl = _beam_search_native_host(engine, prompt, max_length, min_new_tokens, K, length_penalty, early_stopping)
        return _beam_search_tail(engine, seqs, bi, sc, n_prompt, tl if return_token_logprobs else None)
    eos, pad = spec.eos_token_id, spec.pad_token_id
    keep = max(2, 1 + 1) * K                                    # beams_to_keep (:3280-3281), one eos token id
    top_mask = np.arange(keep) < K
    fill = pad if pad else eos                                   # output_fill_value (:3323)
    running_seq = np.full((B, K, max_length), fill, dtype=np.int64)
    running_seq[:, :, :n_prompt] = prompt[:, None, :]
    sequences = running_seq.copy()
    running_scores = np.zeros((B, K), f32); running_scores[:, 1:] = f32(-1e9)
    beam_scores = np.full((B, K), f32(-1e9), f32)
    is_sent_finished = np.zeros((B, K), bool)
    unsat = np.ones((B, 1), bool)
    running_bi = np.full((B, K, max_length - n_prompt), -1, dtype=np.int32)
    beam_indices = running_bi.copy()
    running_tl = np.full((B, K, max_length - n_prompt), np.nan, dtype=f32)
    token_lp = running_tl.copy()
    cur_len = n_prompt
    bidx = np.arange(B)[:, None]
    engine.beam_begin(prompt, K, max_length, min_new_tokens)
    while True:
        vals, toks = engine.beam_step(keep)                      # [B*K, keep] processed log-probs, best first
        vals = vals.reshape(B, K, keep).astype(f32)
        toks = toks.reshape(B, K, keep).astype(np.int64)
        acc = (vals + running_scores[:, :, None]).astype(f32)    # :3436
        acc = np.where(toks >= 0, acc, f32(-np.inf)).reshape(B, K * keep)
        flat = (np.arange(K)[None, :, None] * V + np.maximum(toks, 0)).reshape(B, K * keep)
        # top `keep` of the union in (value desc, flattened index asc) order == torch.topk over [B, K * V] (:3147)
        order = np.lexsort((flat, -acc), axis=-1)[:, :keep]
        topk_lp = np.take_along_axis(acc, order, axis=1)
        topk_flat = np.take_along_axis(flat, order, axis=1)
        topk_cand = np.take_along_axis(vals.reshape(B, K * keep), order, axis=1)   # before the running score is added
        topk_beam, topk_ids = topk_flat // V, topk_flat % V
        topk_seq = running_seq[bidx, topk_beam]                   # [B, keep, max_length]
        topk_seq[:, :, cur_len] = topk_ids
        topk_bi = running_bi[bidx, topk_beam]
        topk_bi[:, :, cur_len - n_prompt] = (topk_beam + np.arange(B)[:, None] * K).astype(np.int32)
        topk_tl = running_tl[bidx, topk_beam]
        topk_tl[:, :, cur_len - n_prompt] = topk_cand
        # d. stopping criteria: eos token, max length (:3456-3462)
        hits = (topk_ids == eos) | (cur_len + 1 >= max_length)
        # e. running beams of the next iteration (:3173-3190)
        run_lp = (topk_lp + hits.astype(f32) * f32(-1.0e9)).astype(f32)
        nxt = _topk_desc(run_lp, K)
        running_seq = np.take_along_axis(topk_seq, nxt[:, :, None], axis=1)
        running_scores = np.take_along_axis(run_lp, nxt, axis=1)
        running_bi = np.take_along_axis(topk_bi, nxt[:, :, None], axis=1)
        running_tl = np.take_along_axis(topk_tl, nxt[:, :, None], axis=1)
        # f. finished hypotheses (:3192-3245)
        did_top = hits & top_mask[None, :]
        lp2 = (topk_lp / f32((cur_len + 1 - n_prompt) ** length_penalty)).astype(f32)
        full = np.all(is_sent_finished, axis=-1, keepdims=True) & (early_stopping is True)
        lp2 = (lp2 + full.astype(f32) * f32(-1.0e9)).astype(f32)
        lp2 = (lp2 + (~unsat).astype(f32) * f32(-1.0e9)).astype(f32)
        lp2 = (lp2 + (~did_top).astype(f32) * f32(-1.0e9)).astype(f32)
        m_seq = np.concatenate([sequences, topk_seq], axis=1)
        m_scores = np.concatenate([beam_scores, lp2], axis=1)
        m_bi = np.concatenate([beam_indices, topk_bi], axis=1)
        m_fin = np.concatenate([is_sent_finished, did_top], axis=1)
        sel = _topk_desc(m_scores, K)
        sequences = np.take_along_axis(m_seq, sel[:, :, None], axis=1)
        beam_scores = np.take_along_axis(m_scores, sel, axis=1)
        beam_indices = np.take_along_axis(m_bi, sel[:, :, None], axis=1)
        token_lp = np.take_along_axis(np.concatenate([token_lp, topk_tl], axis=1), sel[:, :, None], axis=1)
        is_sent_finished = np.take_along_axis(m_fin, sel, axis=1)
        # g. next iteration: cache re-ordering (device), stopping condition of the search as a whole
        parent = running_bi[:, :, cur_len - n_prompt].reshape(-1)
        token = running_seq[:, :, cur_len].reshape(-1)
        cur_len += 1
        best_len = cur_len - n_prompt                              # early_stopping False / length_penalty: :3042-3053
        best_possible = (running_scores[:, :1] / f32(best_len ** length_penalty)).astype(f32)
        worst_finished = np.where(is_sent_finished, beam_scores.min(axis=1, keepdims=True), f32(-1.0e9))
        unsat = unsat & np.any(best_possible > worst_finished, axis=-1, keepdims=True)
        go_on = bool(np.any(unsat)) and (not (bool(np.all(is_sent_finished)) and early_stopping is True)) and (not bool(np.all(hits)))
        if not go_on:
            break
        engine.beam_advance(parent, token)
    return _beam_search_tail(engine, sequences[:, 0, :], beam_indices[:, 0, :], beam_scores[:, 0], n_prompt,
                             token_lp[:, 0, :] if return_token_logprobs else None)


def _beam_search_tail(engine, seq_out, bi_out, scores, n_prompt, tl_out=None):
    """Trim to the longest returned hypothesis and gather the alignment rows of the returned sequences."""
    max_gen = int((bi_out != -1).sum(axis=1).max())
    seq_out = seq_out[:, :n_prompt + max_gen]
    bi_out = bi_out[:, :max_gen]
    # cross-attention rows of the returned sequences: HF's unrolled beam_indices (generation_whisper.py:262-303),
    # -1 (positions after a hypothesis' eos) -> row 0
    unrolled = np.concatenate([np.repeat(bi_out[:, :1], n_prompt - 1, axis=1), bi_out], axis=1) if n_prompt > 1 else bi_out
    unrolled = np.where(unrolled == -1, 0, unrolled).astype(np.int32)
    engine.beam_finish(unrolled)
    if tl_out is not None:
        return seq_out, bi_out, unrolled.shape[1], np.asarray(scores, dtype=np.float32), np.asarray(tl_out[:, :max_gen], np.float32)
    return seq_out, bi_out, unrolled.shape[1], np.asarray(scores, dtype=np.float32)


MAX_FALLBACK_TEMPERATURES = 16          # the temperature index takes the low 4 bits of a row's stream id


def normalise_temperatures(temperature) -> Tuple[float, ...]:
    """``temperature`` of ``generate`` as a tuple of finite floats >= 0 (None: (0.0,)); at most 16 entries."""
    if temperature is None:
        return (0.0,)
    temps = tuple(temperature) if isinstance(temperature, (tuple, list)) else (temperature,)
    if len(temps) == 0:
        raise ValueError("temperature: an empty tuple decodes nothing")
    if len(temps) > MAX_FALLBACK_TEMPERATURES:
        raise ValueError(f"temperature: at most {MAX_FALLBACK_TEMPERATURES} fallback temperatures are supported (the temperature "
                         f"index is 4 bits of the sampler's stream id), got {len(temps)}")
    out = []
    for t in temps:
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)):
            raise ValueError(f"temperature must be a number or a tuple of numbers, got {t!r}")
        t = float(t)
        if not (t >= 0.0) or math.isinf(t):
            raise ValueError(f"temperature must be finite and >= 0, got {t!r}")
        out.append(t)
    return tuple(out)


def compression_ratio(tokens, vocab_size: int) -> float:
    """``_retrieve_compression_ratio`` (generation_whisper.py:1949): raw bytes over zlib-compressed bytes of the tokens written
    as fixed-width little-endian integers."""
    length = int(math.log2(vocab_size) / 8) + 1
    token_bytes = b"".join(int(t).to_bytes(length, "little") for t in np.asarray(tokens).tolist())
    return len(token_bytes) / len(zlib.compress(token_bytes))


def need_fallback(tokens, vocab_size, avg_logprob, no_speech_prob, compression_ratio_threshold, logprob_threshold,
                  no_speech_threshold):
    """``_need_fallback`` (generation_whisper.py:1243-1287) for one window: ``tokens`` are the generated tokens with the padding
    stripped and the eos kept.  Returns (needs_fallback, should_skip, compression ratio or None)."""
    needs, skip, cr = False, False, None
    if compression_ratio_threshold is not None:
        cr = compression_ratio(tokens, vocab_size)
        if cr > compression_ratio_threshold:
            needs = True
    if logprob_threshold is not None and float(avg_logprob) < logprob_threshold:
        needs = True
    if no_speech_threshold is not None:
        if float(avg_logprob) < logprob_threshold and float(no_speech_prob) > no_speech_threshold:
            needs, skip = False, True
    return needs, skip, cr


def stream_id(item_id: int, seek_frame: int, temperature_index: int) -> int:
    """The sampler's 64-bit stream of a window: stream_lo = the caller's item id (the pipeline passes the global window index),
    stream_hi = (seek_frame << 4) | temperature_index."""
    if not 0 <= temperature_index < MAX_FALLBACK_TEMPERATURES:
        raise ValueError(f"temperature index {temperature_index} outside 0 .. {MAX_FALLBACK_TEMPERATURES - 1}")
    hi = ((int(seek_frame) << 4) | int(temperature_index)) & 0xFFFFFFFF
    return (hi << 32) | (int(item_id) & 0xFFFFFFFF)


def check_sequence_bias(sequence_bias, vocab_size: int):
    """transformers' ``sequence_bias`` (the list form ``[[[ids...], bias], ...]`` or the dict form ``{(ids...): bias}``) as a list
    of ``(ids tuple, float bias)`` in the order SequenceBiasLogitsProcessor sums them, or None for None.  Refuses with ValueError
    what the processor's ``_validate_arguments`` refuses (an empty container, non-tuple keys, negative ids, ids <= 0 in the list
    form, biases that are no floats) and what the engine cannot honour: empty sequences, ids >= ``vocab_size`` (transformers raises
    at the first step), more than SEQUENCE_BIAS_MAX sequences or SEQUENCE_BIAS_MAX_LEN tokens, non-finite biases.  Duplicates in
    the list form collapse as the processor's dict conversion does: the last bias wins, at the first one's place."""
    if sequence_bias is None:
        return None
    sb = sequence_bias
    if not isinstance(sb, (dict, list)) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb!r}")

    def is_id(t):
        return isinstance(t, (int, np.integer)) and not isinstance(t, (bool, np.bool_))
    if isinstance(sb, dict):
        if any(not isinstance(k, tuple) for k in sb):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb!r}")
        if any(len(k) == 0 or any(not is_id(t) or t < 0 for t in k) for k in sb):
            raise ValueError(f"each key in `sequence_bias` has to be a non-empty tuple of non-negative integers, but is {sb!r}")
        table = dict(sb)
    else:
        for e in sb:
            if (not isinstance(e, (list, tuple)) or len(e) != 2 or not isinstance(e[0], list) or len(e[0]) == 0
                    or any(not is_id(t) or t <= 0 for t in e[0]) or not isinstance(e[1], float)):
                raise ValueError("each element in `sequence_bias` has to be [non-empty list of positive integers, float], "
                                 f"but one is {e!r}")
        table = {tuple(int(t) for t in e[0]): e[1] for e in sb}
    if any(not isinstance(b, float) for b in table.values()):
        raise ValueError(f"`sequence_bias` has to hold floats as biases, but is {sb!r}")
    if len(table) > SEQUENCE_BIAS_MAX:
        raise ValueError(f"sequence_bias holds {len(table)} sequences; at most {SEQUENCE_BIAS_MAX} are implemented")
    out = []
    for k, b in table.items():
        if len(k) > SEQUENCE_BIAS_MAX_LEN:
            raise ValueError(f"sequence_bias: a sequence of {len(k)} tokens; at most {SEQUENCE_BIAS_MAX_LEN} are implemented")
        bad = [int(t) for t in k if t >= vocab_size]
        if bad:
            raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being biased: {bad}")
        if not np.isfinite(b):
            raise ValueError(f"sequence_bias: the bias of {k} is {b}; it has to be finite")
        out.append((tuple(int(t) for t in k), float(b)))
    return out


def check_alignment_collar(spec, collar) -> int:
    """``alignment_collar_frames``: None = ``median_filter_width // 2`` (the most the median filter can move an edge), else a
    non-negative integer number of 20 ms frames."""
    if collar is None:
        return int(spec.median_filter_width) // 2
    if isinstance(collar, (bool, np.bool_)) or not isinstance(collar, (int, np.integer)) or int(collar) < 0:
        raise ValueError(f"alignment_collar_frames must be a non-negative integer number of frames, got {collar!r}")
    return int(collar)


def set_alignment_scores(engine, want: bool, collar: int):
    """The engine's alignment-score switch as a call wants it.  A call without the flag touches the engine only to switch off
    what an earlier call switched on (``engine.alignment_scores_on``): on an engine that never had it on, such a call is what it
    was before the switch existed, whatever state the engine is in."""
    if hasattr(engine, "set_alignment_scores") and (want or getattr(engine, "alignment_scores_on", False)):
        engine.set_alignment_scores(want, collar)


def generate(engine: Engine, n_items: int, num_frames, *, language: Optional[str], task: Optional[str] = None,
             max_new_tokens: Optional[int] = None, min_new_tokens: Optional[int] = None,
             num_beams: Optional[int] = 1, stats: Optional[dict] = None, native: Optional[bool] = None,
             logprob_threshold: Optional[float] = None, no_speech_threshold: Optional[float] = None, prompt_ids=None,
             temperature=None, compression_ratio_threshold: Optional[float] = None, sampling_seed: int = 0, item_ids=None,
             return_token_logprobs: bool = False, top_logprobs: int = 0, sequence_bias=None,
             return_alignment_scores: bool = False, alignment_collar_frames: Optional[int] = None, language_candidates=None,
             return_token_entropy: bool = False):
    """Transcribe the ``n_items`` 30 s feature windows resident in the engine (items 0..n-1).

    Returns {"sequences": [B, Lmax] int64 (pad-right), "token_timestamps": list of float32 arrays,
    "segments": list of list of Segment (host loop only)} -- the fields the pipeline consumes -- and, in every decoding mode,
    "languages": [B] int64, the language token each item was decoded with (forced or detected; -1 when the decoder prompt
    carries none, as for an English-only checkpoint) and "language_probs": [B] float32, the detection probability (the softmax
    over the candidate language tokens alone; NaN where the language was forced).

    ``language_candidates`` (only with ``language=None``): the languages auto-detection may answer with, in any form
    ``language_to_id`` accepts; at least one, none twice (``check_language_candidates``).

    ``native`` (default: whenever the engine exports it) runs the seek loop inside the library
    (``cw_transcribe``, one C call per batch); ``native=False`` runs the same control flow here, stage by stage
    over ``cw_encode`` / ``cw_decode`` / ``cw_token_timestamps`` -- the two are tested to agree exactly.

    ``logprob_threshold`` / ``no_speech_threshold``: the deterministic (temperature 0) half of HF's
    ``generate_with_fallback`` (generation_whisper.py:970-1116, ``_need_fallback`` :1243-1287): a window whose average token
    log-probability is below the first AND whose no-speech probability is above the second is skipped -- seek moves on by the
    whole window, no segment (:879-881).

    ``temperature`` (a number or a tuple of up to 16) together with ``compression_ratio_threshold`` / ``logprob_threshold`` is the
    stochastic half: the windows that fail a threshold at one temperature are decoded again at the next (only those rows are
    live; the encoder does not run again), the last temperature's result is kept unconditionally.  Positive temperatures sample
    with the engine's seeded Gumbel-max sampler (``cw_set_sampling``): key ``sampling_seed``, stream ``stream_id(item_ids[i],
    seek, temperature index)`` (``item_ids`` defaults to 0 .. n_items-1), so a window's tokens do not depend on the batch it is
    decoded in.  Without a threshold only the first temperature is used, as in transformers.  Greedy rows only; it runs on the
    host seek loop.  ``stats["fallback"]`` receives one record per (window, temperature) decode that was judged.

    ``prompt_ids`` (``processor.get_prompt_ids(text)``): every window of every seek pass decodes from
    ``prompt_ids ++ init_tokens`` (generation_whisper.py:1909-1913, condition_on_prev_tokens False); language detection still
    runs on <|startoftranscript|> alone; the prompt is never part of the output.

    ``return_token_logprobs=True`` adds "token_logprobs": one float32 array per item aligned with ``token_timestamps``,
    ``logits[tok] - logsumexp(logits[:vocab])`` on the raw logits of the step that produced each token (the quantity ``score``
    reports).  Greedy, sampled and forced rows take it from the sampler kernels (``cw_set_token_logprobs``), beam search from
    the candidate values along the winning hypothesis' ancestry; no extra forward runs.

    ``top_logprobs=k`` (1 .. 8; needs ``return_token_logprobs=True`` and ``num_beams=1``) adds "top_ids" and "top_logprobs": one
    [n_tok][k] array per item aligned with ``token_timestamps``, the ids (int32) and log-probabilities (float32) of the k best raw
    logits of each token's step, best first, ties to the lower id (``cw_set_top_logprobs``): no suppress lists, no timestamp
    rule, no temperature, so the written token need not be among them; where it is, its value equals ``token_logprobs`` bit for
    bit.  A rank beyond the number of finite logits holds -1 / NaN.

    ``return_token_entropy=True`` (needs ``return_token_logprobs=True`` and ``num_beams=1``) adds "token_entropy": one float32
    array per item aligned with ``token_timestamps``, the predictive entropy in nats of the raw distribution of each token's step
    (``cw_set_token_entropy``): no suppress lists, no timestamp rule, no temperature, no ``sequence_bias``, and independent of the
    token that was written.  Under temperature fallback the values are those of the pass that was kept.

    ``sequence_bias`` (transformers' list or dict form, ``check_sequence_bias``; needs ``num_beams=1``): phrase boosting with the
    semantics of SequenceBiasLogitsProcessor, applied inside the sampler kernels (``cw_set_sequence_bias``) in front of every other
    logits processor, in every window and every fallback re-decode.  The prompt tokens take part in the prefix match.  The raw
    outputs ("token_logprobs", "top_logprobs") are unchanged by it.  The table is cleared again when the call ends or raises.

    ``return_alignment_scores=True`` adds "alignment_scores" and "alignment_spreads": one float32 array each per item aligned
    with ``token_timestamps``.  The first is the share of the alignment heads' attention that lies inside the frames the DTW path
    gave the token, widened by ``alignment_collar_frames`` 20 ms frames on either side (None: ``median_filter_width // 2``, the
    most the median filter can move an edge); the second the standard deviation of that attention over the frames, in seconds
    (``cw_set_alignment_scores``; NaN where undefined).  One reduction kernel behind every DTW, in every decoding mode; nothing
    else in the result changes."""
    spec = engine.spec
    table = check_sequence_bias(sequence_bias, spec.vocab_size)
    if table is not None:
        if num_beams is not None and int(num_beams) > 1:
            raise ValueError("sequence_bias is implemented for greedy and sampled decoding only (beam search would add it to "
                             "log_softmax(raw), which moves the normaliser): pass num_beams=1")
        if not hasattr(engine, "set_sequence_bias"):
            raise ValueError("this engine does not implement sequence_bias (cw_set_sequence_bias)")
        # the call proper (_generate) checks its own arguments before it touches the engine; whatever happens there, the table
        # does not outlive the call
        engine.set_sequence_bias(table)
    try:
        return _generate(engine, n_items, num_frames, language=language, task=task, max_new_tokens=max_new_tokens,
                         min_new_tokens=min_new_tokens, num_beams=num_beams, stats=stats, native=native,
                         logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold, prompt_ids=prompt_ids,
                         temperature=temperature, compression_ratio_threshold=compression_ratio_threshold,
                         sampling_seed=sampling_seed, item_ids=item_ids, return_token_logprobs=return_token_logprobs,
                         top_logprobs=top_logprobs, return_alignment_scores=return_alignment_scores,
                         alignment_collar_frames=alignment_collar_frames, language_candidates=language_candidates,
                         return_token_entropy=return_token_entropy)
    finally:
        if table is not None:
            engine.set_sequence_bias(None)


def _generate(engine: Engine, n_items: int, num_frames, *, language, task, max_new_tokens, min_new_tokens, num_beams, stats, native,
              logprob_threshold, no_speech_threshold, prompt_ids, temperature, compression_ratio_threshold, sampling_seed, item_ids,
              return_token_logprobs, top_logprobs, return_alignment_scores=False, alignment_collar_frames=None,
              language_candidates=None, return_token_entropy=False):
    """``generate`` proper: everything but the sequence_bias table, which ``generate`` sets around this call."""
    spec = engine.spec
    cand_ids = check_language_candidates(spec, language_candidates)
    if cand_ids is not None and (language is not None or not resolve_prompt(spec, language, task)[1]):
        raise ValueError("language_candidates restricts language auto-detection: it cannot be combined with a language that is "
                         "given (generate_kwargs['language'] or the generation config's own)")
    want_as = bool(return_alignment_scores)
    collar = check_alignment_collar(spec, alignment_collar_frames)
    if want_as and not hasattr(engine, "set_alignment_scores"):
        raise ValueError("this engine does not implement alignment scores (cw_set_alignment_scores)")
    want_lp = bool(return_token_logprobs)
    if want_lp and not hasattr(engine, "set_token_logprobs"):
        raise ValueError("this engine does not implement per-token log-probabilities (cw_set_token_logprobs)")
    want_top = 0 if top_logprobs is None else top_logprobs
    if isinstance(want_top, bool) or not isinstance(want_top, (int, np.integer)) or not 0 <= int(want_top) <= TOP_LOGPROBS_MAX:
        raise ValueError(f"top_logprobs must be an integer in 0 .. {TOP_LOGPROBS_MAX}, got {top_logprobs!r}")
    want_top = int(want_top)
    if want_top:
        if not want_lp:
            raise ValueError("top_logprobs needs return_token_logprobs=True (the alternatives share its normaliser)")
        if num_beams is not None and int(num_beams) > 1:
            raise ValueError("top_logprobs is implemented for greedy and sampled decoding only (beam search re-parents its rows "
                             "every step): pass num_beams=1")
        if not hasattr(engine, "set_top_logprobs"):
            raise ValueError("this engine does not implement top_logprobs (cw_set_top_logprobs)")
    want_ent = bool(return_token_entropy)
    if want_ent:
        if not want_lp:
            raise ValueError("return_token_entropy needs return_token_logprobs=True (the entropy shares its running sums)")
        if num_beams is not None and int(num_beams) > 1:
            raise ValueError("return_token_entropy is implemented for greedy and sampled decoding only (beam search re-parents its "
                             "rows every step): pass num_beams=1")
        if not hasattr(engine, "set_token_entropy"):
            raise ValueError("this engine does not implement token entropy (cw_set_token_entropy)")
    if no_speech_threshold is not None and logprob_threshold is None:
        raise ValueError("no_speech_threshold needs logprob_threshold as well (generation_whisper.py:1275-1285 compares both)")
    # every argument is checked before any engine state changes (a refused call must not leave its thresholds behind)
    skip_on = logprob_threshold is not None and no_speech_threshold is not None
    prefix = None
    if prompt_ids is not None:
        prefix = check_prompt_ids(spec, prompt_ids)
        if logprob_threshold is not None or no_speech_threshold is not None:
            raise ValueError("prompt_ids together with logprob_threshold / no_speech_threshold is not implemented on the native "
                             "path (the no-speech position moves with the prompt)")
        prompted_max_length(spec, len(prefix) + len(resolve_prompt(spec, language, task)[0]), max_new_tokens)
    if skip_on and num_beams is not None and int(num_beams) > 1:
        raise ValueError("logprob_threshold / no_speech_threshold are implemented for greedy decoding only: pass num_beams=1")
    num_beams = 1 if num_beams is None else int(num_beams)
    if num_beams < 1:
        raise ValueError(f"`num_beams` has to be an integer strictly greater than 0, but is {num_beams}")
    if num_beams * n_items > engine.max_batch:
        raise ValueError(f"beam search decodes items x beams = {num_beams * n_items} rows; the engine was created with "
                         f"max_batch = {engine.max_batch}")
    temps = normalise_temperatures(temperature)
    if compression_ratio_threshold is None and logprob_threshold is None and no_speech_threshold is None:
        temps = temps[:1]                               # no threshold, no fallback: the first temperature is kept (:1100-1104)
    fb = None
    if len(temps) > 1 or temps[0] > 0.0:
        if num_beams > 1:
            raise ValueError("a positive temperature samples, and sampling decodes greedy rows only (transformers forces "
                             "num_beams = 1 there, generation_whisper.py:1004-1005): pass num_beams=1")
        if prefix is not None and len(temps) > 1:
            raise ValueError("temperature fallback together with prompt_ids is not implemented on the native path")
        if not hasattr(engine, "set_sampling"):
            raise ValueError("this engine does not implement sampling (cw_set_sampling)")
        ids_ = list(range(n_items)) if item_ids is None else [int(i) for i in item_ids]
        if len(ids_) != n_items:
            raise ValueError(f"{len(ids_)} item_ids for {n_items} items")
        fb = {"temps": temps, "seed": int(sampling_seed), "item_ids": ids_, "cr_thr": compression_ratio_threshold,
              "token_logprobs": want_lp, "top_logprobs": want_top, "alignment_scores": want_as, "token_entropy": want_ent}
        native = False                                  # the fallback loop runs here, like beam search
    if hasattr(engine, "set_thresholds"):
        engine.set_thresholds(logprob_threshold, no_speech_threshold)
    elif logprob_threshold is not None:
        raise ValueError("this engine does not implement logprob_threshold / no_speech_threshold")
    if hasattr(engine, "set_token_logprobs"):
        engine.set_token_logprobs(want_lp)
    if hasattr(engine, "set_top_logprobs"):
        engine.set_top_logprobs(want_top)
    if hasattr(engine, "set_token_entropy"):
        engine.set_token_entropy(want_ent)
    set_alignment_scores(engine, want_as, collar)
    num_frames = np.asarray(num_frames, dtype=np.int64)
    if native is None:
        native = hasattr(engine, "transcribe") and num_beams == 1
    if num_beams > 1:
        native = False                                  # the seek loop runs here, beam bookkeeping in beam_search()
    if native:
        toks, detect = resolve_prompt(spec, language, task)
        if detect and not spec.lang_to_id:
            raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
        if len(toks) < 2 or len(toks) > 3:
            raise ValueError(f"unsupported decoder prompt {toks}: the native path decodes from "
                             "<|startoftranscript|><|lang|>[<|task|>]")
        lang_tok = -1 if detect else int(toks[1])
        task_tok = int(toks[2]) if len(toks) > 2 else -1
        toks, tts, n_calls = engine.transcribe(
            n_items, num_frames, sot=spec.decoder_start_token_id, language_token=lang_tok, task_token=task_tok,
            max_new_tokens=-1 if max_new_tokens is None else int(max_new_tokens), min_new_tokens=min_new_tokens or 0,
            max_length=spec.max_length,
            lang_ids=cand_ids if cand_ids is not None else (sorted(set(spec.lang_to_id.values())) if spec.lang_to_id else None),
            prefix=prefix)
        if stats is not None:
            stats["generate_calls"] = stats.get("generate_calls", 0) + n_calls
        width = max((len(s) for s in toks), default=0)
        sequences = np.full((n_items, width), spec.pad_token_id, dtype=np.int64)
        for i, s in enumerate(toks):
            sequences[i, :len(s)] = s
        out = {"sequences": sequences, "token_timestamps": tts, "segments": None}
        if hasattr(engine, "transcribe_languages"):
            ltok, lprob = engine.transcribe_languages(n_items)
        else:                                   # an engine double without the getter: only a forced language is known here
            ltok, lprob = np.full(n_items, lang_tok), np.full(n_items, np.nan)
        out["languages"], out["language_probs"] = np.asarray(ltok, np.int64), np.asarray(lprob, np.float32)
        if want_lp:
            out["token_logprobs"] = engine.transcribe_token_logprobs([len(s) for s in toks])
        if want_top:
            out["top_ids"], out["top_logprobs"] = engine.transcribe_top_logprobs([len(s) for s in toks])
        if want_as:
            out["alignment_scores"], out["alignment_spreads"] = engine.transcribe_alignment_scores([len(s) for s in toks])
        if want_ent:
            out["token_entropy"] = engine.transcribe_token_entropy([len(s) for s in toks])
        return out
    pre_encoded = False
    _, detect = resolve_prompt(spec, language, task)
    if detect:
        # language auto-detection (the reference does not pass `language`, REF/transcribe.py:33)
        engine.encode(list(range(n_items)), np.zeros(n_items, np.int64), np.full(n_items, N_FRAMES, np.int64))
        langs, lang_probs = detect_language_probs(engine, n_items, cand_ids)
        init = np.asarray([init_tokens(spec, language, task, lang_id=l, prompt_ids=prefix) for l in langs], dtype=np.int32)
        pre_encoded = True
    else:
        toks = resolve_prompt(spec, language, task)[0]
        forced_lang = int(toks[1]) if len(toks) > 1 and toks[1] in set(spec.lang_to_id.values()) else -1
        langs, lang_probs = np.full(n_items, forced_lang, np.int64), np.full(n_items, np.nan, np.float32)
        init = np.tile(np.asarray(init_tokens(spec, language, task, prompt_ids=prefix), dtype=np.int32), (n_items, 1))
    n_prompt = init.shape[1]
    if prefix is not None:
        prompted_len = prompted_max_length(spec, n_prompt, max_new_tokens)
    elif max_new_tokens is not None and max_new_tokens + n_prompt > spec.max_target_positions:
        max_new_tokens = spec.max_target_positions - n_prompt     # :1937-1942
    tb = spec.timestamp_begin
    seek = np.zeros(n_items, dtype=np.int64)
    max_frames = np.full(n_items, N_FRAMES, dtype=np.int64)
    segments: List[List[Segment]] = [[] for _ in range(n_items)]
    n_calls = 0
    set_prefix = getattr(engine, "set_prompt_prefix", None)     # the device engine: lets the prompt prefill engage
    if prefix is not None and set_prefix is not None:
        set_prefix(len(prefix))
    try:
        _seek_loop(engine, spec, n_items, num_frames, init, n_prompt, max_new_tokens, min_new_tokens, num_beams, prefix,
                   prompted_len if prefix is not None else None, skip_on, logprob_threshold, no_speech_threshold, pre_encoded,
                   seek, max_frames, segments, tb, stats, fb, want_lp, want_top, want_as, want_ent)
    finally:
        if prefix is not None and set_prefix is not None:
            set_prefix(0)
    seq_list = [np.concatenate([s.tokens for s in segs]) if segs else np.zeros(0, np.int64) for segs in segments]
    width = max((len(s) for s in seq_list), default=0)
    sequences = np.full((n_items, width), spec.pad_token_id, dtype=np.int64)
    for i, s in enumerate(seq_list):
        sequences[i, :len(s)] = s
    tts = [np.concatenate([s.token_timestamps for s in segs]) if segs else np.zeros(0, np.float32) for segs in segments]
    out = {"sequences": sequences, "token_timestamps": tts, "segments": segments,
           "languages": np.asarray(langs, np.int64), "language_probs": np.asarray(lang_probs, np.float32)}
    if want_lp:
        out["token_logprobs"] = [np.concatenate([s.token_logprobs for s in segs]) if segs else np.zeros(0, np.float32)
                                 for segs in segments]
    if want_top:
        out["top_ids"] = [np.concatenate([s.top_ids for s in segs]) if segs else np.zeros((0, want_top), np.int32)
                          for segs in segments]
        out["top_logprobs"] = [np.concatenate([s.top_logprobs for s in segs]) if segs else np.zeros((0, want_top), np.float32)
                               for segs in segments]
    if want_as:
        out["alignment_scores"] = [np.concatenate([s.alignment_scores for s in segs]) if segs else np.zeros(0, np.float32)
                                   for segs in segments]
        out["alignment_spreads"] = [np.concatenate([s.alignment_spreads for s in segs]) if segs else np.zeros(0, np.float32)
                                    for segs in segments]
    if want_ent:
        out["token_entropy"] = [np.concatenate([s.token_entropy for s in segs]) if segs else np.zeros(0, np.float32)
                                for segs in segments]
    return out


def _seek_loop(engine, spec, n_items, num_frames, init, n_prompt, max_new_tokens, min_new_tokens, num_beams, prefix, prompted_len,
               skip_on, logprob_threshold, no_speech_threshold, pre_encoded, seek, max_frames, segments, tb, stats, fb=None, want_lp=False,
               want_top=0, want_as=False, want_ent=False):
    """The seek loop of the host path of ``generate`` (fills ``segments`` in place).  ``fb``: temperature fallback settings."""
    n_calls = 0
    while True:
        active = [i for i in range(n_items) if seek[i] < max_frames[i]]
        if not active:
            break
        seek_num = np.minimum(max_frames - seek, N_FRAMES)
        if not (pre_encoded and n_calls == 0):            # first pass: windows already encoded for detection
            engine.encode(active, seek[active], seek_num[active])
        if prefix is not None:
            max_length = prompted_len
        else:
            max_length = (n_prompt + max_new_tokens) if max_new_tokens is not None else min(spec.max_length, spec.max_target_positions)
        nsp = engine.no_speech_probs(len(active), spec.decoder_start_token_id) if skip_on else None
        if fb is not None:
            kept = _decode_with_fallback(engine, spec, fb, active, init[active], n_prompt, max_length, min_new_tokens or 0,
                                         (num_frames - seek)[active], seek[active], nsp, logprob_threshold, no_speech_threshold,
                                         stats)
            n_calls += 1
            for row, i in enumerate(active):
                s, ts_row, skip = kept[row][:3]
                lp_row = kept[row][3] if want_lp else None
                top_row = kept[row][4:6] if want_top else None
                as_row = kept[row][-2:] if want_as else None
                ent_row = kept[row][4 + (2 if want_top else 0)] if want_ent else None
                if skip:
                    seek[i] += seek_num[i]                        # should_skip (:879-881)
                    continue
                segs, advance = split_segments(s, ts_row, float(seek[i]) * TIME_PRECISION / INPUT_STRIDE, tb,
                                               int(seek_num[i]), n_prompt, lp_row, top_row, as_row, ent_row)
                seek[i] += advance
                segments[i].extend(segs)
            continue
        if num_beams > 1:
            bs, _, L, alp, *btl = beam_search(engine, init[active], max_length, min_new_tokens or 0, num_beams,
                                              return_token_logprobs=want_lp)
            total = bs.shape[1]
            if want_lp:                                           # indexed by sequence position, like token_ts
                tok_lp = np.full((len(active), total), np.nan, np.float32)
                tok_lp[:, n_prompt:] = btl[0]
            seqs = np.full((len(active), spec.max_target_positions), spec.pad_token_id, dtype=np.int64)
            seqs[:, :total] = bs
        else:
            seqs, lens, _ = engine.decode(init[active], max_length, min_new_tokens or 0)
            total = int(lens.max())
            L = total - 1
            alp = engine.avg_logprobs(len(active)) if skip_on else None
            if want_lp:
                tok_lp = engine.token_logprobs(len(active))
            if want_top:
                tok_top = engine.top_logprobs(len(active))
            if want_ent:
                tok_ent = engine.token_entropy(len(active))
        token_ts = engine.token_timestamps(len(active), L, n_prompt, (num_frames - seek)[active])
        if want_as:
            tok_as = engine.alignment_scores(len(active), L)
        n_calls += 1
        for row, i in enumerate(active):
            if skip_on and float(alp[row]) < logprob_threshold and float(nsp[row]) > no_speech_threshold:
                seek[i] += seek_num[i]                            # should_skip (:879-881)
                continue
            s = seqs[row, n_prompt:total].astype(np.int64)
            if s[-1] == spec.pad_token_id:                        # strip right padding, keep one eos
                npad = int((s == spec.pad_token_id).sum())
                if spec.pad_token_id == spec.eos_token_id:
                    npad -= 1
                if npad:
                    s = s[:-npad]
            if s[-1] == spec.eos_token_id:
                s = s[:-1]
            segs, advance = split_segments(s, token_ts[row], float(seek[i]) * TIME_PRECISION / INPUT_STRIDE, tb,
                                           int(seek_num[i]), n_prompt, tok_lp[row] if want_lp else None,
                                           (tok_top[0][row], tok_top[1][row]) if want_top else None,
                                           (tok_as[0][row], tok_as[1][row]) if want_as else None,
                                           tok_ent[row] if want_ent else None)
            seek[i] += advance
            segments[i].extend(segs)
    if stats is not None:
        stats["generate_calls"] = stats.get("generate_calls", 0) + n_calls


def _decode_with_fallback(engine, spec, fb, active, init_rows, n_prompt, max_length, min_new_tokens, frames, seeks, nsp,
                          logprob_threshold, no_speech_threshold, stats):
    """``generate_with_fallback`` (generation_whisper.py:970-1116) over the encoded windows ``active`` (engine rows 0 .. nb-1).

    One decode per temperature; from the second on only the rows still in the fallback set are live (``row_active``), the others
    idle through the step.  A row is settled by the first decode that needs no fallback, by a no-speech skip, or by the last
    temperature; its token timestamps are taken right after that decode (a later decode overwrites the idle rows' attention
    rows).  Decisions are indexed by the original row throughout -- transformers indexes ``needs_fallback[i]`` /
    ``should_skip[i]`` by the row of the shrunken sub-batch (:1074 against :1088) and reads them back by the original one.
    Returns per row (tokens without eos, token timestamps of the whole row, skip[, token log-probabilities of the whole row when
    ``fb["token_logprobs"]`` is set[, alternative ids and log-probabilities of the whole row when ``fb["top_logprobs"]`` is][, the
    token entropies of the whole row when ``fb["token_entropy"]`` is]][,
    last of all, the row's alignment scores and spreads when ``fb["alignment_scores"]`` is set])."""
    nb = len(active)
    temps = fb["temps"]
    kept = [None] * nb
    pending = list(range(nb))
    try:
        for ti, temp in enumerate(temps):
            if temp > 0.0:
                streams = [stream_id(fb["item_ids"][active[r]], int(seeks[r]), ti) for r in range(nb)]
                engine.set_sampling(temp, fb["seed"], streams)
            else:
                engine.set_sampling(0.0)
            mask = None
            if len(pending) < nb:
                mask = np.zeros(nb, np.int32)
                mask[pending] = 1
            seqs, lens, _ = engine.decode(init_rows, max_length, min_new_tokens, row_active=mask)
            total = int(lens.max())
            alp = engine.avg_logprobs(nb) if logprob_threshold is not None else None
            token_ts = engine.token_timestamps(nb, total - 1, n_prompt, frames)
            tok_as = engine.alignment_scores(nb, total - 1) if fb.get("alignment_scores") else None
            tok_lp = engine.token_logprobs(nb) if fb.get("token_logprobs") else None   # a masked row keeps its settled values
            tok_top = engine.top_logprobs(nb) if tok_lp is not None and fb.get("top_logprobs") else None   # ... and entries
            tok_ent = engine.token_entropy(nb) if tok_lp is not None and fb.get("token_entropy") else None
            again = []
            for r in pending:
                s = seqs[r, n_prompt:total].astype(np.int64)
                if s[-1] == spec.pad_token_id:                    # strip right padding, keep one eos
                    npad = int((s == spec.pad_token_id).sum())
                    if spec.pad_token_id == spec.eos_token_id:
                        npad -= 1
                    if npad:
                        s = s[:-npad]
                needs, skip, cr = need_fallback(s, spec.vocab_size, None if alp is None else alp[r], None if nsp is None else nsp[r],
                                                fb["cr_thr"], logprob_threshold, no_speech_threshold)
                last = ti == len(temps) - 1
                if stats is not None:
                    stats.setdefault("fallback", []).append({
                        "item": fb["item_ids"][active[r]], "seek": int(seeks[r]), "temperature_index": ti, "temperature": temp,
                        "compression_ratio": cr, "avg_logprob": None if alp is None else float(alp[r]),
                        "no_speech_prob": None if nsp is None else float(nsp[r]),
                        "decision": "skip" if skip else ("fallback" if needs and not last else "keep"),
                        "needs_fallback": bool(needs), "tokens": s.copy()})
                if s[-1] == spec.eos_token_id:
                    s = s[:-1]
                kept[r] = (s, np.array(token_ts[r], copy=True), skip)
                if tok_lp is not None:
                    kept[r] += (np.array(tok_lp[r], copy=True),)
                if tok_top is not None:
                    kept[r] += (np.array(tok_top[0][r], copy=True), np.array(tok_top[1][r], copy=True))
                if tok_ent is not None:
                    kept[r] += (np.array(tok_ent[r], copy=True),)
                if tok_as is not None:
                    kept[r] += (np.array(tok_as[0][r], copy=True), np.array(tok_as[1][r], copy=True))
                if needs and not last:
                    again.append(r)
            pending = again
            if not pending:
                break
    finally:
        engine.set_sampling(0.0)
    return kept


def check_transcript_ids(spec, ids) -> np.ndarray:
    """A transcript for ``align``: a 1-D integer sequence (list, numpy array or torch tensor) of text token ids, without the
    init tokens and eos; timestamp tokens, as a generation emits them, are kept.  Special tokens (eos and the tags up to
    <|notimestamps|>) and ids outside the vocabulary raise."""
    if hasattr(ids, "detach") and hasattr(ids, "cpu"):
        ids = ids.detach().cpu().numpy()
    if isinstance(ids, (str, bytes)):
        raise TypeError("a transcript here is a sequence of token ids; encode text with the tokenizer first")
    a = np.asarray(ids)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"a transcript must be a 1-D sequence of integer token ids, got shape {a.shape} dtype {a.dtype}")
    a = a.astype(np.int64)
    bad = a[(a < 0) | (a >= spec.vocab_size)]
    if bad.size:
        raise ValueError(f"token id {int(bad[0])} is outside the vocabulary (0 .. {spec.vocab_size - 1})")
    special = a[(a >= spec.eos_token_id) & (a < spec.timestamp_begin)]
    if special.size:
        raise ValueError(f"token id {int(special[0])} is a special token; a transcript holds text (and timestamp) tokens only "
                         "(the init tokens and eos are added here)")
    return a


def align(engine: Engine, n_items: int, num_frames, transcripts, *, language: Optional[str] = None,
          task: Optional[str] = None, return_scores: bool = False, return_alignment_scores: bool = False,
          alignment_collar_frames: Optional[int] = None, top_logprobs: int = 0, return_entropy: bool = False):
    """Forced alignment of known transcripts to the ``n_items`` 30 s feature windows resident in the engine.

    Row b is the decoder input <|startoftranscript|><|lang|><|task|> ++ transcripts[b] ++ eos, with the init tokens resolved by
    ``resolve_prompt`` exactly as for ``generate`` (``language=None``: detected per item).  The engine runs one teacher-forced
    forward (cw_align_tokens) and the token-timestamp stages on it.  Returns {"sequences": list of int64 arrays (the
    transcripts), "token_timestamps": list of float32 arrays, one timestamp per transcript token} -- the fields the pipeline
    hands to ``collate.decode_asr``, as ``generate`` returns them for its own tokens.  ``return_scores=True`` runs the full
    scoring forward instead of the early-stopping one (cw_align_score_tokens: same timestamps) and adds "token_logprobs",
    "top_ids", "top_logprobs": per transcript one entry per token plus one for the eos; with ``top_logprobs=k`` (1 .. 8) also
    "alt_ids" / "alt_logprobs" [n][k], the k best tokens of each of those positions (``check_score_top_logprobs``).
    ``return_alignment_scores=True`` adds "alignment_scores" and "alignment_spreads", one value per transcript token, as
    ``generate`` defines them.  ``return_entropy=True`` (needs ``return_scores=True``) adds "token_entropy": per transcript the
    predictive entropy (nats, float32) of every scored position, indexed as "token_logprobs" (``cw_set_score_entropy``)."""
    spec = engine.spec
    want_top = check_score_top_logprobs(top_logprobs)
    if want_top and not return_scores:
        raise ValueError("top_logprobs lists the alternatives next to every token's log-probability: it needs return_scores=True")
    want_ent = check_score_entropy(return_entropy, return_scores)
    want_as = bool(return_alignment_scores)
    collar = check_alignment_collar(spec, alignment_collar_frames)
    if want_as and not hasattr(engine, "set_alignment_scores"):
        raise ValueError("this engine does not implement alignment scores (cw_set_alignment_scores)")
    texts = [check_transcript_ids(spec, t) for t in transcripts]
    if len(texts) != n_items:
        raise ValueError(f"{len(texts)} transcripts for {n_items} items")
    if n_items > engine.max_batch:
        raise ValueError(f"{n_items} items exceed the engine's {engine.max_batch} rows")
    toks, detect = resolve_prompt(spec, language, task)
    if detect and not spec.lang_to_id:
        raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
    n_init = len(toks)
    for b, t in enumerate(texts):
        if n_init + len(t) + 1 > spec.max_target_positions:
            raise ValueError(f"transcript {b}: {n_init} init tokens + {len(t)} tokens + eos exceed max_target_positions "
                             f"({spec.max_target_positions})")
    num_frames = np.asarray(num_frames, dtype=np.int64)
    if detect:
        engine.encode(list(range(n_items)), np.zeros(n_items, np.int64), np.full(n_items, N_FRAMES, np.int64))
        inits = [init_tokens(spec, language, task, lang_id=l) for l in detect_language(engine, n_items)]
    else:
        inits = [init_tokens(spec, language, task)] * n_items
    rows = [np.concatenate([np.asarray(i, np.int64), t, [spec.eos_token_id]]) for i, t in zip(inits, texts)]
    set_alignment_scores(engine, want_as, collar)
    if return_scores:
        # (the argument is passed only when set: an engine without it still serves the plain call)
        ts, lp, ti, tl, *alts = engine.align_score_tokens(num_frames, rows, n_init, **({"top_logprobs": want_top} if want_top else {}),
                                                          **({"entropy": True} if want_ent else {}))
        out = {"sequences": texts, "token_timestamps": [s[n_init:n_init + len(t)] for s, t in zip(ts, texts)],
               "token_logprobs": lp, "top_ids": ti, "top_logprobs": tl}
        if want_top:
            out["alt_ids"], out["alt_logprobs"] = alts[:2]
        if want_ent:
            out["token_entropy"] = alts[-1]
    else:
        ts = engine.align_tokens(num_frames, rows, n_init)
        out = {"sequences": texts, "token_timestamps": [s[n_init:n_init + len(t)] for s, t in zip(ts, texts)]}
    if want_as:
        mass, spread = engine.alignment_scores(n_items, max(len(r) for r in rows) - 1)
        out["alignment_scores"] = [mass[b, n_init:n_init + len(t)].copy() for b, t in enumerate(texts)]
        out["alignment_spreads"] = [spread[b, n_init:n_init + len(t)].copy() for b, t in enumerate(texts)]
    return out


def check_score_entropy(return_entropy, return_scores=True) -> bool:
    """``return_entropy`` of ``score`` / ``align`` / ``align_long``: the predictive entropy of every teacher-forced position beside
    its log-probability, so it needs the scoring forward."""
    if return_entropy and not return_scores:
        raise ValueError("return_entropy gives the entropy of every position next to its log-probability: it needs return_scores=True")
    return bool(return_entropy)


def check_score_top_logprobs(k) -> int:
    """``top_logprobs`` of ``score`` / ``align`` / ``align_long``: None or an integer in 0 .. TOP_LOGPROBS_MAX -> int.  k > 0 asks
    for the k best tokens of every teacher-forced position (``Engine.score_tokens``): value descending, the lower id on an exact
    tie, over the raw logits with the normaliser of "token_logprobs"; -1 / NaN where fewer than k logits are finite."""
    if k is None:
        return 0
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= TOP_LOGPROBS_MAX:
        raise ValueError(f"top_logprobs must be an integer in 0 .. {TOP_LOGPROBS_MAX}, got {k!r}")
    return int(k)


def check_text_ids(spec, ids) -> np.ndarray:
    """A transcript for ``align_long``: ``check_transcript_ids`` without timestamp tokens.  The cut of a window is scored by the
    probability that the text stops, i.e. of eos or any timestamp token; a timestamp inside the transcript would make that
    event ambiguous, so every id >= eos raises."""
    a = check_transcript_ids(spec, ids)
    bad = a[a >= spec.eos_token_id]
    if bad.size:
        raise ValueError(f"token id {int(bad[0])} is a timestamp token; align_long takes text tokens only (ids below "
                         f"{spec.eos_token_id}): where the text stops inside a window is scored by eos and the timestamp tokens")
    return a


def align_long(engine: Engine, pcms, transcripts, collate_words, *, language: Optional[str] = None, task: Optional[str] = None,
               return_scores: bool = False, return_alignment_scores: bool = False,
               alignment_collar_frames: Optional[int] = None, max_window_tokens: Optional[int] = None,
               stats: Optional[dict] = None, item_ids=None, sampling_rate: int = 16000, top_logprobs: int = 0,
               return_entropy: bool = False):
    """Forced alignment of known transcripts to recordings of any length: the walk behind ``CrisperWhisperPipeline.align_long``.

    ``pcms``: at most ``engine.max_batch`` mono float32 recordings at ``sampling_rate``; ``transcripts``: one per recording, text
    token ids only (``check_text_ids``).  ``collate_words(tokens, token_timestamps) -> (text, words, groups)`` is the word
    collator (``collate.decode_asr(..., return_timestamps="word", return_token_groups=True)`` bound to a vocabulary).

    Per recording, with pos = 0 (tokens consumed), seek = 0 (samples) and W = the token indices at which the collator starts a
    word (one collation of the whole transcript): the window is pcm[seek : seek + 30 s], the last one iff it reaches the end
    of the recording.  It is offered T[pos : pos + L], L the largest count <= min(N - pos, cap) that ends on a word boundary
    (pos + L in W or == N; cap = ``max_window_tokens`` or max_target_positions - n_init - 1; a single word longer than cap
    raises).  One ``engine.align_cut_tokens`` call tells how many of them, cut, were spoken inside the window -- cuts are allowed
    at word boundaries, at 0 and at N; the last window is forced to take all L -- and gives the timestamps of those cut tokens
    and, from the same forward, their log-probabilities.  The kept tokens are collated on their own, seek / sampling_rate is
    added to every timestamp (rounded to 0.01 s as the collator rounds), pos += cut, and seek moves to the end of the last
    kept word floored to whole 20 ms frames, or by 30 s when cut == 0 (nothing of the text is in this window: silence,
    music); on the last window seek stays and pos grows by L > 0.  Recordings run in lockstep, one batched engine call per
    round, each at its own (seek, pos); finished ones drop out.  ``language=None`` detects once per recording, on its first
    window.

    What is not claimed: cut is the maximum-a-posteriori prefix under the model (``Engine.align_cut_tokens``).  How well that
    places the cut with a trained checkpoint is unmeasured.

    Returns per recording {"text", "chunks": [{"text", "timestamp"}]}; ``return_scores``: "logprob" per chunk and "logprob" /
    "avg_logprob" over the kept tokens and the eos (scored once, where the last token is consumed);
    ``return_alignment_scores``: "alignment_score" / "alignment_spread" per chunk.  ``top_logprobs=k`` (needs
    ``return_scores``): every chunk gains "tokens", one {"id", "logprob", "alt_ids", "alt_logprobs"} per token of its group --
    the k best tokens of that position, carried through the cut as the log-probabilities are: the kept prefix of a window
    only.  ``return_entropy=True`` (needs ``return_scores``): every chunk gains "entropy" / "entropy_max" (float64 mean and maximum
    over its group of the positions' predictive entropies, ``pipeline.add_token_entropy``), every entry of "tokens" its own
    "entropy", and the result "avg_entropy" over the kept tokens and the eos.  ``stats["align_long"]`` gains one record per (recording, window): {"item", "seek_s", "offered", "cut", "cut_score",
    "forced"}."""
    spec = engine.spec
    n_rec = len(pcms)
    want_top = check_score_top_logprobs(top_logprobs)
    if want_top and not return_scores:
        raise ValueError("top_logprobs lists the alternatives next to every token's log-probability: it needs return_scores=True")
    want_ent = check_score_entropy(return_entropy, return_scores)
    want_as = bool(return_alignment_scores)
    collar = check_alignment_collar(spec, alignment_collar_frames)
    if want_as and not hasattr(engine, "set_alignment_scores"):
        raise ValueError("this engine does not implement alignment scores (cw_set_alignment_scores)")
    if len(transcripts) != n_rec:
        raise ValueError(f"{len(transcripts)} transcripts for {n_rec} recordings")
    if n_rec > engine.max_batch:
        raise ValueError(f"{n_rec} recordings exceed the engine's {engine.max_batch} rows")
    texts = [check_text_ids(spec, t) for t in transcripts]
    toks, detect = resolve_prompt(spec, language, task)
    if detect and not spec.lang_to_id:
        raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
    n_init = len(toks)
    cap = spec.max_target_positions - n_init - 1
    if max_window_tokens is not None:
        if isinstance(max_window_tokens, (bool, np.bool_)) or not isinstance(max_window_tokens, (int, np.integer)) or \
                not 1 <= int(max_window_tokens) <= cap:
            raise ValueError(f"max_window_tokens must be an integer in 1 .. {cap} (max_target_positions - init tokens - eos), "
                             f"got {max_window_tokens!r}")
        cap = int(max_window_tokens)
    ids_of = list(range(n_rec)) if item_ids is None else list(item_ids)
    win = N.N_SAMPLES
    frame = win // N_FRAMES                                   # samples per 10 ms mel frame; a 20 ms token frame is two
    trace = stats.setdefault("align_long", []) if stats is not None else None

    class Rec:
        pass
    recs = []
    for b in range(n_rec):
        r = Rec()
        r.pcm, r.T, r.n, r.pos, r.seek, r.init, r.rounds = pcms[b], texts[b], len(texts[b]), 0, 0, None, 0
        r.chunks, r.lp, r.text, r.bounds, r.en = [], [], "", [], []
        if r.n:
            r.text, _, groups = collate_words(r.T, np.zeros(r.n, np.float32))
            starts = {int(min(g)) for g in groups if len(g)}
            r.bounds = sorted(starts | {r.n})                # where a cut may fall: word starts and the end
            first = min(b_ for b_ in r.bounds if b_ > 0)
            if first > cap:
                raise ValueError(f"transcript {b}: its first word holds {first} tokens, above the {cap} a window is offered")
            for lo, hi in zip(r.bounds, r.bounds[1:]):
                if hi - lo > cap:
                    raise ValueError(f"transcript {b}: the word at token {lo} holds {hi - lo} tokens, above the {cap} a window "
                                     "is offered")
            # every recording ends: a round consumes a token or moves seek by 30 s
            r.max_rounds = r.n + -(-len(r.pcm) // win) + 1
        recs.append(r)
    if any(r.n for r in recs):                               # (an empty transcript does not touch the engine)
        set_alignment_scores(engine, want_as, collar)
    first_round = True
    while True:
        active = [b for b in range(n_rec) if recs[b].pos < recs[b].n]
        if not active:
            break
        _, nf = engine.mel([recs[b].pcm[recs[b].seek:recs[b].seek + win] for b in active])
        nf = np.asarray(nf, dtype=np.int64)
        if first_round:
            if detect:
                engine.encode(list(range(len(active))), np.zeros(len(active), np.int64), np.full(len(active), N_FRAMES, np.int64))
                for b, l in zip(active, detect_language(engine, len(active))):
                    recs[b].init = init_tokens(spec, language, task, lang_id=l)
            else:
                for b in active:
                    recs[b].init = init_tokens(spec, language, task)
            first_round = False
        rows, masks, forced, offered = [], [], [], []
        for b in active:
            r = recs[b]
            last = r.seek + win >= len(r.pcm)
            L = max(x for x in r.bounds if r.pos < x <= r.pos + min(r.n - r.pos, cap)) - r.pos
            ok = np.zeros(L + 1, bool)
            ok[0] = True
            for x in r.bounds:
                if r.pos <= x <= r.pos + L:
                    ok[x - r.pos] = True
            rows.append(np.concatenate([np.asarray(r.init, np.int64), r.T[r.pos:r.pos + L], [spec.eos_token_id]]))
            masks.append(ok); forced.append(last); offered.append(L)
        cut, cut_score, ts, lp, _, _, _, *alts = engine.align_cut_tokens(nf, rows, n_init, masks, forced,
                                                                       **({"top_logprobs": want_top} if want_top else {}),
                                                                       **({"entropy": True} if want_ent else {}))
        if want_as:
            mass, spread = engine.alignment_scores(len(active), max(n_init + int(c) for c in cut))
        for k, b in enumerate(active):
            r = recs[b]
            c, L = int(cut[k]), offered[k]
            if not (0 <= c <= L and masks[k][c] and (not forced[k] or c == L)):
                raise RuntimeError(f"align_cut_tokens returned cut {c} for {L} offered tokens (forced: {forced[k]})")
            if trace is not None:
                trace.append({"item": ids_of[b], "seek_s": r.seek / sampling_rate, "offered": L, "cut": c,
                              "cut_score": float(cut_score[k]), "forced": bool(forced[k])})
            seek_before, pos_before = r.seek, r.pos
            if c > 0:
                kept_lp = np.asarray(lp[k][:c], np.float64)
                _, words, groups = collate_words(r.T[r.pos:r.pos + c], np.asarray(ts[k][n_init:n_init + c], np.float32))
                end = max((w["timestamp"][1] for w in words if w["timestamp"][1] is not None), default=0.0)
                if return_scores:
                    words = [{"text": w["text"], "timestamp": w["timestamp"], "logprob": float(np.sum(kept_lp[g]))}
                             for w, g in zip(words, groups)]
                if want_top:                                 # the kept prefix's rows only, as kept_lp
                    a_id, a_lp = alts[0][k][:c], alts[1][k][:c]
                    for w, g in zip(words, groups):
                        w["tokens"] = [{"id": int(r.T[r.pos + j]), "logprob": float(lp[k][j]), "alt_ids": a_id[j].copy(),
                                        "alt_logprobs": a_lp[j].copy()} for j in g]
                if want_ent:                                 # ... and so do the entropies
                    from .pipeline import add_token_entropy
                    add_token_entropy(words, groups, [alts[-1][k][:c]])
                    r.en.append(np.asarray(alts[-1][k][:c], np.float64))
                if want_as:
                    from .pipeline import add_alignment_scores
                    add_alignment_scores(words, groups, [mass[k, n_init:n_init + c]], [spread[k, n_init:n_init + c]])
                off = r.seek / sampling_rate
                for w in words:
                    w["timestamp"] = tuple(None if t is None else round(t + off, 2) for t in w["timestamp"])
                r.chunks.extend(words)
                r.lp.append(kept_lp)
                r.pos += c
                if r.pos == r.n:
                    r.lp.append(np.asarray(lp[k][c:c + 1], np.float64))      # c == L here: the eos after the whole transcript
                    if want_ent:
                        r.en.append(np.asarray(alts[-1][k][c:c + 1], np.float64))
                if not forced[k]:
                    r.seek += (int(round(end * 100)) // 2) * 2 * frame         # whole 20 ms frames, floored
            elif not forced[k]:
                r.seek += win
            r.rounds += 1
            assert r.pos > pos_before or r.seek >= seek_before + win, "align_long: a round neither consumed a token nor moved on"
            assert r.rounds <= r.max_rounds, "align_long: more rounds than tokens and windows"
    out = []
    for r in recs:
        res = {"text": r.text, "chunks": r.chunks}
        if return_scores:
            allp = np.concatenate(r.lp) if r.lp else np.zeros(0, np.float64)
            total = float(allp.sum())
            res["logprob"] = total
            res["avg_logprob"] = total / (r.n + 1)
            if want_ent:
                alle = np.concatenate(r.en) if r.en else np.zeros(0, np.float64)
                res["avg_entropy"] = float(alle.mean()) if len(alle) else float("nan")
        out.append(res)
    return out


ALIGN_HEADS_ROW_BYTES = 1500 * 4          # one recorded attention row (f32 over the encoder frames)


def check_heads(spec, heads):
    """(layer, head) pairs of ``align_heads``: None = every head of the decoder, layer-major; else distinct integer pairs inside
    the decoder's layers x heads.  Returns a list of [layer, head]."""
    if heads is None:
        return [[l, h] for l in range(spec.dec_layers) for h in range(spec.n_heads)]
    if isinstance(heads, (str, bytes)) or not hasattr(heads, "__len__") or len(heads) == 0:
        raise ValueError("heads must be None or a non-empty list of (layer, head) pairs")
    out, seen = [], set()
    for p in heads:
        if isinstance(p, (str, bytes)) or not hasattr(p, "__len__") or len(p) != 2 or any(
                isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in p):
            raise ValueError(f"heads holds {p!r}: every entry is a (layer, head) pair of integers")
        l, h = int(p[0]), int(p[1])
        if not (0 <= l < spec.dec_layers and 0 <= h < spec.n_heads):
            raise ValueError(f"head ({l}, {h}) is outside the decoder's {spec.dec_layers} layers x {spec.n_heads} heads")
        if (l, h) in seen:
            raise ValueError(f"head ({l}, {h}) is listed twice")
        seen.add((l, h))
        out.append([l, h])
    return out


def plan_align_heads_calls(n_ids: Sequence[int], n_heads: int, max_batch: int, max_bytes: Optional[int] = None):
    """Splits the items of ``align_heads`` into engine calls of consecutive items whose capture -- items x heads x (longest
    row's ids - 1) recorded rows of 6000 bytes -- stays within ``max_bytes`` (CW_ALIGN_HEADS_MAX_BYTES) and whose item count
    within ``max_batch``.  Returns a list of lists of item indices."""
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    if max_bytes is None:
        max_bytes = N.ALIGN_HEADS_MAX_BYTES
    calls, cur, longest = [], [], 0
    for b, n in enumerate(n_ids):
        rows = int(n) - 1
        if n_heads * rows * ALIGN_HEADS_ROW_BYTES > max_bytes:
            raise ValueError(f"item {b}: {n_heads} heads x {rows} positions need {n_heads * rows * ALIGN_HEADS_ROW_BYTES} bytes of "
                             f"attention rows, above the cap of {max_bytes}; pass fewer heads per call")
        new_longest = max(longest, rows)
        if cur and (len(cur) + 1 > max_batch or (len(cur) + 1) * n_heads * new_longest * ALIGN_HEADS_ROW_BYTES > max_bytes):
            calls.append(cur)
            cur, new_longest = [], rows
        cur.append(b)
        longest = new_longest
    if cur:
        calls.append(cur)
    return calls


def align_heads(engine: Engine, n_items: int, num_frames, transcripts, heads=None, *, language: Optional[str] = None,
                task: Optional[str] = None, ref=None, clip_frames: int = 200,
                load_items: Optional[Callable[[List[int]], None]] = None):
    """``align`` for every requested decoder cross-attention head on its own (cw_align_heads): what alignment-head selection
    and an audit of the configured heads need.  ``heads``: list of (layer, head) pairs, None = every head in layer-major order.
    Init tokens and language detection as in ``align``.  ``ref``: per item a pair (begin, end) of arrays with one entry per
    transcript token, seconds (NaN: no reference) -- adds "similarity".  Items are split into calls whose capture stays under
    the engine's cap (``plan_align_heads_calls``); a call over items other than 0 .. n-1 needs ``load_items(items)`` to make them
    resident, as in ``score``.  Every argument is checked before the engine is touched.  Returns {"heads", "sequences",
    "token_timestamps": [n_heads][n_items] float32 arrays over the transcript's tokens, "similarity": likewise, with ref}."""
    spec = engine.spec
    texts = [check_transcript_ids(spec, t) for t in transcripts]
    if len(texts) != n_items:
        raise ValueError(f"{len(texts)} transcripts for {n_items} items")
    if n_items > engine.max_batch:
        raise ValueError(f"{n_items} items exceed the engine's {engine.max_batch} rows")
    hd = check_heads(spec, heads)
    toks, detect = resolve_prompt(spec, language, task)
    if detect and not spec.lang_to_id:
        raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
    n_init = len(toks)
    for b, t in enumerate(texts):
        if n_init + len(t) + 1 > spec.max_target_positions:
            raise ValueError(f"transcript {b}: {n_init} init tokens + {len(t)} tokens + eos exceed max_target_positions "
                             f"({spec.max_target_positions})")
    num_frames = np.asarray(num_frames, dtype=np.int64)
    if num_frames.shape != (n_items,):
        raise ValueError(f"num_frames holds {num_frames.shape} entries for {n_items} items")
    refs = None
    if ref is not None:
        if len(ref) != n_items:
            raise ValueError(f"ref holds {len(ref)} entries for {n_items} items")
        refs = []
        for b, r in enumerate(ref):
            if len(r) != 2:
                raise ValueError(f"ref[{b}] must be a pair (begin, end)")
            rb, re = (np.asarray(x, dtype=np.float32).reshape(-1) for x in r)
            if len(rb) != len(texts[b]) or len(re) != len(texts[b]):
                raise ValueError(f"ref[{b}] holds {len(rb)} / {len(re)} times for {len(texts[b])} transcript tokens")
            refs.append((rb, re))
    calls = plan_align_heads_calls([n_init + len(t) + 1 for t in texts], len(hd), engine.max_batch)
    if load_items is None and calls != [list(range(n_items))]:
        raise ValueError(f"align_heads: {n_items} items x {len(hd)} heads do not fit one call (the capture is capped at "
                         f"{N.ALIGN_HEADS_MAX_BYTES} bytes) and no load_items was given")
    if detect:
        engine.encode(list(range(n_items)), np.zeros(n_items, np.int64), np.full(n_items, N_FRAMES, np.int64))
        inits = [init_tokens(spec, language, task, lang_id=l) for l in detect_language(engine, n_items)]
    else:
        inits = [init_tokens(spec, language, task)] * n_items
    rows = [np.concatenate([np.asarray(i, np.int64), t, [spec.eos_token_id]]) for i, t in zip(inits, texts)]
    ts_out = [[None] * n_items for _ in hd]
    sim_out = [[None] * n_items for _ in hd] if refs is not None else None
    nan = np.float32("nan")
    resident = list(range(n_items))
    for items in calls:
        if items != resident[:len(items)]:
            load_items(items)
            resident = list(items)
        r = None
        if refs is not None:
            pad = lambda x: np.concatenate([np.full(n_init, nan, np.float32), x, [nan]])
            r = ([pad(refs[b][0]) for b in items], [pad(refs[b][1]) for b in items])
        res = engine.align_heads(num_frames[items], [rows[b] for b in items], n_init, hd, ref=r, clip_frames=clip_frames)
        ts, sim = res if refs is not None else (res, None)
        for k in range(len(hd)):
            for j, b in enumerate(items):
                ts_out[k][b] = ts[k][j][n_init:n_init + len(texts[b])]
                if sim is not None:
                    sim_out[k][b] = sim[k][j][n_init:n_init + len(texts[b])]
    if resident != list(range(n_items)) and load_items is not None:
        load_items(list(range(n_items)))
    out = {"heads": hd, "sequences": texts, "token_timestamps": ts_out}
    if sim_out is not None:
        out["similarity"] = sim_out
    return out


def plan_score_calls(n_candidates: Sequence[int], max_batch: int):
    """Groups the candidate rows of ``score`` into engine calls of equal rows_per_item: items with the same candidate count K
    share calls of up to max_batch // K items; an item with more candidates than ``max_batch`` rows is split into slices of at
    most max_batch candidates (a slice is grouped like an item of that many candidates).  Returns a list of
    (rows_per_item, [(item, first candidate), ...]) in a deterministic order; every (item, candidate) appears exactly once."""
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    by_k = {}
    for b, k in enumerate(n_candidates):
        if k < 1:
            raise ValueError(f"item {b} has no candidates")
        for c0 in range(0, k, max_batch):
            by_k.setdefault(min(max_batch, k - c0), []).append((b, c0))
    calls = []
    for k in sorted(by_k):
        per = max(1, max_batch // k)
        for i in range(0, len(by_k[k]), per):
            calls.append((k, by_k[k][i:i + per]))
    return calls


def score(engine: Engine, n_items: int, candidates, *, language: Optional[str] = None, task: Optional[str] = None,
          load_items: Optional[Callable[[List[int]], None]] = None, top_logprobs: int = 0, return_entropy: bool = False):
    """Teacher-forced log-probabilities of candidate transcripts of the ``n_items`` 30 s feature windows resident in the engine.

    ``candidates[b]`` is a list of K_b transcripts (token ids, ``check_transcript_ids``).  Row (b, k) is the decoder input
    <|startoftranscript|><|lang|><|task|> ++ candidates[b][k] ++ eos, the init tokens resolved exactly as ``align`` does
    (``language=None``: detected per item).  Calls are planned by ``plan_score_calls``.  The engine scores row r against
    resident item r // rows_per_item, so a call over a subset of the items needs them resident as items 0 .. n-1:
    ``load_items(items)`` is called before such a call (and once more with all items at the end) to make them so -- the
    pipeline passes a function that computes their features again; without it only plans whose every call covers the items
    0 .. n-1 in order run (all items with one candidate count, fitting one call).  Returns per item a list over its candidates of
    {"ids", "token_logprobs", "top_ids", "top_logprobs"}: one entry per token plus one for the eos ("top_logprobs" is the
    arg-max's log-probability).  The argument ``top_logprobs=k`` (1 .. 8, ``check_score_top_logprobs``) adds "alt_ids" /
    "alt_logprobs" [n][k]: the k best tokens of each of those positions.  ``return_entropy=True`` adds "token_entropy": the predictive
    entropy (nats, float32) of each of those positions (``cw_set_score_entropy``)."""
    spec = engine.spec
    want_top = check_score_top_logprobs(top_logprobs)
    want_ent = bool(return_entropy)
    if len(candidates) != n_items:
        raise ValueError(f"{len(candidates)} candidate lists for {n_items} items")
    if n_items > engine.max_batch:
        raise ValueError(f"{n_items} items exceed the engine's {engine.max_batch} rows")
    texts = []
    for b, cands in enumerate(candidates):
        if len(cands) == 0:
            raise ValueError(f"item {b}: empty candidate list")
        texts.append([check_transcript_ids(spec, t) for t in cands])
    toks, detect = resolve_prompt(spec, language, task)
    if detect and not spec.lang_to_id:
        raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
    n_init = len(toks)
    for b, cands in enumerate(texts):
        for k, t in enumerate(cands):
            if n_init + len(t) + 1 > spec.max_target_positions:
                raise ValueError(f"transcript {b}.{k}: {n_init} init tokens + {len(t)} tokens + eos exceed max_target_positions "
                                 f"({spec.max_target_positions})")
    if detect:
        engine.encode(list(range(n_items)), np.zeros(n_items, np.int64), np.full(n_items, N_FRAMES, np.int64))
        inits = [init_tokens(spec, language, task, lang_id=l) for l in detect_language(engine, n_items)]
    else:
        inits = [init_tokens(spec, language, task)] * n_items
    out = [[None] * len(c) for c in texts]
    resident = list(range(n_items))
    for rpi, members in plan_score_calls([len(c) for c in texts], engine.max_batch):
        items = [b for b, _ in members]
        if items != resident[:len(items)]:
            if load_items is None:
                raise ValueError("score: this call covers items %s but the resident items are %s and no load_items was given"
                                 % (items, resident))
            load_items(items)
            resident = list(items)
        rows = [np.concatenate([np.asarray(inits[b], np.int64), texts[b][c0 + j], [spec.eos_token_id]])
                for b, c0 in members for j in range(rpi)]
        lp, ti, tl, *alts = engine.score_tokens(rows, n_init, rows_per_item=rpi, **({"top_logprobs": want_top} if want_top else {}),
                                                **({"entropy": True} if want_ent else {}))
        r = 0
        for b, c0 in members:
            for j in range(rpi):
                out[b][c0 + j] = {"ids": texts[b][c0 + j], "token_logprobs": lp[r], "top_ids": ti[r], "top_logprobs": tl[r]}
                if want_top:
                    out[b][c0 + j]["alt_ids"], out[b][c0 + j]["alt_logprobs"] = alts[0][r], alts[1][r]
                if want_ent:
                    out[b][c0 + j]["token_entropy"] = alts[-1][r]
                r += 1
    if resident != list(range(n_items)) and load_items is not None:
        load_items(list(range(n_items)))
    return out
