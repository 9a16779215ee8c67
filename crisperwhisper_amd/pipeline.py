"""Drop-in call surface of ``transformers.pipeline("automatic-speech-recognition", ...)`` for the
CrisperWhisper word-timestamp path (REF/transcribe.py:21-33, REF/app.py:51-61,102).

    pipe = crisperwhisper_amd.pipeline("automatic-speech-recognition", model=model, tokenizer=tok,
                                       feature_extractor=fe, chunk_length_s=30, batch_size=16,
                                       return_timestamps="word", torch_dtype=dtype, device="cuda:0")
    result = pipe(path_or_array)     # {"text": str, "chunks": [{"text", "timestamp": (start, end)}]}

Same argument names, accepted input forms, error types and output schema as
``AutomaticSpeechRecognitionPipeline`` (TF/pipelines/automatic_speech_recognition.py:190-247, 345-481,
600-710); the device work goes through libcrisperwhisper.so.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional

import numpy as np

from . import audio, collate, dist, generation, utils
from ._native import N_SAMPLES
from .engine import Engine, ModelSpec

logger = logging.getLogger("crisperwhisper_amd")
DEFAULT_NUM_BEAMS = 5       # TF/pipelines/automatic_speech_recognition.py:160-163 (5.x pipeline default)
_warned = set()


def _warn_once(key: str, msg: str):
    if key not in _warned:
        _warned.add(key)
        logger.warning(msg)


_WARPER_NEUTRAL = {"top_k": 0, "top_p": 1.0, "min_p": 0.0, "typical_p": 1.0, "repetition_penalty": 1.0}


def _sampling_warpers(get) -> Dict[str, float]:
    """The generation_config entries besides temperature that would change what a sampling call draws from (None and the
    value that leaves the scores alone count as unset; transformers 5.15.0 defaults all of them to None)."""
    out = {}
    for k, neutral in _WARPER_NEUTRAL.items():
        v = get(k)
        if v is not None and float(v) != float(neutral):
            out[k] = float(v)
    return out


class ModelBundle:
    """Geometry + generation settings + weights (HF state_dict names -> float32 numpy)."""

    def __init__(self, spec: ModelSpec, weights: Dict[str, np.ndarray]):
        self.spec = spec
        self.weights = weights

    @staticmethod
    def check_alignment_heads(alignment_heads, dec_layers: int, n_heads: int):
        """An ``alignment_heads`` override of the loaders, validated against the geometry: a non-empty list of distinct
        (layer, head) pairs inside the decoder's layers x heads."""
        if isinstance(alignment_heads, (str, bytes)) or not hasattr(alignment_heads, "__len__") or len(alignment_heads) == 0:
            raise ValueError("alignment_heads must be a non-empty list of (layer, head) pairs")
        out = []
        for p in alignment_heads:
            if isinstance(p, (str, bytes)) or not hasattr(p, "__len__") or len(p) != 2 or any(
                    isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in p):
                raise ValueError(f"alignment_heads holds {p!r}: every entry is a (layer, head) pair of integers")
            l, h = int(p[0]), int(p[1])
            if not (0 <= l < dec_layers and 0 <= h < n_heads):
                raise ValueError(f"alignment head ({l}, {h}) is outside the decoder's {dec_layers} layers x {n_heads} heads")
            if [l, h] in out:
                raise ValueError(f"alignment head ({l}, {h}) is listed twice")
            out.append([l, h])
        return out

    @classmethod
    def from_hf(cls, model, alignment_heads=None) -> "ModelBundle":
        """``alignment_heads``: a list of (layer, head) pairs that replaces the generation config's (validated against the
        geometry) -- how a checkpoint without heads, or with heads to be re-selected, is loaded
        (``CrisperWhisperPipeline.rank_alignment_heads``).  None: the checkpoint's own, which must exist."""
        cfg, gc = model.config, model.generation_config
        if alignment_heads is not None:
            alignment_heads = cls.check_alignment_heads(alignment_heads, cfg.decoder_layers, cfg.decoder_attention_heads)
        elif not hasattr(gc, "alignment_heads"):
            raise ValueError("Model generation config has no `alignment_heads`, token-level timestamps not available. "
                             "See https://gist.github.com/hollance/42e32852f24243b748ae6bc1f985b13a on how to add this "
                             "property to the generation config.")
        if not hasattr(gc, "no_timestamps_token_id"):
            raise ValueError("The generation config is outdated: `no_timestamps_token_id` is missing.")
        spec = ModelSpec(
            d_model=cfg.d_model, n_heads=cfg.encoder_attention_heads, ffn_dim=cfg.encoder_ffn_dim,
            enc_layers=cfg.encoder_layers, dec_layers=cfg.decoder_layers, n_mels=cfg.num_mel_bins,
            vocab_size=cfg.vocab_size, max_target_positions=cfg.max_target_positions,
            median_filter_width=cfg.median_filter_width,
            alignment_heads=alignment_heads if alignment_heads is not None else [list(h) for h in gc.alignment_heads],
            eos_token_id=gc.eos_token_id if isinstance(gc.eos_token_id, int) else gc.eos_token_id[0],
            pad_token_id=gc.pad_token_id, decoder_start_token_id=gc.decoder_start_token_id,
            no_timestamps_token_id=gc.no_timestamps_token_id,
            max_initial_timestamp_index=getattr(gc, "max_initial_timestamp_index", None),
            suppress_tokens=list(gc.suppress_tokens or []), begin_suppress_tokens=list(gc.begin_suppress_tokens or []),
            lang_to_id=dict(getattr(gc, "lang_to_id", {}) or {}), task_to_id=dict(getattr(gc, "task_to_id", {}) or {}),
            max_length=gc.max_length or cfg.max_target_positions,
            forced_decoder_ids=(getattr(gc, "forced_decoder_ids", None) if getattr(gc, "forced_decoder_ids", None) is not None
                                else getattr(cfg, "forced_decoder_ids", None)),
            language=getattr(gc, "language", None), task=getattr(gc, "task", None),
            sampling_warpers=_sampling_warpers(lambda k: getattr(gc, k, None)))
        weights = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items() if k != "proj_out.weight"}
        return cls(spec, weights)

    @classmethod
    def from_pretrained(cls, path: str, alignment_heads=None) -> "ModelBundle":
        """Load a Whisper checkpoint directory without ``transformers``: ``config.json`` + ``generation_config.json``
        -> ModelSpec, ``model.safetensors`` (or the sharded ``model.safetensors.index.json``) -> weights, streamed tensor
        by tensor as float32.  Replaces ``AutoModelForSpeechSeq2Seq.from_pretrained(model_id)`` (REF/transcribe.py:14-17)
        for a local snapshot; error texts follow the reference's (``generation_whisper.py:1399-1405, 1689-1693``).
        ``alignment_heads``: as in ``from_hf``."""
        import json
        import os
        cfg = json.load(open(os.path.join(path, "config.json")))
        gpath = os.path.join(path, "generation_config.json")
        gc = json.load(open(gpath)) if os.path.exists(gpath) else {}
        if cfg.get("model_type", "whisper") != "whisper":
            raise ValueError(f"not a Whisper checkpoint: model_type={cfg.get('model_type')!r}")
        if alignment_heads is not None:
            alignment_heads = cls.check_alignment_heads(alignment_heads, cfg["decoder_layers"],
                                                        cfg.get("decoder_attention_heads", cfg["encoder_attention_heads"]))
        elif "alignment_heads" not in gc:
            raise ValueError("Model generation config has no `alignment_heads`, token-level timestamps not available. "
                             "See https://gist.github.com/hollance/42e32852f24243b748ae6bc1f985b13a on how to add this "
                             "property to the generation config.")
        if "no_timestamps_token_id" not in gc:
            raise ValueError("The generation config is outdated: `no_timestamps_token_id` is missing.")
        eos = gc.get("eos_token_id", cfg.get("eos_token_id"))
        spec = ModelSpec(
            d_model=cfg["d_model"], n_heads=cfg["encoder_attention_heads"], ffn_dim=cfg["encoder_ffn_dim"],
            enc_layers=cfg["encoder_layers"], dec_layers=cfg["decoder_layers"], n_mels=cfg["num_mel_bins"],
            vocab_size=cfg["vocab_size"], max_target_positions=cfg.get("max_target_positions", 448),
            median_filter_width=cfg.get("median_filter_width", 7),
            alignment_heads=alignment_heads if alignment_heads is not None else [list(h) for h in gc["alignment_heads"]],
            eos_token_id=eos if isinstance(eos, int) else eos[0],
            pad_token_id=gc.get("pad_token_id", cfg.get("pad_token_id")),
            decoder_start_token_id=gc.get("decoder_start_token_id", cfg.get("decoder_start_token_id")),
            no_timestamps_token_id=gc["no_timestamps_token_id"],
            max_initial_timestamp_index=gc.get("max_initial_timestamp_index"),
            suppress_tokens=list(gc.get("suppress_tokens") or []), begin_suppress_tokens=list(gc.get("begin_suppress_tokens") or []),
            lang_to_id=dict(gc.get("lang_to_id") or {}), task_to_id=dict(gc.get("task_to_id") or {}),
            max_length=gc.get("max_length") or cfg.get("max_target_positions", 448),
            forced_decoder_ids=gc.get("forced_decoder_ids") if gc.get("forced_decoder_ids") is not None else cfg.get("forced_decoder_ids"),
            language=gc.get("language"), task=gc.get("task"), sampling_warpers=_sampling_warpers(gc.get))
        return cls(spec, _SafetensorsWeights(path))


    @classmethod
    def from_ctranslate2(cls, path: str) -> "ModelBundle":
        """Load a faster-whisper / CTranslate2 model directory (``model.bin`` + ``config.json`` + ``tokenizer.json`` or
        ``vocabulary.json``; REF/README.md:186-203 distributes CrisperWhisper in this form too).  Geometry comes from the
        tensor shapes and the recorded head count, the generation settings from CTranslate2's ``config.json``
        (``alignment_heads``, ``suppress_ids``, ``suppress_ids_begin``, ``lang_ids``) and the token table; weights are
        de-fused / de-quantised to the transformers names the engine loads.  Layout restated from CTranslate2's published
        spec -- parity unpinned, see ``crisperwhisper_amd/ct2.py``."""
        import json
        import os
        from . import ct2
        from .languages import LANGUAGES
        _, var, aliases = ct2.read_model_bin(os.path.join(path, "model.bin"))
        geo = ct2.geometry(var)
        cpath = os.path.join(path, "config.json")
        cfg = json.load(open(cpath)) if os.path.exists(cpath) else {}
        if not cfg.get("alignment_heads"):
            raise ValueError("Model generation config has no `alignment_heads`, token-level timestamps not available. "
                             "See https://gist.github.com/hollance/42e32852f24243b748ae6bc1f985b13a on how to add this "
                             "property to the generation config.")
        ids = ct2.vocabulary_ids(path)
        if "<|notimestamps|>" not in ids:
            raise ValueError("The generation config is outdated: `no_timestamps_token_id` is missing.")
        lang_to_id = {f"<|{c}|>": ids[f"<|{c}|>"] for c in LANGUAGES if f"<|{c}|>" in ids}
        spec = ModelSpec(
            d_model=geo["d_model"], n_heads=geo["n_heads"], ffn_dim=geo["ffn_dim"], enc_layers=geo["enc_layers"],
            dec_layers=geo["dec_layers"], n_mels=geo["n_mels"], vocab_size=geo["vocab_size"],
            max_target_positions=geo["max_target_positions"], median_filter_width=7,
            alignment_heads=[list(h) for h in cfg["alignment_heads"]],
            eos_token_id=ids["<|endoftext|>"], pad_token_id=ids["<|endoftext|>"],
            decoder_start_token_id=ids["<|startoftranscript|>"], no_timestamps_token_id=ids["<|notimestamps|>"],
            max_initial_timestamp_index=50,
            suppress_tokens=[int(t) for t in cfg.get("suppress_ids", []) if int(t) >= 0],
            begin_suppress_tokens=[int(t) for t in cfg.get("suppress_ids_begin", []) if int(t) >= 0],
            lang_to_id=lang_to_id,
            task_to_id={k: ids[f"<|{k}|>"] for k in ("transcribe", "translate") if f"<|{k}|>" in ids},
            max_length=geo["max_target_positions"], forced_decoder_ids=None, language=None, task=None)
        return cls(spec, ct2.to_hf_state(var, aliases))


class _SafetensorsWeights(dict):
    """``items()`` streams (HF name, float32 array) out of model.safetensors / its shards; nothing is held in memory."""

    def __init__(self, path: str):
        super().__init__()
        import json
        import os
        idx = os.path.join(path, "model.safetensors.index.json")
        if os.path.exists(idx):
            files = sorted(set(json.load(open(idx))["weight_map"].values()))
        else:
            files = ["model.safetensors"]
        self.files = [os.path.join(path, f) for f in files]
        for f in self.files:
            if not os.path.exists(f):
                raise FileNotFoundError(f"{f} not found (only safetensors checkpoints are read natively)")

    def items(self):
        from safetensors import safe_open
        for fn in self.files:
            try:
                with safe_open(fn, framework="np") as f:
                    for k in f.keys():
                        if k != "proj_out.weight":
                            yield k, np.ascontiguousarray(f.get_tensor(k), dtype=np.float32)
            except TypeError:          # bfloat16 has no numpy dtype: go through torch for the cast
                with safe_open(fn, framework="pt") as f:
                    for k in f.keys():
                        if k != "proj_out.weight":
                            yield k, f.get_tensor(k).float().numpy()

    def __bool__(self):
        return True


def _dtype_name(dtype) -> str:
    if dtype is None:
        _warn_once("dtype", "no torch_dtype given: running the bf16 engine (HF would keep the checkpoint dtype)")
        return "bf16"
    s = str(dtype)
    if "float32" in s or s in ("f32", "fp32"):
        return "f32"
    if ("float16" in s and "bfloat16" not in s) or s in ("f16", "fp16", "half"):
        return "f16"       # the reference's GPU dtype (REF/transcribe.py:10): the binary16 build of the MFMA engine
    return "bf16"


def _device_index(device) -> int:
    if device is None:
        return 0
    if isinstance(device, int):
        if device < 0:
            raise ValueError("crisperwhisper_amd has no CPU path: device must be a GPU (e.g. 'cuda:0')")
        return device
    s = str(device)
    if s == "cpu":
        raise ValueError("crisperwhisper_amd has no CPU path: device must be a GPU (e.g. 'cuda:0')")
    return int(s.split(":")[1]) if ":" in s else 0


# generate_kwargs the native path implements (TF generation_whisper.py:generate); everything else raises instead of being
# dropped: a drop-in must either honour an argument or refuse it
_GENERATE_KWARGS = ("language", "task", "max_new_tokens", "min_new_tokens", "num_beams", "length_penalty", "early_stopping",
                    "do_sample", "temperature", "num_return_sequences", "prompt_ids", "assistant_model",
                    "logprob_threshold", "no_speech_threshold", "compression_ratio_threshold", "return_timestamps",
                    "sequence_bias")


def _check_generate_kwargs(gk: Dict[str, Any], default_num_beams: Optional[int] = None, spec=None,
                           sampling_seed: Optional[int] = None) -> None:
    """``default_num_beams``: the width a call without ``num_beams`` decodes with (the pipeline default): the refusals that
    depend on the beam width are then raised here, before any audio is loaded.  ``spec`` (the model's ModelSpec): the
    ``prompt_ids`` checks that need the vocabulary and the length limit run here too.  ``sampling_seed``: the seed a call that
    samples would draw with (constructor or call argument of the pipeline); None = none was named, and such a call is refused."""
    unknown = sorted(k for k in gk if k not in _GENERATE_KWARGS)
    if unknown:
        raise ValueError(f"generate_kwargs {unknown} are not implemented on the native path (implemented: "
                         f"{', '.join(_GENERATE_KWARGS)}); they would be silently ignored otherwise")
    thresholds = [k for k in ("compression_ratio_threshold", "logprob_threshold", "no_speech_threshold") if gk.get(k) is not None]
    if gk.get("do_sample"):
        raise ValueError("generate_kwargs['do_sample'] is not supported on the native path: Whisper's generate derives it from the "
                         "temperature (do_sample = temperature > 0, generation_whisper.py:1002); pass temperature=... instead")
    # do_sample = temperature > 0.0 (generation_whisper.py:1002): any positive temperature, 1.0 included, makes transformers
    # sample, with num_beams forced to 1 (:1004-1005).  Here such a call runs the seeded sampler of the engine (greedy rows only);
    # without a threshold the fallback never fires and only the first temperature of a tuple is used (:1100-1104)
    temps = generation.normalise_temperatures(gk["temperature"]) if gk.get("temperature") is not None else (0.0,)
    if not thresholds:
        temps = temps[:1]
    samples = any(t > 0.0 for t in temps)
    beams = gk.get("num_beams") if gk.get("num_beams") is not None else default_num_beams
    if samples and sampling_seed is None:
        # there is no global generator here: what is drawn is a function of the seed, so a call that samples names one.  A call
        # that only carries transformers' own arguments cannot, and is refused as before
        raise ValueError(f"generate_kwargs['temperature']={gk['temperature']!r} samples (transformers samples at every temperature "
                         "> 0, and re-decodes at the later temperatures of a tuple once a threshold is set), and the native "
                         "sampler draws from a seeded stream, not from torch's generator: name the seed, "
                         "pipeline(..., sampling_seed=0) or pipe(audio, sampling_seed=0, generate_kwargs=...)")
    if samples and beams not in (None, 1):
        raise ValueError(f"generate_kwargs['temperature']={gk['temperature']!r} samples, and sampling decodes greedy rows only "
                         f"(transformers forces num_beams = 1 there); this call decodes with {beams} beams" +
                         ("" if gk.get("num_beams") is not None else " (the pipeline default)") +
                         ": pass generate_kwargs={'num_beams': 1, ...}")
    if spec is not None and getattr(spec, "sampling_warpers", None) and samples:
        raise ValueError(f"the checkpoint's generation_config sets {sorted(spec.sampling_warpers)}: temperature is the only "
                         "sampling warper the native sampler implements")
    if gk.get("num_return_sequences") not in (None, 1):
        raise ValueError("generate_kwargs['num_return_sequences'] > 1 is not supported on the native path")
    if gk.get("assistant_model") is not None:
        raise ValueError("generate_kwargs['assistant_model'] is not supported on the native path")
    if gk.get("prompt_ids") is not None:
        if gk.get("logprob_threshold") is not None or gk.get("no_speech_threshold") is not None:
            raise ValueError("generate_kwargs['prompt_ids'] together with logprob_threshold / no_speech_threshold is not "
                             "supported on the native path: the no-speech position moves with the prompt and that combination "
                             "is not reproduced")
        if len(temps) > 1:
            raise ValueError("generate_kwargs['prompt_ids'] together with temperature fallback (a temperature tuple with "
                             "compression_ratio_threshold) is not supported on the native path")
        if spec is None:                     # ids and length are only checkable against a model's vocabulary and limits
            raise ValueError("generate_kwargs['prompt_ids'] can only be checked against a model: pass its ModelSpec")
        pids = generation.check_prompt_ids(spec, gk["prompt_ids"])
        n_init = len(generation.resolve_prompt(spec, gk.get("language"), gk.get("task"))[0])
        generation.prompted_max_length(spec, len(pids) + n_init, gk.get("max_new_tokens"))
    if gk.get("sequence_bias") is not None:
        if spec is None:
            raise ValueError("generate_kwargs['sequence_bias'] can only be checked against a model: pass its ModelSpec")
        generation.check_sequence_bias(gk["sequence_bias"], spec.vocab_size)
        if beams not in (None, 1):
            raise ValueError(f"sequence_bias is implemented for greedy and sampled decoding only and this call decodes with {beams} "
                             "beams" + ("" if gk.get("num_beams") is not None else " (the pipeline default)") +
                             ": pass generate_kwargs={'num_beams': 1, ...} -- beam search adds the bias to log_softmax(raw), "
                             "and that path is not reproduced")
    if gk.get("return_timestamps") not in (None, True, "word"):
        raise ValueError("generate_kwargs['return_timestamps'] must be left to the pipeline argument of the same name")
    if gk.get("no_speech_threshold") is not None and gk.get("logprob_threshold") is None:
        raise ValueError("no_speech_threshold needs logprob_threshold as well (generation_whisper.py:1275-1285 compares both)")
    if thresholds and beams not in (None, 1) and any(k in thresholds for k in ("logprob_threshold", "no_speech_threshold")):
        raise ValueError(f"logprob_threshold / no_speech_threshold are implemented for greedy decoding only and this call decodes "
                         f"with {beams} beams" + ("" if gk.get("num_beams") is not None else " (the pipeline default)") +
                         ": pass generate_kwargs={'num_beams': 1, ...} -- transformers scores beam hypotheses differently again "
                         "and that path is not reproduced")
    if gk.get("logprob_threshold") is not None and gk.get("temperature") is None:
        raise ValueError("logprob_threshold needs an explicit temperature (pass temperature=0.0): transformers itself fails with "
                         "a TypeError in _retrieve_avg_logprobs otherwise (generation_whisper.py:1959)")
    if len(temps) > 1 and beams not in (None, 1):
        raise ValueError(f"temperature fallback is implemented for greedy decoding only and this call decodes with {beams} beams" +
                         ("" if gk.get("num_beams") is not None else " (the pipeline default)") +
                         ": pass generate_kwargs={'num_beams': 1, ...}")
    # with one temperature a failed compression-ratio / log-probability check has nowhere to fall back to and HF keeps the
    # result (generation_whisper.py:1100-1104): the only observable effect of the thresholds is then the no-speech skip; with
    # several, generation.generate decodes the windows that fail one again at the next temperature


def _check_seed(seed) -> int:
    """``sampling_seed``: the 64-bit key of the engine's counter-based sampler (transformers has no such argument: it draws
    from torch's global generator)."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"sampling_seed must be an integer in 0 .. 2^64 - 1, not {seed!r}")
    return int(seed)


def token_text(vocab, tok: int) -> str:
    """One token as text: its bytes decoded as UTF-8 with replacement; a special token's ``<|name|>``; a timestamp token's
    ``<|seconds|>``."""
    tok = int(tok)
    b = vocab.token_bytes[tok] if 0 <= tok < len(vocab.token_bytes) else None
    if b is not None:
        return bytes(b).decode("utf-8", errors="replace")
    if tok in vocab.specials:
        return vocab.specials[tok]
    if tok >= vocab.timestamp_begin:
        return f"<|{(tok - vocab.timestamp_begin) * 0.02:.2f}|>"
    return ""


def add_alignment_scores(words, groups, token_mass, token_spread):
    """"alignment_score" and "alignment_spread" on every word of ``collate.decode_asr(..., return_token_groups=True)``: the
    float64 mean of the tokens' values (``token_mass`` / ``token_spread``: one array per window, one value per token) over the
    collator's own token group of the word -- the grouping ``scored_words`` uses, so a token the seam merge drops counts in no
    word.  NaN if any member is NaN."""
    mass = np.concatenate([np.asarray(a, np.float64) for a in token_mass]) if len(token_mass) else np.zeros(0, np.float64)
    spread = np.concatenate([np.asarray(a, np.float64) for a in token_spread]) if len(token_spread) else np.zeros(0, np.float64)
    for w, g in zip(words, groups):
        g = np.asarray(g, np.int64).reshape(-1)
        w["alignment_score"] = float(np.mean(mass[g])) if g.size else float("nan")
        w["alignment_spread"] = float(np.mean(spread[g])) if g.size else float("nan")
    return words


def scored_words(vocab, outputs, token_logprobs, warn=None, token_top=None, return_groups=False, return_language=False):
    """``collate.decode_asr(outputs, return_timestamps="word")`` with "logprob" on every word: the float64 sum of
    ``token_logprobs`` (one array per entry of ``outputs``, one value per token) over the collator's own token group of the word.
    The groups address the concatenation of all windows' tokens, so a token the seam merge drops counts in no word.

    ``token_top`` (one (ids [n_tok][k], log-probabilities [n_tok][k]) pair per entry of ``outputs``) adds "tokens" to every
    word, over the same group: ``[{"id", "text", "logprob", "top_logprobs": [{"id", "text", "logprob"}, ...]}]``, alternatives
    best first, entries with id -1 left out.  ``return_groups=True`` returns the collator's token groups as a third value;
    ``return_language=True`` adds "language" to every word (``collate.decode_asr``)."""
    if len(token_logprobs) != len(outputs) or any(len(a) != len(o["tokens"]) for a, o in zip(token_logprobs, outputs)):
        raise ValueError("scored_words: one log-probability per token of every window is required")
    if token_top is not None and (len(token_top) != len(outputs) or any(
            len(t[0]) != len(o["tokens"]) or len(t[1]) != len(o["tokens"]) for t, o in zip(token_top, outputs))):
        raise ValueError("scored_words: one row of alternatives per token of every window is required")
    text, words, groups = collate.decode_asr(vocab, outputs, time_precision=0.02, warn=warn, return_timestamps="word",
                                             return_token_groups=True, return_language=return_language)
    flat = np.concatenate([np.asarray(a, np.float64) for a in token_logprobs]) if token_logprobs else np.zeros(0, np.float64)
    for w, g in zip(words, groups):
        w["logprob"] = float(np.sum(flat[g]))
    if token_top is not None and outputs:
        k = max((np.asarray(t[0]).shape[1] for t in token_top if np.asarray(t[0]).ndim == 2), default=1)
        ids = np.concatenate([np.asarray(o["tokens"], np.int64) for o in outputs])
        tid = np.concatenate([np.asarray(t[0], np.int32).reshape(-1, k) for t in token_top])
        tlp = np.concatenate([np.asarray(t[1], np.float32).reshape(-1, k) for t in token_top])
        lp32 = np.concatenate([np.asarray(a, np.float32) for a in token_logprobs])
        for w, g in zip(words, groups):
            w["tokens"] = [{"id": int(ids[i]), "text": token_text(vocab, ids[i]), "logprob": float(lp32[i]),
                            "top_logprobs": [{"id": int(v), "text": token_text(vocab, v), "logprob": float(x)}
                                             for v, x in zip(tid[i], tlp[i]) if v >= 0]}
                           for i in np.asarray(g, np.int64).reshape(-1)]
    elif token_top is not None:
        for w in words:
            w["tokens"] = []
    if return_groups:
        return text, words, groups
    return text, words


def add_token_entropy(words, groups, token_entropy):
    """Puts "entropy" and "entropy_max" on every word: the float64 mean and the maximum of ``token_entropy`` (one array per
    window, one value per token: the predictive entropy in nats of the raw distribution of the step that wrote the token) over
    the collator's own token group of the word, so a token the seam merge drops counts in no word.  NaN if any member is NaN, or
    the group is empty.  Where a word carries "tokens" (``top_logprobs``), each entry gains its own "entropy"."""
    flat = np.concatenate([np.asarray(a, np.float64) for a in token_entropy]) if len(token_entropy) else np.zeros(0, np.float64)
    for w, g in zip(words, groups):
        g = np.asarray(g, np.int64).reshape(-1)
        h = flat[g]
        bad = (not g.size) or bool(np.isnan(h).any())
        w["entropy"] = float("nan") if bad else float(np.mean(h))
        w["entropy_max"] = float("nan") if bad else float(np.max(h))
        if "tokens" in w and len(w["tokens"]) == g.size:
            for t, x in zip(w["tokens"], h):
                t["entropy"] = float(x)
    return words


def _check_top_logprobs(k) -> int:
    if k is None:
        return 0
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= generation.TOP_LOGPROBS_MAX:
        raise ValueError(f"top_logprobs must be an integer in 0 .. {generation.TOP_LOGPROBS_MAX}, got {k!r}")
    return int(k)


def token_alternatives(vocab, token_id, alt_ids, alt_logprobs):
    """One teacher-forced position's alternatives (``score(top_logprobs=k)``): ("top_logprobs": [{"id", "text", "logprob"}, ...]
    best first, entries with id -1 left out; "rank": the index of ``token_id`` in that list, None when it is not among them)."""
    top = [{"id": int(v), "text": token_text(vocab, v), "logprob": float(x)} for v, x in zip(alt_ids, alt_logprobs) if v >= 0]
    rank = next((j for j, t in enumerate(top) if t["id"] == int(token_id)), None)
    return top, rank


class CrisperWhisperPipeline:
    def __init__(self, model, tokenizer=None, feature_extractor=None, chunk_length_s=0, stride_length_s=None,
                 batch_size=1, return_timestamps=None, torch_dtype=None, dtype=None, device=None,
                 shard: Optional[dist.Shard] = None, contexts: int = 1, cross_kv_dtype: Optional[str] = None,
                 encoder_gemm_dtype: Optional[str] = None,
                 engines: Optional[List[Engine]] = None, num_beams: Optional[int] = None,
                 sampling_seed: Optional[int] = None, return_scores: bool = False, top_logprobs: int = 0,
                 return_alignment_scores: bool = False, alignment_collar_frames: Optional[int] = None,
                 return_entropy: bool = False, **kwargs):
        """``return_entropy`` (here or per call, default False; needs ``return_scores=True``, ``return_timestamps="word"`` and
        ``num_beams=1``): every word chunk gains "entropy", the float64 mean over its tokens of the predictive entropy (nats) of
        the raw next-token distribution at the decode step that chose each token, and "entropy_max", the largest of them
        (``add_token_entropy``); with ``top_logprobs`` every entry of "tokens" gains its own "entropy".  A word written at
        log-probability -0.7 with entropy 0.7 was a choice between two tokens; the same -0.7 with entropy 5 is a model that is
        lost.  Everything else in the result is unchanged.

        ``return_alignment_scores`` (here or per call, default False; needs ``return_timestamps="word"``): every word chunk
        gains "alignment_score", the share of the alignment heads' attention that lies inside the frames the DTW path gave the
        word's tokens (1: every head looks exactly there; near 0: the path had to invent the boundary), and "alignment_spread",
        the standard deviation of that attention over the frames in seconds -- float64 means over the collator's own token groups,
        NaN where undefined.  ``alignment_collar_frames`` (here or per call): the window is widened by that many 20 ms frames on
        either side; None = ``median_filter_width // 2``, the most the median filter can move an edge.  Independent of
        ``return_scores`` / ``top_logprobs``; everything else in the result is unchanged.

        ``return_scores`` (here or per call, default False): with ``return_timestamps="word"`` every chunk gains
        "logprob", the float64 sum over its tokens of ``logits[tok] - logsumexp(logits[:vocab])`` on the raw logits of the
        decode step that chose each token -- grouped by the collator's own token groups, so tokens dropped in a seam
        overlap count in no word.

        ``top_logprobs`` (here or per call, 0 .. 8, default 0; needs ``return_scores=True``, ``return_timestamps="word"`` and
        ``num_beams=1``): every word chunk also gains "tokens", one entry per token of the word with its id, text, log-probability
        and the k most probable tokens of its decode step (``scored_words``).  Everything else in the result is unchanged.

        ``num_beams`` (construction time): the widest beam the contexts are provisioned for -- decoder rows =
        batch_size x num_beams, at most 64.  Default 5 = ``AutomaticSpeechRecognitionPipeline._default_generation_config``
        of the installed transformers (TF/pipelines/automatic_speech_recognition.py:160-163), which is what a call
        without ``generate_kwargs`` runs (REF/transcribe.py:33); pass ``generate_kwargs={"num_beams": 1}`` per call for
        the greedy decoding of the 2024 reference."""
        if isinstance(model, str):               # local checkpoint directory: no transformers object needed
            if tokenizer is None:
                tokenizer = collate.Vocabulary.from_pretrained(model)
            import os as _os
            # a faster-whisper / CTranslate2 directory (model.bin, no safetensors) is read through its own loader
            ct2_dir = _os.path.exists(_os.path.join(model, "model.bin")) and not any(
                _os.path.exists(_os.path.join(model, f)) for f in ("model.safetensors", "model.safetensors.index.json"))
            model = ModelBundle.from_ctranslate2(model) if ct2_dir else ModelBundle.from_pretrained(model)
        self.bundle = model if isinstance(model, ModelBundle) else ModelBundle.from_hf(model)
        if tokenizer is None:
            raise ValueError("a tokenizer (WhisperTokenizer or crisperwhisper_amd.collate.Vocabulary) is required")
        if isinstance(tokenizer, str):
            tokenizer = collate.Vocabulary.from_pretrained(tokenizer)
        self.vocab = tokenizer if isinstance(tokenizer, collate.Vocabulary) else collate.Vocabulary.from_hf_tokenizer(tokenizer)
        self.tokenizer = tokenizer              # align(): a str transcript needs a tokenizer with `encode`
        self.sampling_rate = getattr(feature_extractor, "sampling_rate", audio.SAMPLING_RATE)
        if feature_extractor is not None and getattr(feature_extractor, "feature_size", self.bundle.spec.n_mels) != self.bundle.spec.n_mels:
            raise ValueError("feature_extractor.feature_size does not match model.config.num_mel_bins")
        self.chunk_length_s = chunk_length_s
        self.stride_length_s = stride_length_s
        self.batch_size = int(batch_size or 1)
        self.default_num_beams = DEFAULT_NUM_BEAMS
        self.max_rows = min(64, self.batch_size * int(num_beams or DEFAULT_NUM_BEAMS))
        self.max_rows = max(self.max_rows, min(64, self.batch_size))
        self.return_timestamps = return_timestamps
        self.return_scores = bool(return_scores)
        self.top_logprobs = _check_top_logprobs(top_logprobs)
        self.return_entropy = bool(return_entropy)
        self.return_alignment_scores = bool(return_alignment_scores)
        if alignment_collar_frames is not None:
            generation.check_alignment_collar(self.bundle.spec, alignment_collar_frames)
        self.alignment_collar_frames = alignment_collar_frames
        # the key of the engine's sampler for calls with a positive temperature / temperature fallback; None: such calls must
        # name one themselves (a call without any seed is refused, it does not draw from a hidden default)
        self.sampling_seed = None if sampling_seed is None else _check_seed(sampling_seed)
        self.shard = shard or dist.Shard()
        # `contexts` > 1: independent engine contexts on the same GPU, each running its own batches from a host
        # thread -- the decode chain is latency-bound, so a second in-flight batch fills idle CUs.
        if engines:                                # already created and loaded by the caller (bench.py shares them)
            self.engines = list(engines)
            if any(e.max_batch < self.batch_size for e in self.engines):
                raise ValueError("engines were created with a smaller max_batch than batch_size")
            self.max_rows = min(e.max_batch for e in self.engines)
        else:
            self.engines = [Engine(self.bundle.spec, dtype=_dtype_name(dtype if dtype is not None else torch_dtype),
                                   max_batch=self.max_rows, device=_device_index(device), cross_kv_dtype=cross_kv_dtype,
                                   encoder_gemm_dtype=encoder_gemm_dtype)
                            for _ in range(max(1, int(contexts)))]
            for e in self.engines:
                e.load_state_dict(self.bundle.weights)
        self.engine = self.engines[0]
        utils.bind_engine(self.engine)
        self.stats: Dict[str, Any] = {}

    # -- input forms (TF/pipelines/automatic_speech_recognition.py:345-430) ------------------------
    def _load(self, inputs) -> np.ndarray:
        if isinstance(inputs, str):
            if inputs.startswith("http://") or inputs.startswith("https://"):
                raise ValueError("remote URLs are not fetched by the native pipeline; pass a local path or an array")
            inputs = audio.read_audio(inputs, self.sampling_rate, self.engine)
        elif isinstance(inputs, bytes):
            inputs = audio.decode_wav_bytes(inputs, self.sampling_rate, self.engine)
        if hasattr(inputs, "detach") and hasattr(inputs, "cpu"):       # torch.Tensor
            inputs = inputs.detach().cpu().numpy()
        if isinstance(inputs, dict):
            inputs = dict(inputs)
            inputs.pop("stride", None)
            if not ("sampling_rate" in inputs and ("raw" in inputs or "array" in inputs)):
                raise ValueError(
                    "When passing a dictionary to AutomaticSpeechRecognitionPipeline, the dict needs to contain a "
                    '"raw" key containing the numpy array or torch tensor representing the audio and a "sampling_rate" key, '
                    "containing the sampling_rate associated with that array")
            arr = inputs.pop("raw", None)
            if arr is None:
                arr = inputs.pop("array", None)
            if hasattr(arr, "detach"):
                arr = arr.detach().cpu().numpy()
            inputs = audio.resample(np.asarray(arr, dtype=np.float32), int(inputs["sampling_rate"]), self.sampling_rate, self.engine)
        if not isinstance(inputs, np.ndarray):
            raise TypeError(f"We expect a numpy ndarray or torch tensor as input, got `{type(inputs)}`")
        if inputs.ndim != 1:
            logger.warning("We expect a single channel audio input for AutomaticSpeechRecognitionPipeline, got %d. "
                           "Taking the mean of the channels for mono conversion.", inputs.ndim)
            inputs = inputs.mean(axis=0)
        return np.ascontiguousarray(inputs, dtype=np.float32)

    def __call__(self, inputs, **kwargs):
        if isinstance(inputs, (list, tuple)):
            return [self._run_one(x, **kwargs) for x in inputs]
        return self._run_one(inputs, **kwargs)

    def _run_one(self, inputs, return_timestamps=None, generate_kwargs=None, chunk_length_s=None,
                 stride_length_s=None, return_language=None, sampling_seed=None, return_scores=None, top_logprobs=None,
                 return_alignment_scores=None, alignment_collar_frames=None, language_candidates=None, return_entropy=None,
                 **unused):
        """``return_language=True``: every chunk gains "language", the full lowercase name of the language its window was
        decoded with (``LANGUAGES[code]``, as transformers gives it; None when the decoder prompt carries no language), in word
        and in segment mode and in every decoding mode.  Each window's language token -- forced or detected -- is put in front
        of the window's tokens for the collation, as the transformers pipeline does, with a placeholder in front of every
        per-token array so that they stay aligned.  Knowing the language changes word splitting for the six languages written
        without spaces (chinese, japanese, thai, lao, myanmar, cantonese), exactly as it does in transformers: their words are
        split per character.  For every other language ``text`` and every ``timestamp`` equal the call without it.

        ``language_candidates`` (a call argument, not a ``generate_kwargs`` key; only with ``language`` unset): the languages
        auto-detection may answer with during this call, e.g. ``["de", "es"]``."""
        seed = self.sampling_seed if sampling_seed is None else _check_seed(sampling_seed)
        rt = return_timestamps if return_timestamps is not None else self.return_timestamps
        scores = self.return_scores if return_scores is None else bool(return_scores)
        if scores and rt != "word":
            raise ValueError('return_scores=True gives every word its log-probability: it needs return_timestamps="word" '
                             f"(got {rt!r}; segment-level scores are not implemented)")
        align_on = getattr(self, "return_alignment_scores", False) if return_alignment_scores is None else bool(return_alignment_scores)
        if align_on and rt != "word":
            raise ValueError('return_alignment_scores=True gives every word its alignment score: it needs return_timestamps="word" '
                             f"(got {rt!r})")
        collar = getattr(self, "alignment_collar_frames", None) if alignment_collar_frames is None else alignment_collar_frames
        if collar is not None:
            collar = generation.check_alignment_collar(None, collar)
        top_k = getattr(self, "top_logprobs", 0) if top_logprobs is None else _check_top_logprobs(top_logprobs)
        if top_k and not scores:
            raise ValueError("top_logprobs lists the alternatives next to every token's log-probability: it needs "
                             'return_scores=True and return_timestamps="word"')
        ent_on = getattr(self, "return_entropy", False) if return_entropy is None else bool(return_entropy)
        if ent_on and not (scores and rt == "word"):
            raise ValueError("return_entropy gives every word the entropy of its tokens' decode steps next to their "
                             'log-probability: it needs return_scores=True and return_timestamps="word"')
        if not (rt == "word" or rt is True):
            raise ValueError("crisperwhisper_amd implements the timestamped paths: pass return_timestamps='word' "
                             "(CrisperWhisper's purpose, REF/transcribe.py:28) or True (segment-level chunks, the "
                             "setting REF/app.py:51-61 constructs its pipeline with)")
        want_lang = bool(return_language)
        gk = dict(generate_kwargs or {})
        _check_generate_kwargs(gk, self.default_num_beams, self.bundle.spec, seed)
        if language_candidates is not None:                 # refused before any audio is loaded
            generation.check_language_candidates(self.bundle.spec, language_candidates)
            if gk.get("language") is not None or not generation.resolve_prompt(self.bundle.spec, None, gk.get("task"))[1]:
                raise ValueError("language_candidates restricts language auto-detection: it cannot be combined with a language "
                                 "that is given (generate_kwargs['language'] or the generation config's own)")
        if "num_beams" not in gk:
            _warn_once("beams", f"no num_beams given: decoding with {self.default_num_beams} beams like the installed transformers "
                                "ASR pipeline default; pass generate_kwargs={'num_beams': 1} for the greedy decoding of the 2024 reference")
        num_beams = int(gk.get("num_beams", self.default_num_beams))
        if gk.get("length_penalty") not in (None, 1.0) or gk.get("early_stopping") not in (None, False):
            raise ValueError("only the default length_penalty=1.0 / early_stopping=False beam search is implemented")
        if top_k and num_beams > 1:
            raise ValueError(f"top_logprobs is implemented for greedy and sampled decoding only, this call decodes with "
                             f"{num_beams} beams: pass generate_kwargs={{'num_beams': 1}}")
        if ent_on and num_beams > 1:
            raise ValueError(f"return_entropy is implemented for greedy and sampled decoding only, this call decodes with "
                             f"{num_beams} beams: pass generate_kwargs={{'num_beams': 1}}")
        import time as _time
        t_ph = [_time.perf_counter()]                       # phase clock of this call: load | local batches | gather | collation
        pcm = self._load(inputs)
        t_ph.append(_time.perf_counter())
        cl = self.chunk_length_s if chunk_length_s is None else chunk_length_s
        sl = self.stride_length_s if stride_length_s is None else stride_length_s
        sr = self.sampling_rate
        if cl:
            if sl is None:
                sl = cl / 6
            if isinstance(sl, (int, float)):
                sl = [sl, sl]
            chunk_len = int(round(cl * sr))
            windows = audio.chunk_windows(len(pcm), chunk_len, int(round(sl[0] * sr)), int(round(sl[1] * sr)))
            if chunk_len > N_SAMPLES:
                raise ValueError("chunk_length_s must be <= 30 for Whisper")
            with_stride = True
        else:
            if len(pcm) > N_SAMPLES:
                raise ValueError("audio longer than 30 s needs chunk_length_s=30 (the reference call, REF/transcribe.py:26); "
                                 "sequential long-form decoding is not implemented on the native path")
            windows = [(0, len(pcm), (len(pcm), 0, 0), True)]
            with_stride = False

        lo, hi = dist.shard_bounds(len(windows), self.shard.world)[self.shard.rank]
        mine = list(range(lo, hi))
        fallback_trace = []                                 # one record per judged (window, temperature) decode
        def run_batch(args):
            slot, idxs = args
            eng = self.engines[slot % len(self.engines)]
            clips = [pcm[windows[i][0]: windows[i][0] + windows[i][1]] for i in idxs]
            _, nf = eng.mel(clips)
            st = {}
            out = generation.generate(
                eng, len(idxs), nf, language=gk.get("language"), task=gk.get("task"),
                max_new_tokens=gk.get("max_new_tokens"), min_new_tokens=gk.get("min_new_tokens"),
                num_beams=num_beams, stats=st, logprob_threshold=gk.get("logprob_threshold"),
                no_speech_threshold=gk.get("no_speech_threshold"), prompt_ids=gk.get("prompt_ids"),
                temperature=gk.get("temperature"), compression_ratio_threshold=gk.get("compression_ratio_threshold"),
                sampling_seed=seed or 0, item_ids=idxs, **({"return_token_logprobs": True} if scores else {}),
                **({"top_logprobs": top_k} if top_k else {}), **({"return_token_entropy": True} if ent_on else {}),
                **({"return_alignment_scores": True, "alignment_collar_frames": collar} if align_on else {}),
                **({"sequence_bias": gk["sequence_bias"]} if gk.get("sequence_bias") is not None else {}),
                **({"language_candidates": language_candidates} if language_candidates is not None else {}))
            if "fallback" in st:
                fallback_trace.extend(st["fallback"])
            rs = []
            for k, i in enumerate(idxs):
                n_tok = len(out["token_timestamps"][k])
                stride = tuple(x / sr for x in windows[i][2])
                r_tok, r_ts = out["sequences"][k][:n_tok], out["token_timestamps"][k]
                r_lp = out["token_logprobs"][k] if scores else None
                r_top = (out["top_ids"][k], out["top_logprobs"][k]) if top_k else None
                r_as = (out["alignment_scores"][k], out["alignment_spreads"][k]) if align_on else None
                r_en = out["token_entropy"][k] if ent_on else None
                if want_lang and int(out["languages"][k]) >= 0:
                    # the window's language token leads its tokens (TF/pipelines/automatic_speech_recognition.py:640-650); it
                    # belongs to no word, so the placeholder in front of every per-token array belongs to no group
                    nan1 = np.full(1, np.nan, np.float32)
                    r_tok = np.concatenate([np.asarray([out["languages"][k]], np.int64), np.asarray(r_tok, np.int64)])
                    r_ts = np.concatenate([np.zeros(1, np.float32), np.asarray(r_ts, np.float32)])
                    if scores:
                        r_lp = np.concatenate([nan1, np.asarray(r_lp, np.float32)])
                    if top_k:
                        r_top = (np.concatenate([np.full((1, top_k), -1, np.int32), np.asarray(r_top[0], np.int32).reshape(-1, top_k)]),
                                 np.concatenate([np.full((1, top_k), np.nan, np.float32), np.asarray(r_top[1], np.float32).reshape(-1, top_k)]))
                    if align_on:
                        r_as = (np.concatenate([nan1, np.asarray(r_as[0], np.float32)]), np.concatenate([nan1, np.asarray(r_as[1], np.float32)]))
                    if ent_on:
                        r_en = np.concatenate([nan1, np.asarray(r_en, np.float32)])
                rs.append(dist.pack_record(i, r_tok, r_ts, stride, r_lp, r_top))
                if align_on:                               # the alignment scores travel behind the record, whatever its width
                    rs[-1] = dist.append_alignment(rs[-1], r_as[0], r_as[1])
                if ent_on:                                 # ... and the token entropies behind that
                    rs[-1] = dist.append_entropy(rs[-1], r_en)
            return rs, st.get("generate_calls", 0)

        per = self.batch_size
        if num_beams > 1:
            if num_beams > self.max_rows:
                raise ValueError(f"num_beams={num_beams} exceeds the {self.max_rows} decoder rows this pipeline was provisioned "
                                 "with (constructor argument num_beams / batch_size)")
            per = max(1, min(self.batch_size, self.max_rows // num_beams))
            if per < self.batch_size:
                _warn_once("rows", f"batch_size {self.batch_size} x {num_beams} beams exceeds {self.max_rows} decoder rows: "
                                   f"generating {per} chunks at a time")
        batches = [(n, mine[b0:b0 + per]) for n, b0 in enumerate(range(0, len(mine), per))]
        if len(self.engines) > 1 and len(batches) > 1:
            import concurrent.futures as cf
            # one worker per context; batch n always runs on context n % C, so a context is never re-entered
            lanes = [[b for b in batches if b[0] % len(self.engines) == c] for c in range(len(self.engines))]
            with cf.ThreadPoolExecutor(len(self.engines)) as ex:
                lane_out = list(ex.map(lambda lane: [run_batch(b) for b in lane], lanes))
            done = {b[0]: r for lane, outs in zip(lanes, lane_out) for b, r in zip(lane, outs)}
            results = [done[n] for n, _ in batches]
        else:
            results = [run_batch(b) for b in batches]
        recs = [r for rs, _ in results for r in rs]
        self.stats["fallback"] = sorted(fallback_trace, key=lambda d: (d["item"], d["seek"], d["temperature_index"]))
        self.stats["generate_calls"] = self.stats.get("generate_calls", 0) + sum(c for _, c in results)
        # an empty shard sends the width the other ranks send
        width = dist.rec_words_top(top_k) if top_k else (dist.REC_WORDS_SCORED if scores else dist.REC_WORDS)
        if align_on:
            width += dist.REC_ALIGN_WORDS
        if ent_on:
            width += dist.REC_ENTROPY_WORDS
        recs = np.stack(recs) if recs else np.zeros((0, width), np.int32)
        max_per_rank = max(h - l for l, h in dist.shard_bounds(len(windows), self.shard.world))
        t_ph.append(_time.perf_counter())
        allr = self.shard.all_gather_records(recs, max_per_rank)
        t_ph.append(_time.perf_counter())
        outputs, token_lp, token_top, token_mass, token_spread, token_ent = [], [], [], [], [], []
        for r in allr:
            if ent_on:
                r, ent = dist.split_entropy(r)
                token_ent.append(ent)
            if align_on:
                r, mass, spread = dist.split_alignment(r)
                token_mass.append(mass)
                token_spread.append(spread)
            _, toks, ts, stride, *lp = dist.unpack_record(r)
            if top_k:
                token_top.append((lp[1], lp[2]))
                lp = lp[:1]
            o = {"tokens": toks, "token_timestamps": ts}
            if with_stride:
                o["stride"] = stride
            outputs.append(o)
            token_lp.extend(lp)
        if scores:
            text, words, groups = scored_words(self.vocab, outputs, token_lp, warn=logger.warning,
                                               token_top=token_top if top_k else None, return_groups=True,
                                               return_language=want_lang)
        elif align_on:
            text, words, groups = collate.decode_asr(self.vocab, outputs, time_precision=0.02, warn=logger.warning,
                                                     return_timestamps="word", return_token_groups=True, return_language=want_lang)
        else:
            text, words = collate.decode_asr(self.vocab, outputs, time_precision=0.02, warn=logger.warning,
                                             return_timestamps="word" if rt == "word" else True, return_language=want_lang)
        if align_on:
            add_alignment_scores(words, groups, token_mass, token_spread)
        if ent_on:
            add_token_entropy(words, groups, token_ent)
        t_ph.append(_time.perf_counter())
        # where the wall time of the last call went on this rank (bench.py's long-form leg prints it: the scaling model of
        # DESIGN.md section 5 needs the rank-local part, which shrinks with the rank count, apart from the rest, which does not)
        self.stats["last_call_phase_s"] = {"load": t_ph[1] - t_ph[0], "local_batches": t_ph[2] - t_ph[1], "gather": t_ph[3] - t_ph[2],
                                           "collate_all_chunks": t_ph[4] - t_ph[3], "local_chunks": len(mine), "all_chunks": len(windows)}
        return {"text": text, "chunks": words}


    def detect_language(self, inputs, candidates=None):
        """Which language is this, how sure is the model, and is there speech at all -- without transcribing.  ``inputs`` in
        any form ``__call__`` takes (one, or a list); ``candidates``: the languages to choose among, in any form
        ``generate_kwargs["language"]`` accepts (None: every language of the generation config).  The audio is cut into
        consecutive non-overlapping 30 s windows, batched by ``batch_size``; a batch is one encoder pass, one decoder step on
        <|startoftranscript|> and one kernel on the logits where they lie (``Engine.detect_language``).  Per input
        {"language": "german", "code": "de", "token_id", "probability", "no_speech_prob", "probabilities": {code: p},
        "windows": [{"timestamp": (t0, t1), the same fields}]}: ``probabilities`` is the softmax over the candidates alone
        (Whisper's own detect_language), ``no_speech_prob`` the probability of <|nospeech|> over the whole vocabulary.  With
        more than one window the top-level vector is the float64 mean of the windows' vectors (the language its arg-max, the
        lower token id on a tie) and ``no_speech_prob`` their mean; with one window the top level is that window.  Runs on this
        rank's engine; it is not sharded."""
        from ._native import N_FRAMES
        from .languages import LANGUAGES
        spec = self.bundle.spec
        ids = generation.check_language_candidates(spec, candidates)
        if ids is None:
            if not spec.lang_to_id:
                raise ValueError("Cannot detect language for an English-only checkpoint: the generation config has no `lang_to_id`.")
            ids = sorted(set(spec.lang_to_id.values()))
        if len(ids) > generation.LANG_IDS_MAX:
            raise ValueError(f"{len(ids)} candidate languages; the kernel takes at most {generation.LANG_IDS_MAX}")
        code_of = {int(t): tag[2:-2] for tag, t in spec.lang_to_id.items()}
        codes = [code_of[t] for t in ids]
        single = not isinstance(inputs, (list, tuple))
        pcms = [self._load(x) for x in ([inputs] if single else inputs)]
        sr = self.sampling_rate
        wins = [(k, s0) for k, pcm in enumerate(pcms) for s0 in range(0, max(len(pcm), 1), N_SAMPLES)]
        eng = self.engine
        per = max(1, min(self.batch_size, eng.max_batch))
        rows = []                                           # per window (best id, float64 probabilities, no-speech probability)
        for b0 in range(0, len(wins), per):
            batch = wins[b0:b0 + per]
            n = len(batch)
            eng.mel([pcms[k][s0:s0 + N_SAMPLES] for k, s0 in batch])
            eng.encode(list(range(n)), [0] * n, [N_FRAMES] * n)
            best, prob, ns = eng.detect_language(n, ids, no_speech=True)
            rows.extend((int(best[r]), prob[r].astype(np.float64), float(ns[r])) for r in range(n))

        def record(best, p, ns):
            j = ids.index(best)
            return {"language": LANGUAGES.get(codes[j], codes[j]), "code": codes[j], "token_id": int(best),
                    "probability": float(p[j]), "no_speech_prob": float(ns),
                    "probabilities": {c: float(x) for c, x in zip(codes, p)}}
        results = []
        for k, pcm in enumerate(pcms):
            mine = [(s0, rows[w]) for w, (kk, s0) in enumerate(wins) if kk == k]
            windows = [dict(timestamp=(s0 / sr, min(len(pcm), s0 + N_SAMPLES) / sr), **record(*r)) for s0, r in mine]
            if len(mine) == 1:
                top = record(*mine[0][1])
            else:
                p = np.mean(np.stack([r[1] for _, r in mine]), axis=0)
                j = int(np.argmax(np.where(np.isnan(p), -np.inf, p)))
                top = record(ids[j], p, float(np.mean([r[2] for _, r in mine])))
            top["windows"] = windows
            results.append(top)
        return results[0] if single else results

    def phrase_bias(self, phrases) -> list:
        """A ``sequence_bias`` list for ``generate_kwargs`` from ``{phrase: bias}``: for every phrase its token sequence as the
        tokenizer encodes it with and without a leading space (a word inside a sentence and one at the start of a segment are
        different tokens), each with the phrase's bias.  Needs a tokenizer with ``encode``, like a text transcript of ``align``.
        Nothing is applied implicitly: pass the result as ``generate_kwargs={"num_beams": 1, "sequence_bias": ...}``."""
        if not isinstance(phrases, dict) or not phrases:
            raise ValueError("phrase_bias takes a non-empty dict {phrase: bias}")
        table = {}
        for phrase, bias in phrases.items():
            if not isinstance(phrase, str) or not phrase.strip():
                raise ValueError(f"phrase_bias: a phrase is a non-empty str, got {phrase!r}")
            if isinstance(bias, bool) or not isinstance(bias, (int, float)) or not np.isfinite(bias):
                raise ValueError(f"phrase_bias: the bias of {phrase!r} has to be a finite number, got {bias!r}")
            for text in (phrase.strip(), " " + phrase.strip()):
                ids = tuple(int(t) for t in self._transcript_ids(text))
                if ids:
                    table[ids] = float(bias)
        out = [[list(ids), b] for ids, b in table.items()]
        generation.check_sequence_bias(out, self.bundle.spec.vocab_size)
        return out

    # -- forced alignment of known transcripts ------------------------------------------------------
    def _transcript_ids(self, transcript) -> np.ndarray:
        if isinstance(transcript, str):
            enc = getattr(self.tokenizer, "encode", None)
            if enc is None or isinstance(self.tokenizer, collate.Vocabulary):
                raise ValueError("a text transcript needs a tokenizer with `encode` (a transformers WhisperTokenizer); this "
                                 "pipeline's Vocabulary has no BPE merges: pass the transcript as token ids")
            return generation.check_transcript_ids(self.bundle.spec, enc(transcript, add_special_tokens=False))
        return generation.check_transcript_ids(self.bundle.spec, transcript)

    def _forced_kwargs(self, who, language, task, kwargs):
        gk = dict(kwargs.pop("generate_kwargs", None) or {})
        if "sequence_bias" in kwargs or "sequence_bias" in gk:
            raise ValueError(f"sequence_bias is not accepted by {who}: it reports the model's raw scores of a given transcript, "
                             "nothing is chosen that a bias could steer")
        if "prompt_ids" in kwargs or "prompt_ids" in gk:
            raise ValueError(f"prompt_ids is not accepted by {who}: the decoder input is the init tokens and the transcript")
        if kwargs:
            raise TypeError(f"{who}() got unexpected keyword arguments {sorted(kwargs)}")
        unknown = set(gk) - {"language", "task"}
        if unknown:
            raise ValueError(f"{who}() takes only language / task generate_kwargs, got {sorted(unknown)}")
        return (language if language is not None else gk.get("language")), (task if task is not None else gk.get("task"))

    def _load_clips(self, who, inputs):
        pcms = []
        for k, x in enumerate(inputs):
            pcm = self._load(x)
            if len(pcm) > N_SAMPLES:
                raise ValueError(f"input {k} is {len(pcm) / self.sampling_rate:.2f} s long: {who} takes at most 30 s "
                                 f"({N_SAMPLES} samples) per input; "
                                 + ("long-form scoring is not implemented" if who == "score" else
                                    "long-form alignment is not implemented here: align_long walks a transcript over longer audio"))
            pcms.append(pcm)
        return pcms

    @staticmethod
    def _check_align_top(who, top_logprobs, return_scores):
        """``top_logprobs`` of ``align`` / ``align_long``, checked before anything is loaded."""
        top_k = _check_top_logprobs(top_logprobs)
        if top_k and not return_scores:
            raise ValueError(f"{who}: top_logprobs lists the alternatives next to every token's log-probability: it needs "
                             "return_scores=True")
        return top_k

    def _alt_tokens(self, ids, token_logprobs, alt_ids, alt_logprobs, group):
        """"tokens" of one chunk: the tokens of ``group`` with their log-probability, alternatives and rank."""
        toks = []
        for i in np.asarray(group, np.int64).reshape(-1):
            top, rank = token_alternatives(self.vocab, ids[i], alt_ids[i], alt_logprobs[i])
            toks.append({"id": int(ids[i]), "text": token_text(self.vocab, ids[i]),
                         "logprob": float(np.float32(token_logprobs[i])), "top_logprobs": top, "rank": rank})
        return toks

    def _scored_words(self, ids, token_logprobs, token_timestamps=None, return_groups=False):
        """Words of one transcript with the sum of their tokens' log-probabilities, grouped by the collator itself
        (``return_groups=True``: its token groups as a third value)."""
        ts = token_timestamps if token_timestamps is not None else np.zeros(len(ids), np.float32)
        text, words, groups = collate.decode_asr(self.vocab, [{"tokens": ids, "token_timestamps": ts}], time_precision=0.02,
                                                 return_timestamps="word", return_token_groups=True)
        chunks = []
        for w, g in zip(words, groups):
            c = {"text": w["text"], "logprob": float(np.sum(np.asarray(token_logprobs, np.float64)[g]))}
            if token_timestamps is not None:
                c["timestamp"] = w["timestamp"]
            chunks.append(c)
        if return_groups:
            return text, chunks, groups
        return text, chunks

    @staticmethod
    def _candidate_list(t):
        """transcripts[b] of ``score``: (list of candidates, whether it was given as a list).  A str, or a sequence whose
        elements are integers, is one transcript; a list / tuple of str or of id sequences is a list of candidates."""
        if isinstance(t, str):
            return [t], False
        if hasattr(t, "detach") and hasattr(t, "cpu"):
            t = t.detach().cpu().numpy()
        if isinstance(t, np.ndarray):
            if t.ndim == 1:
                return [t], False
            raise ValueError(f"a transcript must be a 1-D sequence of token ids; give candidates as a list, got shape {t.shape}")
        if not isinstance(t, (list, tuple)):
            raise TypeError(f"a transcript is a str, a sequence of token ids or a list of those, got {type(t).__name__}")
        if len(t) == 0:
            raise ValueError("empty candidate list (an empty transcript is given as one candidate: [[]])")
        is_int = [isinstance(e, (int, np.integer)) and not isinstance(e, bool) for e in t]
        if all(is_int):
            return [t], False
        if any(is_int):
            raise ValueError("a transcript mixes token ids with other elements: give either one sequence of ids or a list of candidates")
        return list(t), True

    def score(self, inputs, transcripts, language: Optional[str] = None, task: Optional[str] = None, top_logprobs=None,
              return_entropy: bool = False, **kwargs):
        """How well known transcripts fit the audio: teacher-forced log-probabilities under the model.  ``inputs`` as
        ``align`` takes them (one, or a list; each at most 30 s); ``transcripts[b]`` one transcript (``str`` or token ids) or
        a list of candidates for input b, which share one encoder pass.  Per input one dict, or a list of dicts in the order
        of the candidates: {"text", "logprob": sum over the tokens and the eos, "avg_logprob": logprob / (n_tokens + 1),
        "tokens": [{"id", "logprob", "top_id", "top_logprob"}] (the eos last), "chunks": [{"text", "logprob"}]} -- a word's
        logprob is the sum over the tokens the collator groups into it.  Raw logits: no suppress lists, no timestamp rules.
        ``top_logprobs=k`` (0 .. 8; the constructor's ``top_logprobs`` concerns ``__call__`` only): every entry of "tokens"
        gains "top_logprobs": [{"id", "text", "logprob"}, ...], the k most probable tokens of that position best first (ties
        to the lower id), and "rank": the index of the token's own id in that list, None when it is not among the k.
        ``return_entropy=True``: every entry of "tokens" gains "entropy", the predictive entropy (nats) of that position's whole
        distribution; every chunk "entropy" / "entropy_max", the float64 mean and the maximum over its tokens; the result
        "avg_entropy", the mean over the tokens and the eos (``cw_set_score_entropy``; the definition of ``__call__``'s)."""
        top_k = _check_top_logprobs(top_logprobs)
        want_ent = bool(return_entropy)
        language, task = self._forced_kwargs("score", language, task, kwargs)
        single = not isinstance(inputs, (list, tuple))
        if single:
            inputs, transcripts = [inputs], [transcripts]
        elif not isinstance(transcripts, (list, tuple)) or len(transcripts) != len(inputs):
            raise ValueError(f"{len(inputs)} inputs need a list of {len(inputs)} transcripts, got "
                             f"{len(transcripts) if isinstance(transcripts, (list, tuple)) else type(transcripts).__name__}")
        cands, listed = [], []
        for t in transcripts:
            c, l = self._candidate_list(t)
            cands.append([self._transcript_ids(x) for x in c])
            listed.append(l)
        generation.resolve_prompt(self.bundle.spec, language, task)        # refuses a bad language / task before any audio work
        pcms = self._load_clips("score", inputs)
        eng = self.engine
        per = max(1, eng.max_batch)
        eos = self.bundle.spec.eos_token_id
        results = []
        for b0 in range(0, len(pcms), per):
            idx = list(range(b0, min(len(pcms), b0 + per)))
            eng.mel([pcms[i] for i in idx])
            out = generation.score(eng, len(idx), [cands[i] for i in idx], language=language, task=task,
                                   load_items=lambda items: eng.mel([pcms[idx[j]] for j in items]),
                                   **({"top_logprobs": top_k} if top_k else {}), **({"return_entropy": True} if want_ent else {}))
            for k, i in enumerate(idx):
                rs = []
                for o in out[k]:
                    lp = np.asarray(o["token_logprobs"], np.float64)
                    text, chunks, groups = self._scored_words(o["ids"], lp[:-1], return_groups=True)
                    toks = [{"id": int(t), "logprob": float(a), "top_id": int(ti), "top_logprob": float(tl)}
                            for t, a, ti, tl in zip(list(o["ids"]) + [eos], lp, o["top_ids"], o["top_logprobs"])]
                    if top_k:
                        for t, ai, al in zip(toks, o["alt_ids"], o["alt_logprobs"]):
                            t["top_logprobs"], t["rank"] = token_alternatives(self.vocab, t["id"], ai, al)
                    total = float(lp.sum())
                    rs.append({"text": text, "logprob": total, "avg_logprob": total / (len(o["ids"]) + 1), "tokens": toks,
                               "chunks": chunks})
                    if want_ent:
                        en = np.asarray(o["token_entropy"], np.float64)
                        for t, x in zip(toks, en):
                            t["entropy"] = float(x)
                        add_token_entropy(chunks, groups, [en[:-1]])
                        rs[-1]["avg_entropy"] = float(en.mean())
                results.append(rs if listed[i] else rs[0])
        return results[0] if single else results

    def align(self, inputs, transcripts, language: Optional[str] = None, task: Optional[str] = None,
              return_scores: bool = False, return_alignment_scores: bool = False,
              alignment_collar_frames: Optional[int] = None, top_logprobs=None, return_entropy: bool = False, **kwargs):
        """Word timestamps for known transcripts: ``inputs`` in any form ``__call__`` takes (one, or a list), each at most
        30 s; ``transcripts`` one per input, a ``str`` (needs a transformers tokenizer) or token ids without special
        tokens.  ``language`` / ``task`` resolve like ``generate_kwargs`` in ``__call__`` (``language=None``: detected per
        item).  Returns {"text", "chunks": [{"text", "timestamp": (start, end)}]} like ``__call__(..., return_timestamps=
        "word")``, or a list of them for a list of inputs; lists run in batches of up to the pipeline's decoder rows.
        ``return_scores=True`` adds what ``score`` computes, from the same forward: "logprob" on every chunk, and "logprob" /
        "avg_logprob" of the whole transcript (eos included) at the top level.  ``return_alignment_scores=True`` adds
        "alignment_score" / "alignment_spread" to every chunk, as ``__call__`` defines them (``alignment_collar_frames`` likewise;
        None: the pipeline's own setting).  ``top_logprobs=k`` (0 .. 8, needs ``return_scores=True``): every chunk gains
        "tokens": [{"id", "text", "logprob", "top_logprobs", "rank"}] over the collator's own token group, as ``score`` lists
        them.  ``return_entropy=True`` (needs ``return_scores=True``): every chunk gains "entropy" / "entropy_max", every entry of
        "tokens" its own "entropy", and the result "avg_entropy", as ``score`` defines them."""
        top_k = self._check_align_top("align", top_logprobs, return_scores)
        want_ent = generation.check_score_entropy(return_entropy, return_scores)
        language, task = self._forced_kwargs("align", language, task, kwargs)
        collar = getattr(self, "alignment_collar_frames", None) if alignment_collar_frames is None else alignment_collar_frames
        if collar is not None:
            collar = generation.check_alignment_collar(None, collar)
        akw = {"return_alignment_scores": True, "alignment_collar_frames": collar} if return_alignment_scores else {}

        def with_alignment(out, k, chunks, groups):          # groups: the collator's, from the one collation of item k
            if akw:
                add_alignment_scores(chunks, groups, [out["alignment_scores"][k]], [out["alignment_spreads"][k]])
            return chunks
        single = not isinstance(inputs, (list, tuple))
        if single:
            inputs, transcripts = [inputs], [transcripts]
        elif not isinstance(transcripts, (list, tuple)) or len(transcripts) != len(inputs):
            raise ValueError(f"{len(inputs)} inputs need a list of {len(inputs)} transcripts, got "
                             f"{len(transcripts) if isinstance(transcripts, (list, tuple)) else type(transcripts).__name__}")
        ids = [self._transcript_ids(t) for t in transcripts]
        generation.resolve_prompt(self.bundle.spec, language, task)        # refuses a bad language / task before any audio work
        pcms = self._load_clips("align", inputs)
        eng = self.engine
        per = max(1, eng.max_batch)
        results = []
        for b0 in range(0, len(pcms), per):
            idx = list(range(b0, min(len(pcms), b0 + per)))
            _, nf = eng.mel([pcms[i] for i in idx])
            if return_scores:
                out = generation.align(eng, len(idx), nf, [ids[i] for i in idx], language=language, task=task, return_scores=True,
                                       **akw, **({"top_logprobs": top_k} if top_k else {}),
                                       **({"return_entropy": True} if want_ent else {}))
                for k in range(len(idx)):
                    lp = np.asarray(out["token_logprobs"][k], np.float64)
                    text, chunks, groups = self._scored_words(out["sequences"][k], lp[:-1], out["token_timestamps"][k],
                                                              return_groups=True)
                    total = float(lp.sum())
                    chunks = [{"text": c["text"], "timestamp": c["timestamp"], "logprob": c["logprob"]} for c in chunks]
                    if top_k:
                        for c, g in zip(chunks, groups):
                            c["tokens"] = self._alt_tokens(out["sequences"][k], out["token_logprobs"][k], out["alt_ids"][k],
                                                           out["alt_logprobs"][k], g)
                    results.append({"text": text, "chunks": with_alignment(out, k, chunks, groups),
                                    "logprob": total, "avg_logprob": total / (len(out["sequences"][k]) + 1)})
                    if want_ent:
                        en = np.asarray(out["token_entropy"][k], np.float64)
                        add_token_entropy(chunks, groups, [en[:-1]])
                        results[-1]["avg_entropy"] = float(en.mean())
                continue
            out = generation.align(eng, len(idx), nf, [ids[i] for i in idx], language=language, task=task, **akw)
            for k in range(len(idx)):
                text, words, *groups = collate.decode_asr(self.vocab, [{"tokens": out["sequences"][k],
                                                                        "token_timestamps": out["token_timestamps"][k]}],
                                                          time_precision=0.02, return_timestamps="word",
                                                          **({"return_token_groups": True} if akw else {}))
                results.append({"text": text, "chunks": with_alignment(out, k, words, groups[0] if akw else None)})
        return results[0] if single else results

    def align_long(self, inputs, transcripts, language: Optional[str] = None, task: Optional[str] = None,
                   return_scores: bool = False, return_alignment_scores: bool = False,
                   alignment_collar_frames: Optional[int] = None, max_window_tokens: Optional[int] = None, top_logprobs=None,
                   return_entropy: bool = False):
        """``align`` for audio of any length: walks a known transcript over the recording in 30 s windows.  ``inputs`` one
        input or a list, as ``align`` takes them but of any length; ``transcripts`` one per input, a ``str`` or text token ids
        (no timestamp tokens).  Every window is offered the transcript from the first token not yet placed, up to
        ``max_window_tokens`` (None: what fits the decoder, max_target_positions - init tokens - eos) and ending on a word
        boundary; one teacher-forced HIP forward per window tells how much of it was spoken inside the window (the cut: the
        most probable prefix under the model, scored by the probability that eos or a timestamp token follows it), aligns
        that part and scores it, and the next window starts where the last placed word ends -- or 30 s later where the window
        held none of the text.  The last window takes whatever is left.  A list of inputs runs in lockstep, one batched
        forward per round over up to the pipeline's decoder rows.  ``language=None`` detects once per input, on its first
        window.  Returns what ``align`` returns, with the same options; for audio of at most 30 s it is ``align``'s result.
        ``stats["align_long"]`` lists per (input, window) {"item", "seek_s", "offered", "cut", "cut_score", "forced"}.

        Not claimed: that the cut is right.  It is the maximum-a-posteriori prefix under the model; how well that places
        the cut with a trained checkpoint is unmeasured."""
        top_k = self._check_align_top("align_long", top_logprobs, return_scores)
        want_ent = generation.check_score_entropy(return_entropy, return_scores)
        collar = getattr(self, "alignment_collar_frames", None) if alignment_collar_frames is None else alignment_collar_frames
        if collar is not None:
            collar = generation.check_alignment_collar(None, collar)
        single = not isinstance(inputs, (list, tuple))
        if single:
            inputs, transcripts = [inputs], [transcripts]
        elif not isinstance(transcripts, (list, tuple)) or len(transcripts) != len(inputs):
            raise ValueError(f"{len(inputs)} inputs need a list of {len(inputs)} transcripts, got "
                             f"{len(transcripts) if isinstance(transcripts, (list, tuple)) else type(transcripts).__name__}")
        ids = [generation.check_text_ids(self.bundle.spec, self._transcript_ids(t)) for t in transcripts]
        generation.resolve_prompt(self.bundle.spec, language, task)        # refuses a bad language / task before any audio work
        pcms = [self._load(x) for x in inputs]
        eng = self.engine
        per = max(1, eng.max_batch)

        def collate_words(tokens, token_ts):
            return collate.decode_asr(self.vocab, [{"tokens": tokens, "token_timestamps": token_ts}], time_precision=0.02,
                                      return_timestamps="word", return_token_groups=True)
        self.stats["align_long"] = []
        results = []
        for b0 in range(0, len(pcms), per):
            idx = list(range(b0, min(len(pcms), b0 + per)))
            results.extend(generation.align_long(
                eng, [pcms[i] for i in idx], [ids[i] for i in idx], collate_words, language=language, task=task,
                return_scores=return_scores, return_alignment_scores=return_alignment_scores, alignment_collar_frames=collar,
                max_window_tokens=max_window_tokens, stats=self.stats, item_ids=idx, sampling_rate=self.sampling_rate,
                **({"top_logprobs": top_k} if top_k else {}), **({"return_entropy": True} if want_ent else {})))
        if top_k:                                            # the walk's raw rows -> what align(top_logprobs=k) lists
            for res in results:
                for c in res["chunks"]:
                    raw = c["tokens"]
                    c["tokens"] = self._alt_tokens([t["id"] for t in raw], [t["logprob"] for t in raw], [t["alt_ids"] for t in raw],
                                                   [t["alt_logprobs"] for t in raw], range(len(raw)))
                    for t, r_ in zip(c["tokens"], raw):
                        if "entropy" in r_:
                            t["entropy"] = r_["entropy"]
        return results[0] if single else results

    # -- per-head forced alignment, alignment-head selection -----------------------------------------
    def _align_heads(self, who, inputs, transcripts, heads, language, task, word_refs=None):
        """Shared by ``align_heads`` and ``rank_alignment_heads``: per input (heads, token timestamps [n_heads][n_tokens], word
        chunks per head, similarity [n_heads][n_tokens] or None).  ``word_refs``: per input [W][2] reference word intervals."""
        if not isinstance(transcripts, (list, tuple)) or len(transcripts) != len(inputs):
            raise ValueError(f"{len(inputs)} inputs need a list of {len(inputs)} transcripts, got "
                             f"{len(transcripts) if isinstance(transcripts, (list, tuple)) else type(transcripts).__name__}")
        ids = [self._transcript_ids(t) for t in transcripts]
        hd = generation.check_heads(self.bundle.spec, heads)
        generation.resolve_prompt(self.bundle.spec, language, task)        # refuses a bad language / task before any audio work
        tok_refs = None
        if word_refs is not None:
            tok_refs = []
            for k, (t, wr) in enumerate(zip(ids, word_refs)):
                _, words, groups = collate.decode_asr(self.vocab, [{"tokens": t, "token_timestamps": np.zeros(len(t), np.float32)}],
                                                      time_precision=0.02, return_timestamps="word", return_token_groups=True)
                if len(words) != len(wr):
                    raise ValueError(f"input {k}: the transcript splits into {len(words)} words ({[w['text'] for w in words]}) "
                                     f"but {len(wr)} references were given")
                rb = np.full(len(t), np.nan, np.float32)
                re = np.full(len(t), np.nan, np.float32)
                for g, (s, e) in zip(groups, wr):
                    rb[list(g)] = s
                    re[list(g)] = e
                tok_refs.append((rb, re))
        pcms = self._load_clips(who, inputs)
        eng = self.engine
        per = max(1, eng.max_batch)
        results = []
        for b0 in range(0, len(pcms), per):
            idx = list(range(b0, min(len(pcms), b0 + per)))
            _, nf = eng.mel([pcms[i] for i in idx])
            out = generation.align_heads(eng, len(idx), nf, [ids[i] for i in idx], hd, language=language, task=task,
                                         ref=[tok_refs[i] for i in idx] if tok_refs is not None else None,
                                         load_items=lambda items: eng.mel([pcms[idx[j]] for j in items]))
            for k in range(len(idx)):
                chunks = []
                for h in range(len(hd)):
                    _, words = collate.decode_asr(self.vocab, [{"tokens": out["sequences"][k],
                                                                "token_timestamps": out["token_timestamps"][h][k]}],
                                                  time_precision=0.02, return_timestamps="word")
                    chunks.append(words)
                results.append((hd, [out["token_timestamps"][h][k] for h in range(len(hd))], chunks,
                                [out["similarity"][h][k] for h in range(len(hd))] if "similarity" in out else None))
        return results

    def align_heads(self, inputs, transcripts, heads=None, language: Optional[str] = None, task: Optional[str] = None, **kwargs):
        """``align`` for every requested decoder cross-attention head on its own: which heads of this checkpoint align, and do
        the configured ones still.  ``inputs`` / ``transcripts`` as ``align`` takes them (audio at most 30 s); ``heads`` a list
        of (layer, head) pairs, None = every head of the decoder in layer-major order.  Returns per input {"heads": [[l, h],
        ...], "token_timestamps": [n_heads][n_tokens], "chunks": per head the word chunks ``align`` would return with that head
        as the only alignment head}, or a list of them for a list of inputs."""
        language, task = self._forced_kwargs("align_heads", language, task, kwargs)
        single = not isinstance(inputs, (list, tuple))
        if single:
            inputs, transcripts = [inputs], [transcripts]
        res = self._align_heads("align_heads", inputs, transcripts, heads, language, task)
        out = [{"heads": [list(h) for h in hd], "token_timestamps": [np.asarray(t) for t in ts], "chunks": chunks}
               for hd, ts, chunks, _ in res]
        return out[0] if single else out

    def rank_alignment_heads(self, inputs, transcripts, references, top: int = 15, collar: float = 0.05, heads=None,
                             language: Optional[str] = None, task: Optional[str] = None, **kwargs):
        """Alignment-head selection: every head's own forced alignment of ``transcripts`` against reference word times.
        ``references``: per input ``[{"text", "timestamp": (start, end)}, ...]``, one entry per word of the transcript as the
        collation splits it (a different word count is an error that names the input).  Returns {"ranking": per head, best
        first, {"head": [l, h], "mean_abs_error" (s, over word boundaries), "within_collar" (share of boundaries within
        ``collar`` s), "mean_iou" (word intervals), "mean_similarity" (attention rows against the words' intervals), "n_within",
        "n_boundaries"}, "alignment_heads": the ``top`` heads by share within the collar, ties by mean IoU, then similarity,
        then (layer, head) -- the list for ``generation_config.json``}.  Arithmetic: ``crisperwhisper_amd.metrics``."""
        from . import metrics
        language, task = self._forced_kwargs("rank_alignment_heads", language, task, kwargs)
        if not isinstance(inputs, (list, tuple)):
            inputs, transcripts, references = [inputs], [transcripts], [references]
        if not isinstance(references, (list, tuple)) or len(references) != len(inputs):
            raise ValueError(f"{len(inputs)} inputs need a list of {len(inputs)} reference lists")
        if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or top < 1:
            raise ValueError(f"top must be a positive integer, got {top!r}")
        if not (isinstance(collar, (int, float)) and np.isfinite(collar) and collar >= 0):
            raise ValueError(f"collar must be a non-negative number of seconds, got {collar!r}")
        word_refs = []
        for k, ref in enumerate(references):
            rows = []
            for w in ref:
                ts = w.get("timestamp") if isinstance(w, dict) else None
                if ts is None or len(ts) != 2 or not all(isinstance(x, (int, float, np.floating, np.integer)) and np.isfinite(x) for x in ts):
                    raise ValueError(f"input {k}: every reference is {{'text', 'timestamp': (start, end)}} with finite times, got {w!r}")
                rows.append((float(ts[0]), float(ts[1])))
            word_refs.append(np.asarray(rows, np.float64).reshape(-1, 2))
        res = self._align_heads("rank_alignment_heads", inputs, transcripts, heads, language, task, word_refs=word_refs)
        hd = res[0][0] if res else generation.check_heads(self.bundle.spec, heads)
        rows = []
        for h in range(len(hd)):
            pred = [np.asarray([c["timestamp"] for c in chunks[h]], np.float64).reshape(-1, 2) for _, _, chunks, _ in res]
            rows.append(metrics.head_metrics(pred, word_refs, [sim[h] for _, _, _, sim in res], collar=float(collar)))
        return metrics.rank_heads(hd, rows, top=int(top))


def pipeline(task: str = "automatic-speech-recognition", model=None, tokenizer=None, feature_extractor=None, **kwargs):
    """Factory with the signature the reference uses (REF/transcribe.py:21-31)."""
    if task != "automatic-speech-recognition":
        raise KeyError(f"Unknown task {task}, available tasks are ['automatic-speech-recognition']")
    if model is None:
        raise ValueError("a model (WhisperForConditionalGeneration or ModelBundle) is required")
    return CrisperWhisperPipeline(model, tokenizer=tokenizer, feature_extractor=feature_extractor, **kwargs)
