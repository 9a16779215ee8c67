"""Host side of temperature fallback (generation._decode_with_fallback, generation.need_fallback, the pipeline's argument
checks) without a GPU: the loop over a scripted engine, every decision against transformers' own `_need_fallback` /
`_retrieve_compression_ratio` on the same inputs, the stream-id formula, the refusals, and the numpy Philox4x32-10 of
tests/sampling_ref.py against the known-answer vectors of the Random123 distribution."""
import types

import numpy as np
import pytest

from crisperwhisper_amd import generation
from crisperwhisper_amd.pipeline import _check_generate_kwargs as chk, _check_seed, _sampling_warpers
from tests import helpers as Hh
from tests import sampling_ref as R


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


def test_philox4x32_10_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds (Salmon et al., SC 2011): counter, key -> output."""
    kat = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10(np.array([ctr], np.uint64), np.array([key], np.uint64))[0]
        assert tuple(int(x) for x in got) == want
    # vectorised over counters, and the noise is finite everywhere the uniform can land
    g = R.gumbel_noise(1000, 7, 2 ** 64 - 1, 2 ** 63 + 5)
    assert np.isfinite(g).all() and -2.86 < g.min() and g.max() < 17.4


def test_stream_ids_follow_the_formula():
    assert generation.stream_id(5, 0, 0) == 5
    assert generation.stream_id(5, 1500, 3) == (((1500 << 4) | 3) << 32) | 5
    assert generation.stream_id(2 ** 32 - 1, 3000, 15) == (((3000 << 4) | 15) << 32) | (2 ** 32 - 1)
    with pytest.raises(ValueError):
        generation.stream_id(0, 0, 16)
    with pytest.raises(ValueError):
        generation.normalise_temperatures(tuple(0.05 * i for i in range(17)))
    assert generation.normalise_temperatures(tuple(0.05 * i for i in range(16)))[15] == pytest.approx(0.75)
    assert generation.normalise_temperatures(None) == (0.0,) and generation.normalise_temperatures(0.5) == (0.5,)
    for bad in ((), -0.1, float("nan"), float("inf"), True, "0.2", (0.0, None)):
        with pytest.raises(ValueError):
            generation.normalise_temperatures(bad)


def _hf_decision(tokens, vocab_size, avg_logprob, no_speech_prob, cr_thr, lp_thr, ns_thr):
    """transformers' own _need_fallback (and through it _retrieve_compression_ratio) on the same inputs: the scores are
    replaced by a precomputed `sequences_scores`, the branch _need_fallback takes for beam outputs."""
    torch = pytest.importorskip("torch")
    GW = pytest.importorskip("transformers.models.whisper.generation_whisper")
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    proc = WhisperNoSpeechDetection.__new__(WhisperNoSpeechDetection)
    proc._no_speech_prob = [no_speech_prob]
    cfg = types.SimpleNamespace(compression_ratio_threshold=cr_thr, logprob_threshold=lp_thr, no_speech_threshold=ns_thr)

    class _O(dict):
        sequences_scores = avg_logprob
    mixin = GW.WhisperGenerationMixin
    self = types.SimpleNamespace(_retrieve_compression_ratio=mixin._retrieve_compression_ratio)
    return mixin._need_fallback(self, torch.tensor(list(tokens)), [_O(sequences_scores=avg_logprob)], 0, [proc], cfg, vocab_size, 0.0)


CASES = [  # tokens, avg_logprob, no_speech_prob
    ([270, 40, 41, 42, 43, 44, 45, 300, 256], -0.4, 0.1),
    ([270] + [40, 41] * 10 + [300, 256], -0.4, 0.1),              # a loop: compresses well
    ([270] + [40, 41] * 10 + [300, 256], -2.5, 0.9),              # ... in silence
    ([270, 50, 61, 72, 83, 94, 105, 116, 127, 300, 256], -2.5, 0.1),
    ([270, 50, 61, 72, 83, 94, 105, 116, 127, 300, 256], -2.5, 0.9),
    ([256], -0.01, 0.99),
]
THRESHOLDS = [(1.35, -1.0, 0.6), (1.35, None, None), (None, -1.0, None), (None, -1.0, 0.6), (1.05, -3.0, 0.95), (None, None, None)]


def test_need_fallback_agrees_with_transformers(tiny):
    g, v, W, spec = tiny
    seen = set()
    for tokens, lp, nsp in CASES:
        for cr_thr, lp_thr, ns_thr in THRESHOLDS:
            needs, skip, cr = generation.need_fallback(np.array(tokens), spec.vocab_size, lp, nsp, cr_thr, lp_thr, ns_thr)
            want = _hf_decision(tokens, spec.vocab_size, lp, nsp, cr_thr, lp_thr, ns_thr)
            assert (needs, skip) == tuple(bool(x) for x in want), (tokens, lp, nsp, cr_thr, lp_thr, ns_thr)
            seen.add((needs, skip))
            if cr is not None:
                GW = pytest.importorskip("transformers.models.whisper.generation_whisper")
                import torch
                assert cr == GW.WhisperGenerationMixin._retrieve_compression_ratio(torch.tensor(tokens), spec.vocab_size)
    assert seen == {(False, False), (True, False), (False, True)}


class ScriptedEngine:
    """Rows are scripted per (item, temperature index): tokens, average log-probability; no-speech probability per item."""

    def __init__(self, spec, script, nsp, max_batch=8):
        self.spec, self.script, self.nsp, self.max_batch = spec, script, nsp, max_batch
        self.calls, self.sampling, self.items = [], None, []
        self.thresholds = None

    def set_thresholds(self, lp, ns):
        self.thresholds = (lp, ns)

    def encode(self, item, seek, n_frames):
        self.items = [int(i) for i in item]
        self.calls.append(("encode", list(self.items), [int(s) for s in seek]))

    def no_speech_probs(self, nb, sot):
        return np.array([self.nsp[i] for i in self.items[:nb]], np.float32)

    def set_sampling(self, temperature=0.0, seed=0, row_streams=None):
        self.sampling = None if not temperature > 0 else (float(temperature), int(seed), [int(s) for s in row_streams])
        self.calls.append(("sampling", self.sampling))

    def decode(self, prompt, max_length, min_new_tokens=0, forced=None, want_argmax=False, row_active=None):
        nb, n_prompt = prompt.shape
        act = [1] * nb if row_active is None else [int(a) for a in row_active]
        ti = 0 if self.sampling is None else self.sampling[2][0] >> 32 & 15
        self.calls.append(("decode", ti, act))
        seqs = np.full((nb, self.spec.max_target_positions), self.spec.pad_token_id, np.int32)
        lens = np.zeros(nb, np.int32)
        self._lp = np.zeros(nb, np.float32)
        for r in range(nb):
            if not act[r]:
                continue
            toks, lp = self.script[(self.items[r], ti)]
            seqs[r, :n_prompt] = prompt[r]
            seqs[r, n_prompt:n_prompt + len(toks)] = toks
            lens[r] = n_prompt + len(toks)
            self._lp[r] = lp
        self._last = (ti, act)
        return seqs, lens, None

    def avg_logprobs(self, nb):
        return self._lp[:nb].copy()

    def token_timestamps(self, nb, L, n_prompt, num_frames):
        ti, act = self._last
        return np.full((nb, L + 1), float(ti), np.float32)         # a row's timestamps tell which decode they came from


def _generate(spec, eng, n_items, temps, thr, **kw):
    st = {}
    out = generation.generate(eng, n_items, [3000] * n_items, language="<|en|>", task="transcribe", num_beams=1, stats=st,
                              temperature=temps, compression_ratio_threshold=thr[0], logprob_threshold=thr[1],
                              no_speech_threshold=thr[2], **kw)
    return out, st


def test_fallback_loop_over_a_scripted_engine(tiny):
    g, v, W, spec = tiny
    tb, eos = spec.timestamp_begin, spec.eos_token_id
    good = [tb, 50, 61, 72, 83, 94, 105, tb + 1500, eos]            # ends the window: one pass
    loop = [tb] + [40, 41] * 10 + [tb + 1500, eos]
    script = {
        (0, 0): (good, -0.3),                                        # kept at temperature 0
        (1, 0): (loop, -0.3), (1, 1): (loop, -0.3), (1, 2): (good, -0.2),      # compression: settles at index 2
        (2, 0): (good, -2.0), (2, 1): (good, -2.0), (2, 2): (loop, -2.0),      # never passes: the last temperature is kept
        (3, 0): (loop, -2.0),                                        # silence: the no-speech skip overrides the fallback
        (4, 0): (good, -2.0), (4, 1): (good, -0.5),                  # log-probability: settles at index 1
    }
    nsp = {0: 0.1, 1: 0.1, 2: 0.1, 3: 0.9, 4: 0.1}
    eng = ScriptedEngine(spec, script, nsp)
    temps, thr = (0.0, 0.4, 0.8), (1.35, -1.0, 0.6)
    out, st = _generate(spec, eng, 5, temps, thr, sampling_seed=77, item_ids=[10, 11, 12, 13, 14])
    decodes = [c for c in eng.calls if c[0] == "decode"]
    assert decodes == [("decode", 0, [1, 1, 1, 1, 1]), ("decode", 1, [0, 1, 1, 0, 1]), ("decode", 2, [0, 1, 1, 0, 0])]
    assert sum(1 for c in eng.calls if c[0] == "encode") == 1       # a re-decode never encodes again
    # the kept tokens and the decode their timestamps came from
    strip = lambda t: [x for x in t if x != eos]
    assert out["sequences"][0][:len(good) - 1].tolist() == strip(good) and set(out["token_timestamps"][0]) == {0.0}
    assert out["sequences"][1][:len(good) - 1].tolist() == strip(good) and set(out["token_timestamps"][1]) == {2.0}
    assert out["sequences"][2][:len(loop) - 1].tolist() == strip(loop) and set(out["token_timestamps"][2]) == {2.0}
    assert len(out["token_timestamps"][3]) == 0                      # skipped: no segment
    assert out["sequences"][4][:len(good) - 1].tolist() == strip(good) and set(out["token_timestamps"][4]) == {1.0}
    # every judged decode agrees with transformers on the same quantities
    decisions = {}
    for r in st["fallback"]:
        want = _hf_decision(r["tokens"].tolist(), spec.vocab_size, r["avg_logprob"], r["no_speech_prob"], *thr)
        last = r["temperature_index"] == len(temps) - 1
        assert (r["needs_fallback"], r["decision"] == "skip") == tuple(bool(x) for x in want)
        assert r["decision"] == ("skip" if want[1] else "fallback" if want[0] and not last else "keep")
        decisions[(r["item"], r["temperature_index"])] = r["decision"]
    assert decisions == {(10, 0): "keep", (11, 0): "fallback", (11, 1): "fallback", (11, 2): "keep", (12, 0): "fallback",
                         (12, 1): "fallback", (12, 2): "keep", (13, 0): "skip", (14, 0): "fallback", (14, 1): "keep"}
    # sampling settings: greedy at temperature 0, then the seed and one stream per row from (item id, seek, temperature index)
    samp = [c[1] for c in eng.calls if c[0] == "sampling"]
    assert samp[0] is None and samp[-1] is None
    assert samp[1] == (0.4, 77, [generation.stream_id(10 + r, 0, 1) for r in range(5)])
    assert samp[2] == (0.8, 77, [generation.stream_id(10 + r, 0, 2) for r in range(5)])


def test_decisions_are_indexed_by_the_original_item(tiny):
    """transformers writes needs_fallback[i] / should_skip[i] with i the row of the shrunken sub-batch (generation_whisper.py
    :1074) and the caller reads should_skip by the original row (:1088): with item 0 settled at temperature 0, a skip decided
    for item 1 at the second temperature lands on item 0 there.  Here the skip stays with the item it was decided for."""
    g, v, W, spec = tiny
    tb, eos = spec.timestamp_begin, spec.eos_token_id
    good = [tb, 50, 61, 72, 83, 94, 105, tb + 1500, eos]
    loop = [tb] + [40, 41] * 10 + [tb + 1500, eos]
    # item 1 falls back on its compression ratio (its log-probability is fine, so no skip yet); the re-decode scores low and
    # the window is silent: skipped at the second temperature, when it is row 0 of transformers' sub-batch
    script = {(0, 0): (good, -0.3), (1, 0): (loop, -0.3), (1, 1): (good, -2.0)}
    eng = ScriptedEngine(spec, script, {0: 0.1, 1: 0.9})
    out, st = _generate(spec, eng, 2, (0.0, 0.5), (1.35, -1.0, 0.6))
    assert [(r["item"], r["temperature_index"], r["decision"]) for r in st["fallback"]] == \
        [(0, 0, "keep"), (1, 0, "fallback"), (1, 1, "skip")]
    assert out["sequences"][0][:len(good) - 1].tolist() == [t for t in good if t != eos]     # item 0 keeps its segment
    assert len(out["token_timestamps"][0]) == len(good) - 1 and len(out["token_timestamps"][1]) == 0


def test_refusals(tiny):
    g, v, W, spec = tiny
    full = {"num_beams": 1, "temperature": (0.0, 0.2, 0.4, 0.6, 0.8, 1.0), "compression_ratio_threshold": 1.35,
            "logprob_threshold": -1.0, "no_speech_threshold": 0.6}
    chk(dict(full), 5, spec, 0)                                            # the call of the issue, with the seed it draws with
    # a call that samples names its seed: there is no global generator to draw from, and a call that carries only
    # transformers' own arguments stays refused
    for unseeded in (full, {"num_beams": 1, "temperature": 0.7}, {"num_beams": 1, "temperature": (0.0, 0.2), "logprob_threshold": -1.0}):
        with pytest.raises(ValueError, match="sampling_seed"):
            chk(dict(unseeded), 5, spec)
    chk({"num_beams": 1, "temperature": (0.0, 0.2)}, 5, spec)            # no threshold: only the first temperature, nothing drawn
    for ok in ({"num_beams": 1, "temperature": 0.7}, {"num_beams": 1, "temperature": (0.5, 1.0)},
               {"num_beams": 1, "temperature": (0.0, 0.4), "compression_ratio_threshold": 2.0},
               {"temperature": (0.0, 0.5)}, {"temperature": 0.0, "compression_ratio_threshold": 1.35}):
        chk(dict(ok), 5, spec, 0)
    with pytest.raises(ValueError, match="do_sample"):
        chk({**full, "do_sample": True}, 5, spec, 0)
    for bad in ({**full, "num_beams": 2}, {"temperature": 0.7, "num_beams": 5}):
        with pytest.raises(ValueError, match="num_beams"):
            chk(dict(bad), 5, spec, 0)
    with pytest.raises(ValueError, match="pipeline default.*num_beams"):
        chk({k: x for k, x in full.items() if k != "num_beams"}, 5, spec, 0)
    with pytest.raises(ValueError, match="pipeline default.*num_beams"):
        chk({"temperature": 0.3}, 5, spec, 0)
    with pytest.raises(ValueError, match="prompt_ids"):
        chk({**full, "prompt_ids": np.array([v.startofprev, 40, 41])}, 5, spec, 0)
    with pytest.raises(ValueError, match="prompt_ids"):
        chk({"num_beams": 1, "temperature": (0.0, 0.4), "compression_ratio_threshold": 1.35,
             "prompt_ids": np.array([v.startofprev, 40, 41])}, 5, spec, 0)
    with pytest.raises(ValueError, match="at most 16"):
        chk({**full, "temperature": tuple(0.05 * i for i in range(17))}, 5, spec, 0)
    for k, val in (("top_k", 50), ("top_p", 0.9), ("min_p", 0.05), ("typical_p", 0.8), ("repetition_penalty", 1.2)):
        import dataclasses
        warped = dataclasses.replace(spec, sampling_warpers=_sampling_warpers({k: val}.get))
        with pytest.raises(ValueError, match=k):
            chk(dict(full), 5, warped, 0)
        chk({"num_beams": 1, "temperature": 0.0}, 5, warped, 0)            # a greedy call is what it was
    assert _sampling_warpers({"top_k": None, "top_p": 1.0, "repetition_penalty": 1.0}.get) == {}
    for bad in (-1, 2 ** 64, 1.5, True, "7"):
        with pytest.raises(ValueError):
            _check_seed(bad)
    assert _check_seed(2 ** 64 - 1) == 2 ** 64 - 1
    # generation.generate itself refuses the same before it touches the engine
    eng = ScriptedEngine(spec, {}, {})
    with pytest.raises(ValueError, match="num_beams"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", num_beams=2, temperature=0.5)
    with pytest.raises(ValueError, match="prompt_ids"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", num_beams=1, temperature=(0.0, 0.5),
                            compression_ratio_threshold=1.35, prompt_ids=np.array([v.startofprev, 40, 41]))
    assert eng.calls == []
