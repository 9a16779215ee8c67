"""Host side of sequence_bias: the pipeline's argument check, generate's handling of the engine's table (set before the decode,
cleared when it ends or raises, refusals touching nothing), the align / score refusals and ``phrase_bias``.  Host-only: no GPU."""
import numpy as np
import pytest

from crisperwhisper_amd import _native, collate, generation
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline, _GENERATE_KWARGS, _check_generate_kwargs
from tests import helpers as Hh
from tests import sequence_bias_refs as S
from tests.test_top_logprobs_host import _bare_pipeline


def test_exported_symbols():
    for name in ("cw_set_sequence_bias", "cw_test_sample_biased"):
        assert name in _native.exported_symbols()
    assert _native.load().cw_abi_version() == 1
    assert (generation.SEQUENCE_BIAS_MAX, generation.SEQUENCE_BIAS_MAX_LEN) == (S.MAX_SEQ, S.MAX_LEN) == (256, 16)
    assert "sequence_bias" in _GENERATE_KWARGS


GOOD = [
    [[[37], 30.0]],
    [[[223, 37], 30.0], [[263, 300], 40.0]],
    {(223, 37): 30.0, (0, 5): -2.0},
    [[[5, 6], 1.0], [[5, 6], 2.0]],                                     # a duplicate collapses, the last bias wins
    [[[i + 1], 0.5] for i in range(256)],
    [[list(range(1, 17)), 3.0]],
]
BAD = [
    [], {}, "x", 7, {(1, 2): 1.0, 3: 2.0}, {(): 1.0}, {(1, -2): 1.0}, {(1, 2): 1}, [[[1, 2], 1]], [[[1, 0], 1.0]], [[[1, -1], 1.0]],
    [[(1, 2), 1.0]], [[[1.5], 1.0]], [[[], 1.0]], [[[True], 1.0]],
    [[[1769], 1.0]], {(5, 1769): 1.0},                                  # beyond the vocabulary (tiny: 1769 tokens)
    [[[1], float("inf")]], {(1,): float("nan")},
    [[[i + 1], 0.5] for i in range(257)], [[list(range(1, 18)), 3.0]],   # beyond the engine's limits
]


@pytest.mark.parametrize("arg", GOOD, ids=[repr(a)[:40] for a in GOOD])
def test_check_generate_kwargs_accepts(arg):
    g, v, W, spec = Hh.tiny_setup()
    _check_generate_kwargs({"num_beams": 1, "sequence_bias": arg}, 5, spec)
    assert generation.check_sequence_bias(arg, spec.vocab_size) == S.validate(arg, spec.vocab_size)


@pytest.mark.parametrize("arg", BAD, ids=[repr(a)[:40] for a in BAD])
def test_check_generate_kwargs_refuses(arg):
    g, v, W, spec = Hh.tiny_setup()
    with pytest.raises(ValueError):
        _check_generate_kwargs({"num_beams": 1, "sequence_bias": arg}, 5, spec)


def test_the_beam_refusals_name_the_way_out():
    g, v, W, spec = Hh.tiny_setup()
    for gk, default in (({"num_beams": 5}, 5), ({}, 5), ({"num_beams": 2}, 1)):
        with pytest.raises(ValueError, match="num_beams': 1"):
            _check_generate_kwargs(dict(gk, sequence_bias=GOOD[0]), default, spec)
    _check_generate_kwargs({"sequence_bias": GOOD[0]}, 1, spec)
    _check_generate_kwargs({"sequence_bias": None}, 5, spec)              # absent


class _Recorder:
    """An engine that records the calls that change its state and fails in ``transcribe``."""

    def __init__(self, spec, with_bias=True, fail=True):
        self.spec, self.max_batch, self.calls, self.fail = spec, 64, [], fail
        if with_bias:
            self.set_sequence_bias = lambda table: self.calls.append(("set_sequence_bias", table))

    def set_thresholds(self, *a):
        self.calls.append(("set_thresholds",) + a)

    def set_token_logprobs(self, on):
        self.calls.append(("set_token_logprobs", on))

    def set_top_logprobs(self, k):
        self.calls.append(("set_top_logprobs", k))

    def transcribe(self, n_items, *a, **kw):
        self.calls.append(("transcribe",))
        if self.fail:
            raise RuntimeError("decode failed")
        return [np.zeros(0, np.int64)] * n_items, [np.zeros(0, np.float32)] * n_items, 1

    def __getattr__(self, name):
        raise AttributeError(f"engine.{name} reached by a call that must be refused")


def test_generate_sets_the_table_and_clears_it_when_the_decode_raises():
    g, v, W, spec = Hh.tiny_setup()
    table = [[[223, 37], 30.0], [[37], 1.5], [[223, 37], 2.0]]
    want = [((223, 37), 2.0), ((37,), 1.5)]
    eng = _Recorder(spec)
    with pytest.raises(RuntimeError, match="decode failed"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", sequence_bias=table)
    names = [c[0] for c in eng.calls]
    assert eng.calls[0] == ("set_sequence_bias", want) and eng.calls[-1] == ("set_sequence_bias", None)
    assert names.index("transcribe") > 0 and names.count("set_sequence_bias") == 2
    eng = _Recorder(spec, fail=False)                                    # ... and when it ends normally
    generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", sequence_bias=table)
    assert eng.calls[0] == ("set_sequence_bias", want) and eng.calls[-1] == ("set_sequence_bias", None)
    eng = _Recorder(spec, fail=False)                                    # without the key the engine's table is not touched
    generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe")
    assert "set_sequence_bias" not in [c[0] for c in eng.calls]
    # an argument the call proper refuses: the table does not stay behind either
    eng = _Recorder(spec)
    with pytest.raises(ValueError, match="return_token_logprobs"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", sequence_bias=table, top_logprobs=3)
    assert eng.calls == [("set_sequence_bias", want), ("set_sequence_bias", None)]


@pytest.mark.parametrize("kw", [dict(num_beams=5), dict(num_beams=2)])
def test_generate_refuses_beams_before_the_engine_is_touched(kw):
    g, v, W, spec = Hh.tiny_setup()
    eng = _Recorder(spec)
    with pytest.raises(ValueError, match="num_beams=1"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", sequence_bias=[[[37], 30.0]], **kw)
    assert eng.calls == []
    with pytest.raises(ValueError):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", sequence_bias=[[[0], 30.0]])     # id 0 in list form
    assert eng.calls == []
    eng = _Recorder(spec, with_bias=False)
    with pytest.raises(ValueError, match="cw_set_sequence_bias"):
        generation.generate(eng, 1, [3000], language="<|en|>", task="transcribe", sequence_bias=[[[37], 30.0]])
    assert eng.calls == []


def test_pipeline_refusals_come_before_the_audio_is_loaded():
    """The input is no audio at all: loading it raises TypeError, every refusal is a ValueError before that."""
    g, v, W, spec = Hh.tiny_setup()
    p = _bare_pipeline(spec)
    sb = [[[37], 30.0]]
    with pytest.raises(ValueError, match="num_beams': 1"):
        p._run_one(12345, generate_kwargs={"sequence_bias": sb})                            # the pipeline default of 5 beams
    with pytest.raises(ValueError, match="num_beams': 1"):
        p._run_one(12345, generate_kwargs={"sequence_bias": sb, "num_beams": 5})
    with pytest.raises(ValueError):
        p._run_one(12345, generate_kwargs={"sequence_bias": [], "num_beams": 1})
    with pytest.raises(TypeError):
        p._run_one(12345, generate_kwargs={"sequence_bias": sb, "num_beams": 1})            # accepted: only now is the input loaded
    for who in ("align", "score"):
        with pytest.raises(ValueError, match="sequence_bias"):
            getattr(p, who)(12345, [1, 2], sequence_bias=sb)
        with pytest.raises(ValueError, match="sequence_bias"):
            getattr(p, who)(12345, [1, 2], generate_kwargs={"sequence_bias": sb})


class _StubTokenizer:
    """Bytes as ids, a leading space as its own id 32: enough to tell the two spellings apart."""

    def encode(self, text, add_special_tokens=True):
        assert add_special_tokens is False
        return [b for b in text.encode("utf-8")]


def test_phrase_bias_lists_both_spellings():
    g, v, W, spec = Hh.tiny_setup()
    p = _bare_pipeline(spec, tokenizer=_StubTokenizer())
    out = p.phrase_bias({"Metoprolol": 6.0, " ab ": -1})
    m = [b for b in b"Metoprolol"]
    assert out == [[m, 6.0], [[32] + m, 6.0], [[97, 98], -1.0], [[32, 97, 98], -1.0]]
    assert all(isinstance(b, float) for _, b in out)
    _check_generate_kwargs({"num_beams": 1, "sequence_bias": out}, 5, spec)                 # what it returns is accepted as it is
    for bad in ({}, [], {"": 1.0}, {"x": float("inf")}, {"x": "1"}, {"x" * 17: 1.0}, {3: 1.0}):
        with pytest.raises(ValueError):
            p.phrase_bias(bad)
    q = _bare_pipeline(spec, tokenizer=collate.Vocabulary.from_synthetic(v))               # no `encode`: refused, as align refuses text
    with pytest.raises(ValueError, match="encode"):
        q.phrase_bias({"ab": 1.0})
