"""generate_kwargs={"prompt_ids": ...} on the host side (no GPU): argument handling in pipeline._check_generate_kwargs, the
decoder input of generation.init_tokens, and generation.generate's host loop (greedy and beam search) over the oracle-backed
engine against the transformers goldens of tests/golden/gen_golden_prompt.py."""
import numpy as np
import pytest
import torch

from crisperwhisper_amd import audio, collate, generation, synthetic as syn
from crisperwhisper_amd.pipeline import _check_generate_kwargs as chk
from tests import helpers as Hh

PROMPTS = list(Hh.gold_json("e2e_prompt_golden.json"))


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


def test_prompt_ids_accepted_forms(tiny):
    g, v, W, spec = tiny
    ids = [v.startofprev, 32, 120, 121]
    for form in (ids, np.array(ids, np.int64), np.array(ids, np.int32), torch.tensor(ids), tuple(ids)):
        chk({"prompt_ids": form, "num_beams": 1, "language": "<|en|>", "task": "transcribe"}, 5, spec)
        assert generation.check_prompt_ids(spec, form).tolist() == ids
    chk({"prompt_ids": torch.tensor(ids), "max_new_tokens": 448 - 3 - len(ids)}, 5, spec)   # exactly the limit


def test_prompt_ids_refused_forms(tiny):
    g, v, W, spec = tiny
    for bad in ([], [[v.startofprev, 32]], np.zeros((2, 2), np.int64), [1.5, 2.0], np.array([1.0, 2.0]), [True, 3],
                [-1, 5], [spec.vocab_size], torch.tensor([0, spec.vocab_size]), "hello", 7):
        with pytest.raises(ValueError, match="prompt_ids"):
            chk({"prompt_ids": bad, "num_beams": 1}, 5, spec)
    # the check needs the model: ids and lengths cannot be validated without its vocabulary and limits
    with pytest.raises(ValueError, match="prompt_ids"):
        chk({"prompt_ids": [v.startofprev, 32]})


def test_prompt_ids_length_error_is_transformers(tiny):
    """_set_max_new_tokens_and_length (generation_whisper.py:1920-1930): decoder input + max_new_tokens > 448 raises, with
    and without max_new_tokens, and with 2 (no task) or 3 init tokens."""
    g, v, W, spec = tiny
    p = [v.startofprev] + [97] * 439                                          # 440 ids
    with pytest.raises(ValueError, match="exceeds the `max_target_positions`"):
        chk({"prompt_ids": p, "language": "<|en|>", "task": "transcribe", "max_new_tokens": 6}, 5, spec)
    chk({"prompt_ids": p, "language": "<|en|>", "task": "transcribe", "max_new_tokens": 5}, 5, spec)
    with pytest.raises(ValueError, match="combined length of `decoder_input_ids` and `max_new_tokens` is: 449"):
        chk({"prompt_ids": [v.startofprev] + [97] * 445, "language": "<|en|>", "task": "transcribe"}, 5, spec)
    chk({"prompt_ids": [v.startofprev] + [97] * 443, "language": "<|en|>", "task": "transcribe"}, 5, spec)   # 447: one to generate
    chk({"prompt_ids": [v.startofprev] + [97] * 443, "num_beams": 1}, 5, spec)   # language detected: 2 init tokens
    with pytest.raises(ValueError, match="leaves no room"):                       # 448 input ids: nothing left to generate
        chk({"prompt_ids": [v.startofprev] + [97] * 445, "num_beams": 1}, 5, spec)
    with pytest.raises(ValueError, match="exceeds"):
        chk({"prompt_ids": [v.startofprev] + [97] * 445, "language": "<|en|>"}, 5, spec)   # a language brings <|transcribe|>
    with pytest.raises(ValueError, match="exceeds"):
        generation.check_prompt_length(spec, 446, 3)


def test_prompt_ids_refused_combinations(tiny):
    g, v, W, spec = tiny
    p = [v.startofprev, 32, 120]
    thr = {"temperature": 0.0, "logprob_threshold": -1.0, "no_speech_threshold": 0.6, "num_beams": 1}
    with pytest.raises(ValueError, match="no-speech position moves"):
        chk({**thr, "prompt_ids": p}, 5, spec)
    with pytest.raises(ValueError, match="no-speech position moves"):
        chk({"temperature": 0.0, "logprob_threshold": -1.0, "num_beams": 1, "prompt_ids": p}, 5, spec)
    for k in ("prompt_condition_type", "condition_on_prev_tokens"):       # unknown keys: still refused as such
        with pytest.raises(ValueError, match="not implemented on the native path"):
            chk({"prompt_ids": p, k: "all-segments" if k == "prompt_condition_type" else True}, 5, spec)
    with pytest.raises(ValueError, match="no-speech position moves"):     # generate itself refuses before touching the engine
        generation.generate(_NoEngine(spec), 1, [3000], language="<|en|>", task="transcribe",
                            prompt_ids=p, logprob_threshold=-1.0, no_speech_threshold=0.6)


class _NoEngine:
    """Any engine call is a failure: the refusals must come first."""

    def __init__(self, spec):
        self.spec = spec
        self.max_batch = 64

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} reached")


def test_init_tokens_with_prefix(tiny):
    g, v, W, spec = tiny
    p = np.array([v.startofprev, 32, 120], np.int64)
    assert generation.init_tokens(spec, "<|en|>", "transcribe", prompt_ids=p) == \
        [v.startofprev, 32, 120, v.sot, v.lang_id("en"), v.transcribe]
    assert generation.init_tokens(spec, None, "translate", lang_id=v.lang_id("de"), prompt_ids=torch.tensor(p)) == \
        [v.startofprev, 32, 120, v.sot, v.lang_id("de"), v.translate]
    assert generation.init_tokens(spec, "<|en|>", "transcribe") == [v.sot, v.lang_id("en"), v.transcribe]


def test_prompted_max_length_rule(tiny):
    """:1932-1946 with a prompt: max_new_tokens wins; without it max_length grows by min(223, n_in), capped at 448."""
    g, v, W, spec = tiny
    assert generation.prompted_max_length(spec, 20, 7) == 27
    assert generation.prompted_max_length(spec, 20, None) == 448
    import dataclasses
    s2 = dataclasses.replace(spec, max_length=100)
    assert generation.prompted_max_length(s2, 20, None) == 120
    assert generation.prompted_max_length(s2, 300, None) == 323
    with pytest.raises(ValueError, match="leaves no room"):          # a short checkpoint max_length below the prompt: refused
        generation.prompted_max_length(s2, 440, None)
    with pytest.raises(ValueError, match="leaves no room"):
        generation.prompted_max_length(spec, 20, 0)
    assert generation.prompted_max_length(dataclasses.replace(spec, max_length=300), 40, None) == 340
    assert generation.prompted_max_length(dataclasses.replace(spec, max_length=300), 200, None) == 448


@pytest.mark.parametrize("name", PROMPTS)
def test_host_loop_with_prompt_ids_vs_transformers(tiny, name):
    """generation.generate(native=False, prompt_ids=...) over the oracle-backed engine, chunk by chunk like the pipeline: the
    sequences of every generate call (prompt included), the token timestamps and the collated words equal transformers'."""
    g, v, W, spec = tiny
    meta = Hh.gold_json("e2e_prompt_golden.json")[name]
    z = Hh.gold_npz("e2e_prompt_golden.npz")
    x = syn.synth_audio(meta["seed"], int(round(meta["secs"] * 16000)), meta["kind"])
    eng = Hh.OracleBackedEngine(g, v, W, spec)
    vocab = collate.Vocabulary.from_synthetic(v)
    windows = audio.chunk_windows(len(x), 480000, 80000, 80000)
    gk = meta["generate_kwargs"]
    outputs, call = [], 0
    for b0 in range(0, len(windows), meta["batch_size"]):
        batch = windows[b0:b0 + meta["batch_size"]]
        _, nf = eng.mel([x[s:s + n] for s, n, _, _ in batch])
        out = generation.generate(eng, len(batch), nf, language=gk.get("language"), task=gk.get("task"),
                                  max_new_tokens=gk.get("max_new_tokens"), min_new_tokens=gk.get("min_new_tokens"),
                                  num_beams=gk.get("num_beams", 5), native=False, prompt_ids=np.array(meta["prompt_ids"]))
        want = z[f"{name}/call{call}/sequences"]
        assert np.array_equal(out["sequences"], want), (out["sequences"], want)
        for k, (_, _, st, _) in enumerate(batch):
            assert np.allclose(out["token_timestamps"][k], z[f"{name}/call{call}/tts{k}"], atol=1e-6)
            n = len(out["token_timestamps"][k])
            outputs.append({"tokens": out["sequences"][k][:n], "token_timestamps": out["token_timestamps"][k],
                            "stride": tuple(t / 16000 for t in st)})
        call += 1
    assert call == meta["n_generate_calls"]
    text, words = collate.decode_asr(vocab, outputs)
    assert text == meta["text"]
    ok, why = Hh.words_equal(words, meta["chunks"])
    assert ok, why
