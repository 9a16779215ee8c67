"""Host logic of per-head forced alignment and alignment-head selection (generation.align_heads, CrisperWhisperPipeline.align_heads
/ rank_alignment_heads, crisperwhisper_amd.metrics, the loaders' alignment_heads override, tools/select_alignment_heads.py).
No GPU: a stand-in engine records the calls; every refusal must come before it sees one."""
import importlib.util
import io
import json
import os
import types

import numpy as np
import pytest

from crisperwhisper_amd import collate, generation, metrics, synthetic as syn
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline, ModelBundle
from tests import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


class FakeEngine:
    """Records every call.  align_heads: head k of the request puts token i of a row at (i + shift[(l, h)]) * 0.02 s."""

    def __init__(self, spec, max_batch=4, shift=None):
        self.spec, self.max_batch, self.calls, self.shift = spec, max_batch, [], shift or {}

    def mel(self, clips):
        self.calls.append(("mel", len(clips)))
        return None, np.array([(len(c) + 159) // 160 for c in clips], np.int32)

    def align_heads(self, num_frames, ids, n_init, heads, ref=None, clip_frames=200):
        self.calls.append(("align_heads", [np.asarray(r).copy() for r in ids], n_init, np.asarray(num_frames).copy(),
                           [list(h) for h in heads], ref, clip_frames))
        ts = [[(np.arange(len(r)) + self.shift.get(tuple(h), 0)).astype(np.float32) * np.float32(0.02) for r in ids] for h in heads]
        if ref is None:
            return ts
        sim = [[np.where(np.isnan(ref[0][b]), np.nan, 0.1 * (k + 1)).astype(np.float32) for b in range(len(ids))]
               for k in range(len(heads))]
        return ts, sim


def _pipe(spec, v, eng=None):
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.vocab = collate.Vocabulary.from_synthetic(v)
    p.tokenizer = p.vocab
    p.sampling_rate = 16000
    p.engine = eng
    return p


# ------------------------------------------------------------------------------------------------------------ generation
def test_generation_align_heads_rows_heads_and_slices(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, shift={(1, 0): 10})
    out = generation.align_heads(eng, 2, [3000, 1200], [[5, 6, 7], np.array([8])], language="<|en|>", task="transcribe")
    (_, rows, n_init, nf, heads, ref, clip), = eng.calls
    init = [v.sot, v.lang_id("en"), v.transcribe]
    assert n_init == 3 and nf.tolist() == [3000, 1200] and ref is None and clip == 200
    assert heads == [[0, 0], [0, 1], [1, 0], [1, 1]] == out["heads"]              # None: every head, layer-major
    assert rows[0].tolist() == init + [5, 6, 7, v.eos] and rows[1].tolist() == init + [8, v.eos]
    assert len(out["token_timestamps"]) == 4 and len(out["token_timestamps"][0]) == 2
    assert np.allclose(out["token_timestamps"][0][0], [0.06, 0.08, 0.10]) and np.allclose(out["token_timestamps"][2][1], [0.26])
    assert "similarity" not in out
    eng = FakeEngine(spec)
    nan = float("nan")
    out = generation.align_heads(eng, 1, [3000], [[5, 6, 7]], [[1, 1], [0, 1]], language="<|en|>",
                                 ref=[([0.5, nan, 0.9], [0.7, nan, 1.0])], clip_frames=30)
    (_, rows, n_init, nf, heads, ref, clip), = eng.calls
    assert heads == [[1, 1], [0, 1]] and clip == 30
    assert np.array_equal(ref[0][0], np.array([nan, nan, nan, 0.5, nan, 0.9, nan], np.float32), equal_nan=True)
    assert np.array_equal(ref[1][0], np.array([nan, nan, nan, 0.7, nan, 1.0, nan], np.float32), equal_nan=True)
    assert np.array_equal(out["similarity"][1][0], np.array([0.2, nan, 0.2], np.float32), equal_nan=True)


def test_refusals_before_the_engine_sees_a_call(tiny):
    g, v, W, spec = tiny
    eng = FakeEngine(spec, max_batch=2)
    ok = dict(language="<|en|>")
    for heads, word in (([], "non-empty"), ([[0, 0], [0, 0]], "twice"), ([[2, 0]], "outside"), ([[0, 2]], "outside"),
                        ([[-1, 0]], "outside"), ([[0]], "pair"), ([[0.5, 1]], "pair"), ("all", "non-empty"), ([[True, 0]], "pair")):
        with pytest.raises(ValueError, match=word):
            generation.align_heads(eng, 1, [3000], [[5]], heads, **ok)
    with pytest.raises(ValueError, match="max_target_positions"):
        generation.align_heads(eng, 1, [3000], [[5] * (g.max_target_positions - 3)], **ok)
    with pytest.raises(ValueError, match="rows"):
        generation.align_heads(eng, 3, [3000] * 3, [[5]] * 3, **ok)
    with pytest.raises(ValueError, match="transcripts"):
        generation.align_heads(eng, 2, [3000] * 2, [[5]], **ok)
    with pytest.raises(ValueError, match="num_frames"):
        generation.align_heads(eng, 1, [3000, 3000], [[5]], **ok)
    with pytest.raises(ValueError, match="special"):
        generation.align_heads(eng, 1, [3000], [[v.eos]], **ok)
    for ref, word in (([([0.1], [0.2]), ([0.1], [0.2])], "entries"), ([([0.1],)], "pair"), ([([0.1, 0.2], [0.2])], "times"),
                      ([([0.1], [0.2, 0.3])], "times")):
        with pytest.raises(ValueError, match=word):
            generation.align_heads(eng, 1, [3000], [[5]], ref=ref, **ok)
    with pytest.raises(ValueError):
        generation.align_heads(eng, 1, [3000], [[5]], language="<|xx|>")
    p = _pipe(spec, v, eng)
    x = np.zeros(16000, np.float32)
    with pytest.raises(ValueError, match="prompt_ids"):
        p.align_heads(x, [5], language="<|en|>", prompt_ids=[1, 2])
    with pytest.raises(ValueError, match="sequence_bias"):
        p.align_heads(x, [5], generate_kwargs={"sequence_bias": [[[5], 1.0]]})
    with pytest.raises(ValueError, match="sequence_bias"):
        p.rank_alignment_heads([x], [[5]], [[]], sequence_bias=[[[5], 1.0]])
    with pytest.raises(ValueError, match="token ids"):
        p.align_heads(x, "hello", language="<|en|>")
    with pytest.raises(ValueError, match="2 transcripts"):
        p.align_heads([x, x], [[5]], language="<|en|>")
    with pytest.raises(ValueError, match="twice"):
        p.align_heads(x, [5], heads=[[1, 1], [1, 1]], language="<|en|>")
    with pytest.raises(ValueError, match="30 s"):
        p.align_heads(np.zeros(480001, np.float32), [5], language="<|en|>")
    with pytest.raises(TypeError):
        p.align_heads(x, [5], bogus=1)
    ids = [32, 97, 98, 32, 99]                                                    # " ab c": two words
    two = [{"text": " ab", "timestamp": (0.1, 0.2)}, {"text": " c", "timestamp": (0.3, 0.4)}]
    with pytest.raises(ValueError, match="input 1.*2 words.*1 references"):
        p.rank_alignment_heads([x, x], [ids, ids], [two, two[:1]], language="<|en|>")
    with pytest.raises(ValueError, match="input 0.*finite"):
        p.rank_alignment_heads([x], [ids], [[{"text": " ab", "timestamp": (0.1, float("nan"))}, two[1]]], language="<|en|>")
    with pytest.raises(ValueError, match="reference lists"):
        p.rank_alignment_heads([x, x], [ids, ids], [two], language="<|en|>")
    for kw, word in (({"top": 0}, "top"), ({"top": 1.5}, "top"), ({"collar": -1}, "collar"), ({"collar": float("nan")}, "collar")):
        with pytest.raises(ValueError, match=word):
            p.rank_alignment_heads([x], [ids], [two], language="<|en|>", **kw)
    assert eng.calls == []


def test_item_splitting_stays_under_the_cap(tiny):
    g, v, W, spec = tiny
    row = generation.ALIGN_HEADS_ROW_BYTES
    assert row == 6000
    n_ids = [41, 11, 41, 21, 5, 5, 5]
    for n_heads, max_batch, cap in ((4, 8, 4 * 40 * row * 2), (4, 2, 1 << 40), (1, 8, 40 * row), (3, 8, 3 * 40 * row * 3 - 1)):
        calls = generation.plan_align_heads_calls(n_ids, n_heads, max_batch, cap)
        assert [b for c in calls for b in c] == list(range(len(n_ids)))           # every item once, in order, consecutive groups
        for c in calls:
            assert len(c) <= max_batch
            assert len(c) * n_heads * (max(n_ids[b] for b in c) - 1) * row <= cap
    assert generation.plan_align_heads_calls(n_ids, 4, 8, 4 * 40 * row * 2) == [[0, 1], [2, 3], [4, 5, 6]]
    assert generation.plan_align_heads_calls([129] * 8, 640, 8) == [list(range(8))]      # 3.96 GB: one call under the 8 GiB cap
    assert len(generation.plan_align_heads_calls([448] * 8, 640, 8)) == 2                # 13.7 GB: split
    with pytest.raises(ValueError, match="fewer heads"):
        generation.plan_align_heads_calls([41], 4, 8, 4 * 40 * row - 1)
    # through generation.align_heads: the groups become calls, load_items makes a later group resident and restores the batch
    eng = FakeEngine(spec, max_batch=4)
    loaded = []
    import crisperwhisper_amd._native as N
    old = N.ALIGN_HEADS_MAX_BYTES
    try:
        N.ALIGN_HEADS_MAX_BYTES = 4 * 10 * row * 2                                # two items of <= 11 ids and 4 heads
        texts = [[5] * 7, [6] * 7, [7] * 3]
        with pytest.raises(ValueError, match="load_items"):
            generation.align_heads(eng, 3, [3000, 2000, 1000], texts, language="<|en|>")
        assert eng.calls == []
        out = generation.align_heads(eng, 3, [3000, 2000, 1000], texts, language="<|en|>", load_items=loaded.append)
    finally:
        N.ALIGN_HEADS_MAX_BYTES = old
    assert [len(c[1]) for c in eng.calls] == [2, 1] and loaded == [[2], [0, 1, 2]]
    assert eng.calls[1][3].tolist() == [1000] and eng.calls[1][1][0].tolist()[3:6] == [7, 7, 7]
    assert [len(t) for t in out["token_timestamps"][3]] == [7, 7, 3]


# --------------------------------------------------------------------------------------------------------------- metrics
def test_metrics_on_hand_made_intervals():
    ref = [[0.10, 0.30], [0.50, 0.90]]
    pred = [[0.12, 0.30], [0.40, 0.70]]
    e = metrics.boundary_errors(pred, ref)
    assert np.allclose(e, [[0.02, 0.0], [0.10, 0.20]])
    iou = metrics.interval_iou(pred, ref)
    assert np.allclose(iou, [0.18 / 0.20, 0.20 / 0.50])
    assert np.allclose(metrics.interval_iou([[0.2, 0.2], [0.2, 0.2], [0.1, 0.2]], [[0.2, 0.2], [0.3, 0.3], [0.3, 0.4]]), [1.0, 0.0, 0.0])
    m = metrics.head_metrics([pred], [ref], [[0.5, np.nan, 0.7]], collar=0.05)
    assert m["n_boundaries"] == 4 and m["n_within"] == 2 and m["within_collar"] == 0.5
    assert m["mean_abs_error"] == pytest.approx(0.08) and m["mean_iou"] == pytest.approx((0.9 + 0.4) / 2)
    assert m["mean_similarity"] == pytest.approx(0.6)
    assert metrics.head_metrics([[[0.15, 0.30]]], [[[0.10, 0.30]]], collar=0.05)["n_within"] == 2     # exactly the collar: within
    with pytest.raises(ValueError, match="words"):
        metrics.boundary_errors(pred, ref[:1])
    # tie order: share, then IoU, then similarity, then (layer, head)
    rows = {(0, 0): (0.5, 0.4, 0.9), (0, 1): (0.75, 0.1, 0.1), (1, 0): (0.5, 0.6, 0.1), (1, 1): (0.5, 0.4, 0.9), (2, 0): (0.5, 0.4, 0.95),
            (2, 1): (0.5, 0.4, float("nan"))}
    heads = list(rows)
    ms = [{"within_collar": a, "mean_iou": b, "mean_similarity": c} for a, b, c in rows.values()]
    r = metrics.rank_heads(heads, ms, top=3)
    assert [x["head"] for x in r["ranking"]] == [[0, 1], [1, 0], [2, 0], [0, 0], [1, 1], [2, 1]]
    assert r["alignment_heads"] == [[0, 1], [1, 0], [2, 0]]


def test_rank_alignment_heads_end_to_end_on_a_stand_in(tiny):
    g, v, W, spec = tiny
    # head (1, 1) puts every token where the reference has it, (1, 0) one frame late, (0, 1) three frames, (0, 0) ten
    eng = FakeEngine(spec, max_batch=2, shift={(1, 1): 0, (1, 0): 1, (0, 1): 3, (0, 0): 10})
    p = _pipe(spec, v, eng)
    ids = [[32, 97, 98, 32, 99], [32, 100], [32, 101, 102]]                       # " ab c", " d", " ef"
    clips = [np.zeros(16000, np.float32), np.zeros(8000, np.float32), np.zeros(4000, np.float32)]
    base = p.align_heads(clips, ids, heads=[[1, 1]], language="<|en|>")
    assert [len(c) for c in eng.calls if c[0] == "align_heads"] and [c[1] for c in eng.calls if c[0] == "mel"] == [2, 1]
    assert set(base[0]) == {"heads", "token_timestamps", "chunks"} and base[0]["heads"] == [[1, 1]]
    assert [w["text"] for w in base[0]["chunks"][0]] == [" ab", " c"]
    want = collate.decode_asr(p.vocab, [{"tokens": np.array(ids[0]), "token_timestamps": np.arange(3, 8, dtype=np.float32) * np.float32(0.02)}])
    assert base[0]["chunks"][0] == want[1]
    one = p.align_heads(clips[0], ids[0], language="<|en|>")
    assert isinstance(one, dict) and len(one["heads"]) == 4 and len(one["chunks"]) == 4 and len(one["token_timestamps"][0]) == 5
    refs = [[{"text": w["text"], "timestamp": w["timestamp"]} for w in b["chunks"][0]] for b in base]
    eng.calls.clear()
    r = p.rank_alignment_heads(clips, ids, refs, top=2, collar=0.05, language="<|en|>")
    call = [c for c in eng.calls if c[0] == "align_heads"][0]
    # every token of a word carries the word's interval; init tokens and eos carry none
    rb, re = call[5][0][0], call[5][1][0]
    w0, w1 = refs[0][0]["timestamp"], refs[0][1]["timestamp"]
    assert np.allclose(rb[3:8], [w0[0]] * 3 + [w1[0]] * 2) and np.allclose(re[3:8], [w0[1]] * 3 + [w1[1]] * 2)
    assert np.isnan(rb[:3]).all() and np.isnan(rb[8])
    assert r["alignment_heads"] == [[1, 1], [1, 0]]
    assert [x["head"] for x in r["ranking"]] == [[1, 1], [1, 0], [0, 1], [0, 0]]
    by = {tuple(x["head"]): x for x in r["ranking"]}
    assert by[(1, 1)]["within_collar"] == 1.0 and by[(1, 1)]["mean_abs_error"] == 0.0 and by[(1, 1)]["mean_iou"] == 1.0
    # the other heads: the metrics of the words the collator makes of their shifted token times
    ref_iv = [np.asarray([w["timestamp"] for w in rf], np.float64) for rf in refs]
    for head, shift in (((1, 0), 1), ((0, 1), 3), ((0, 0), 10)):
        pred = []
        for t in ids:
            ts = (np.arange(3, 3 + len(t)) + shift).astype(np.float32) * np.float32(0.02)
            pred.append(np.asarray([w["timestamp"] for w in collate.decode_asr(p.vocab, [{"tokens": np.array(t), "token_timestamps": ts}])[1]]))
        want = metrics.head_metrics(pred, ref_iv, collar=0.05)
        for key in ("mean_abs_error", "within_collar", "mean_iou", "n_boundaries", "n_within"):
            assert by[head][key] == pytest.approx(want[key]), (head, key)
    assert by[(1, 0)]["within_collar"] == 1.0 and 0 < by[(1, 0)]["mean_abs_error"] <= 0.02 + 1e-9
    assert by[(0, 1)]["within_collar"] < by[(1, 0)]["within_collar"] and by[(0, 0)]["n_boundaries"] == 8
    assert by[(0, 0)]["mean_similarity"] == pytest.approx(0.1) and by[(1, 1)]["mean_similarity"] == pytest.approx(0.4)


# --------------------------------------------------------------------------------------------------------------- loaders
def _checkpoint_dir(tmp_path, g, v, heads):
    cfg = {"model_type": "whisper", "d_model": g.d_model, "encoder_attention_heads": g.heads, "decoder_attention_heads": g.heads,
           "encoder_ffn_dim": g.ffn, "encoder_layers": g.enc_layers, "decoder_layers": g.dec_layers, "num_mel_bins": g.n_mels,
           "vocab_size": g.vocab, "max_target_positions": g.max_target_positions, "eos_token_id": v.eos, "pad_token_id": v.eos,
           "decoder_start_token_id": v.sot}
    gc = {"no_timestamps_token_id": v.notimestamps}
    if heads is not None:
        gc["alignment_heads"] = heads
    json.dump(cfg, open(tmp_path / "config.json", "w"))
    json.dump(gc, open(tmp_path / "generation_config.json", "w"))
    open(tmp_path / "model.safetensors", "wb").close()
    return str(tmp_path)


def test_loader_override_and_unchanged_default(tiny, tmp_path):
    g, v, W, spec = tiny
    d = tmp_path / "a"; d.mkdir()
    path = _checkpoint_dir(d, g, v, None)
    with pytest.raises(ValueError, match="no `alignment_heads`"):
        ModelBundle.from_pretrained(path)
    b = ModelBundle.from_pretrained(path, alignment_heads=[(1, 0), [0, 1]])
    assert b.spec.alignment_heads == [[1, 0], [0, 1]]
    for bad, word in (([[2, 0]], "outside"), ([[0, 2]], "outside"), ([[0, 0], [0, 0]], "twice"), ([], "non-empty"), ([[0]], "pair")):
        with pytest.raises(ValueError, match=word):
            ModelBundle.from_pretrained(path, alignment_heads=bad)
    d = tmp_path / "b"; d.mkdir()
    path = _checkpoint_dir(d, g, v, [[1, 1]])
    assert ModelBundle.from_pretrained(path).spec.alignment_heads == [[1, 1]]                   # the checkpoint's own, as before
    assert ModelBundle.from_pretrained(path, alignment_heads=[[0, 0]]).spec.alignment_heads == [[0, 0]]

    def hf_model(heads):
        cfg = types.SimpleNamespace(d_model=g.d_model, encoder_attention_heads=g.heads, decoder_attention_heads=g.heads,
                                    encoder_ffn_dim=g.ffn, encoder_layers=g.enc_layers, decoder_layers=g.dec_layers,
                                    num_mel_bins=g.n_mels, vocab_size=g.vocab, max_target_positions=g.max_target_positions,
                                    median_filter_width=7)
        gc = types.SimpleNamespace(no_timestamps_token_id=v.notimestamps, eos_token_id=v.eos, pad_token_id=v.eos,
                                   decoder_start_token_id=v.sot, suppress_tokens=None, begin_suppress_tokens=None, max_length=None)
        if heads is not None:
            gc.alignment_heads = heads
        return types.SimpleNamespace(config=cfg, generation_config=gc, state_dict=lambda: {})
    with pytest.raises(ValueError, match="no `alignment_heads`"):
        ModelBundle.from_hf(hf_model(None))
    assert ModelBundle.from_hf(hf_model(None), alignment_heads=[[1, 1]]).spec.alignment_heads == [[1, 1]]
    assert ModelBundle.from_hf(hf_model([[0, 1]])).spec.alignment_heads == [[0, 1]]
    assert ModelBundle.from_hf(hf_model([[0, 1]]), alignment_heads=[[1, 0]]).spec.alignment_heads == [[1, 0]]
    with pytest.raises(ValueError, match="outside"):
        ModelBundle.from_hf(hf_model([[0, 1]]), alignment_heads=[[5, 0]])


# ------------------------------------------------------------------------------------------------------------------ tool
def test_select_alignment_heads_tool_on_a_two_line_manifest(tmp_path):
    spec_ = importlib.util.spec_from_file_location("select_alignment_heads", os.path.join(ROOT, "tools", "select_alignment_heads.py"))
    tool = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(tool)
    man = tmp_path / "m.jsonl"
    man.write_text(json.dumps({"audio": "a.wav", "words": [{"text": "so", "start": 0.1, "end": 0.3}, {"text": "uh", "start": 0.5, "end": 0.6}]})
                   + "\n\n" + json.dumps({"audio": "/abs/b.wav", "words": [{"text": "ok", "start": 1.0, "end": 1.2}]}) + "\n")
    seen = {}

    class FakePipe:
        def rank_alignment_heads(self, inputs, transcripts, references, top, collar, language, task):
            seen.update(inputs=inputs, transcripts=transcripts, references=references, top=top, collar=collar, language=language,
                        task=task)
            ms = [{"within_collar": 0.25, "mean_iou": 0.2, "mean_similarity": 0.1, "mean_abs_error": 0.5},
                  {"within_collar": 0.75, "mean_iou": 0.6, "mean_similarity": 0.3, "mean_abs_error": 0.04}]
            return metrics.rank_heads([[0, 0], [1, 1]], ms, top=top)

    def make(a):
        seen["model"], seen["dtype"] = a.model, a.dtype
        return FakePipe()
    out = io.StringIO()
    res = tool.main(["--model", "DIR", "--manifest", str(man), "--top", "1", "--collar", "0.1", "--language", "en"],
                    make_pipeline=make, out=out)
    assert seen["inputs"] == [str(tmp_path / "a.wav"), "/abs/b.wav"] and seen["transcripts"] == [" so uh", " ok"]
    assert seen["references"][0][1] == {"text": "uh", "timestamp": (0.5, 0.6)} and len(seen["references"][1]) == 1
    assert (seen["top"], seen["collar"], seen["language"], seen["task"], seen["model"], seen["dtype"]) == (1, 0.1, "<|en|>", "transcribe", "DIR", "bf16")
    text = out.getvalue().splitlines()
    assert text[0].split() == ["rank", "layer", "head", "within_collar", "mean_iou", "mean_abs_error_s", "mean_similarity"]
    assert text[1].split()[:4] == ["1", "1", "1", "0.7500"] and text[2].split()[:3] == ["2", "0", "0"]
    assert text[-1] == '"alignment_heads": [[1, 1]]' and res["alignment_heads"] == [[1, 1]]
    bad = tmp_path / "bad.jsonl"
    bad.write_text(json.dumps({"audio": "a.wav", "words": [{"text": "so", "start": 0.1}]}) + "\n")
    with pytest.raises(ValueError, match="start and end"):
        tool.main(["--model", "DIR", "--manifest", str(bad)], make_pipeline=make, out=out)
