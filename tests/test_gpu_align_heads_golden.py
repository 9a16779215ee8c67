"""Per-head forced alignment against transformers (tests/golden/align_heads_golden.json, written by
tests/golden/gen_golden_align_heads.py): every head's token timestamps, and the head ranking end to end.

f32: within 20 ms of transformers on every well-conditioned (case, head) pair -- a pair is ill-conditioned when transformers'
own timestamps move by more than 20 ms under a relative perturbation of 1e-6 of the attention rows; the golden flags those.
bf16 / f16: the share within 20 ms is reported, not held to a floor of its own (tests/test_gpu_align_vs_transformers.py holds
the mean of the configured heads)."""
import numpy as np
import pytest

import crisperwhisper_amd as cw
from crisperwhisper_amd import collate, synthetic as syn
from crisperwhisper_amd.engine import Engine
from tests import align_heads_models as M
from tests import helpers as Hh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return Hh.gold_json("align_heads_golden.json")


def _conditioning(gm):
    designed = gm["designed"]
    pairs = [(ci, p) for ci, c in enumerate(gm["cases"]) for p in c["heads"]]
    ill_designed = [1 for _, p in pairs if p["head"] in designed and p["ill_conditioned"]]
    other = [p["ill_conditioned"] for _, p in pairs if p["head"] not in designed]
    assert not ill_designed, "the golden leaves a designed alignment head out"
    assert 2 * sum(other) <= len(other), "the golden leaves more than half of the other pairs out"


def _rows(v, case):
    return np.asarray([v.sot, v.lang_id("en"), v.transcribe] + case["ids"] + [v.eos], np.int64)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_every_head_vs_transformers(gold, name, dtype):
    gm = gold["models"][name]
    _conditioning(gm)
    g, v, W, spec = M.setup(name)
    heads = M.all_heads(g)
    assert [p["head"] for p in gm["cases"][0]["heads"]] == heads
    eng = Engine(spec, dtype=dtype, max_batch=4)
    eng.load_state_dict(W)
    try:
        cases = gm["cases"]
        _, nf = eng.mel([syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"]) for c in cases])
        assert nf.tolist() == [c["num_frames"] for c in cases]
        got = eng.align_heads(nf, [_rows(v, c) for c in cases], 3, heads)
    finally:
        eng.close()
    near, total, worst = 0, 0, 0.0
    for k, head in enumerate(heads):
        for b, c in enumerate(cases):
            p = c["heads"][k]
            if p["ill_conditioned"]:
                continue
            d = np.abs(got[k][b].astype(np.float64) - np.asarray(p["token_timestamps"]))
            near += int(np.sum(d <= 0.02 + 1e-6)); total += d.size; worst = max(worst, float(d.max()))
            if dtype == "f32":
                assert d.max() <= 0.02 + 1e-6, (head, b, float(d.max()))
    print(f"{name} {dtype}: {near} of {total} token timestamps of the well-conditioned pairs within 20 ms of transformers "
          f"({near / total:.4f}); worst {worst:.2f} s")


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_rank_alignment_heads_vs_transformers(gold, name):
    gm = gold["models"][name]
    g, v, W, spec = M.setup(name)
    pipe = cw.pipeline("automatic-speech-recognition", model=cw.ModelBundle(spec, W), tokenizer=collate.Vocabulary.from_synthetic(v),
                       batch_size=4, num_beams=1, return_timestamps="word", torch_dtype="float32", device="cuda:0")
    try:
        cases = gm["cases"]
        clips = [syn.synth_audio(c["clip"]["seed"], int(round(c["clip"]["secs"] * 16000)), c["clip"]["kind"]) for c in cases]
        refs = [[{"text": w["text"], "timestamp": tuple(w["timestamp"])} for w in c["configured"]["chunks"]] for c in cases]
        got = pipe.rank_alignment_heads(clips, [c["ids"] for c in cases], refs, top=gm["top"], collar=gold["collar"],
                                        language="<|en|>", task="transcribe")
        words = pipe.align_heads(clips[1], cases[1]["ids"], heads=[gm["designed"][0]], language="<|en|>")
    finally:
        pipe.engine.close()
    want = gm["ranking"]
    print(f"{name}: engine   {[(r['head'], r['n_within']) for r in got['ranking']]}")
    print(f"{name}: transformers {[(r['head'], r['n_within']) for r in want]}")
    assert [w["text"] for w in words["chunks"][0]] == [w["text"] for w in cases[1]["configured"]["chunks"]]
    assert len(got["ranking"]) == len(want) and got["ranking"][0]["n_boundaries"] == want[0]["n_boundaries"]
    # a place of the reference ranking is decided where its share differs from both neighbours' by at least one boundary
    n = [r["n_within"] for r in want]
    decided = [i for i in range(len(n)) if (i == 0 or n[i - 1] - n[i] >= 1) and (i + 1 == len(n) or n[i] - n[i + 1] >= 1)]
    for i in decided:
        if i < gm["top"]:
            assert got["alignment_heads"][i] == want[i]["head"], (i, got["alignment_heads"], want[i]["head"])
    if gm["designed_first"]:
        assert sorted(got["alignment_heads"]) == sorted(gm["designed"])
    else:
        assert got["alignment_heads"] == gm["alignment_heads"]
