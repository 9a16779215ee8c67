"""The references of tests/align_heads_refs.py, checked without a device.

* The per-head timestamp reference (oracle.timestamps.extract_token_timestamps on one head) against the installed transformers:
  WhisperGenerationMixin._extract_token_timestamps(..., alignment_heads=[[l, h]], ...) over one teacher-forced eager forward, as
  tests/golden/gen_golden_align.py obtains it -- on the tiny model and on the 3-layer x 4-head model, for every head.
* Planted faults in a numpy model of the cw_align_heads path: the comparison against the references rejects each of them.
"""
import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from tests import align_heads_models as M
from tests import align_heads_refs as R

CLIPS = [(41, 30.0, 40), (43, 4.0, 17), (44, 12.5, 9)]            # (audio seed, seconds, ids in the row)


class _Out(dict):
    __getattr__ = dict.__getitem__


def _forward(name):
    """Per clip: (num_frames, ids, all cross-attention rows [1][layers * H][L][S] layer-major, the HF model, its forward)."""
    import torch
    g, v, W, spec, model, _, fe = M.hf_model(name)
    out = []
    for seed, secs, n in CLIPS:
        x = syn.synth_audio(seed, int(secs * 16000), "mixed")
        r = fe(x, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        ids = M.rows(v, [n], seed)[0]
        dec_in = torch.tensor([ids[:-1].tolist()])
        with torch.no_grad():
            o = model(input_features=r.input_features, decoder_input_ids=dec_in, output_attentions=True)
        allw = torch.cat(list(o.cross_attentions), dim=1).numpy()
        out.append((int(r.attention_mask.sum()), ids, allw, dec_in, o))
    return g, spec, model, out


_FWD = {}


@pytest.fixture(params=["tiny", "mid"])
def fwd(request):
    if request.param not in _FWD:
        _FWD[request.param] = _forward(request.param)
    return _FWD[request.param]


def test_per_head_reference_equals_transformers(fwd):
    g, spec, model, clips = fwd
    assert len(M.all_heads(g)) == {2: 4, 3: 12}[g.dec_layers]
    distinct = set()
    for nf, ids, allw, dec_in, o in clips:
        for k, (l, h) in enumerate(M.all_heads(g)):
            want = model._extract_token_timestamps(_Out(sequences=dec_in, cross_attentions=(o.cross_attentions,)), [[l, h]],
                                                   num_frames=[nf], num_input_ids=3)[0].numpy()
            got = R.head_timestamps(allw, [nf], 3, g.median_filter_width, k)[0]
            assert len(got) == len(ids) and np.array_equal(got, want), (nf, (l, h), got, want)
            distinct.add(tuple(got.tolist()))
    assert len(distinct) > len(clips) * 2                         # the heads do differ: the comparison is not one of copies


# ------------------------------------------------------------------------------------------------------- planted faults
def _batch(fwd):
    """The three clips as one ragged batch: weights padded to the longest row, as the engine's capture holds them."""
    g, spec, model, clips = fwd
    Lmax = max(a.shape[2] for _, _, a, _, _ in clips)
    allw = np.zeros((len(clips), clips[0][2].shape[1], Lmax, 1500), np.float32)
    for b, (_, _, a, _, _) in enumerate(clips):
        allw[b, :, :a.shape[2]] = a[0]
    return g, allw, [c[0] for c in clips], [len(c[1]) for c in clips]


def _reference(g, allw, nf, n_ids, heads):
    out = []
    for l, h in heads:
        k = l * g.heads + h
        out.append([R.head_timestamps(allw[b:b + 1, :, :n_ids[b] - 1], [nf[b]], 3, g.median_filter_width, k)[0]
                    for b in range(len(nf))])
    return out


def _equal(a, b):
    return all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_timestamp_model_matches_and_planted_faults_are_rejected(fwd):
    g, allw, nf, n_ids = _batch(fwd)
    heads = M.all_heads(g)
    heads = [heads[i] for i in ([3, 0, 2, 1] if g.dec_layers == 2 else [9, 3, 6, 1, 11])]     # shuffled, l != h among them
    want = _reference(g, allw, nf, n_ids, heads)
    good = R.model_align_heads(allw, g.heads, heads, nf, 3, n_ids, g.median_filter_width)
    assert _equal(good, want)
    for fault in ("head_mean", "swap_layer_head", "slot_order", "ncols_item0"):
        bad = R.model_align_heads(allw, g.heads, heads, nf, 3, n_ids, g.median_filter_width, fault=fault)
        assert not _equal(bad, want), fault


def _accepts(got, want, n_cols):
    """The comparator of the GPU test (NaN exactly where the definition has it, the rest within the bound) on one value."""
    bound = 0.0 if np.isnan(want) else R.similarity_bound(want, n_cols)
    return R.compare_similarity(np.array([got]), np.array([want]), np.array([bound]))[0]


def test_similarity_planted_faults_are_rejected():
    rng = np.random.default_rng(3)
    n_cols = 200
    x = rng.standard_normal((6, 1500)) * 2
    a = np.exp(x) / np.exp(x[:, :n_cols]).sum(axis=1, keepdims=True)
    a = a.astype(np.float32)
    s, e = np.float32(1.0), np.float32(1.19)                      # frames 50 .. 59
    assert R.interval_frames(s, e) == (50, 60)
    for clip in (0, 2, 200, -1):
        for row in a:
            want = R.similarity64(row, n_cols, s, e, clip)
            assert _accepts(R.model_similarity(row, n_cols, s, e, clip), want, n_cols)
            bad = R.model_similarity(row, n_cols, s, e, clip, fault="ramp_shift")
            assert not _accepts(bad, want, n_cols), ("ramp_shift", clip)
            if 0 <= clip < 200:
                bad = R.model_similarity(row, n_cols, s, e, clip, fault="clip_g")
                assert not _accepts(bad, want, n_cols), ("clip_g", clip)
            z = R.similarity64(row, n_cols, s, s, clip)           # a zero-length interval still covers one frame
            bad = R.model_similarity(row, n_cols, s, s, clip, fault="f1_eq_f0")
            assert not _accepts(bad, z, n_cols), ("f1_eq_f0", clip)
    # hand-checked values: all mass on the interval's single frame, and on the first ramp frame
    row = np.zeros(1500, np.float32); row[50] = 1.0
    g = R.target(50, 51, 200)
    assert g[46:55].tolist() == pytest.approx([0.2, 0.4, 0.6, 0.8, 1.0, 0.8, 0.6, 0.4, 0.2])
    assert R.similarity64(row, 200, 1.0, 1.0, -1) == pytest.approx(1.0 / np.sqrt(np.dot(g, g)))
    row = np.zeros(1500, np.float32); row[49] = 1.0
    assert R.similarity64(row, 200, 1.0, 1.0, -1) == pytest.approx(0.8 / np.sqrt(np.dot(g, g)))
    assert np.isnan(R.similarity64(row, 200, 1.0, 1.0, 0))       # clipped to the interval: nothing left of the row
    assert np.isnan(R.similarity64(row, 200, np.nan, 1.0, -1)) and np.isnan(R.similarity64(row, 40, 1.0, 1.0, -1))
    assert R.similarity_bound(1.0, 1500) == pytest.approx((2 * (1 + 24 + 6) + 6) * 2.0 ** -24)
