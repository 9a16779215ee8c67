"""The cross-query x term in qkv_self_kernel's V-tile blocks and the two-segment fused stage over 16-bit attention rows
(DESIGN.md 6g''', <= 8 greedy rows, 16-bit engines, packed LN-folded weights) against the three-segment launch they replace.

One engine per (geometry, dtype); option "no_xq_in_qkv" (cw_set_option: what CW_NO_XQ_IN_QKV=1 selects when a context is created) flips
the plan in place and drops the step graphs.  Both positions run the same forced-token decode -- N_NEW consecutive forwards behind the
prompt -- twice: as graph replays, and launch by launch with every step's logits captured (capturing takes the engine off the graph).
Held byte for byte between the two positions and between replay and launches: the logits of every step, the alignment rows, the rows
the forwards appended to the self-attention caches of every layer, and the qa plane the last layer left.

Geometries: the tiny model (d_model 128, two layers: the one-slot kernel forms, 16 q/k/v tiles per 8 V-tile blocks) and ONE decoder
layer of the large-v3 geometry (d_model 1280: the three-slot forms the benchmark runs, 80 V-tile blocks, one more weight tile each)."""
import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "f16")
ROWS = (1, 5, 8)
GEOMS = ("tiny", "wide")
N_PROMPT = 3
N_NEW = 205                        # forced-token forwards behind the prompt (the issue asks for at least 200)
T = N_PROMPT + N_NEW


@pytest.fixture(scope="module")
def models():
    g, v, W, spec = Hh.tiny_setup()
    out = {"tiny": (g, v, W, spec)}
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 1, 1
    spec = syn.model_spec(g, v, n_align=4)
    spec.alignment_heads = [[0, 0], [0, 3], [0, 7], [0, 19]]
    out["wide"] = (g, v, syn.random_weights(g, seed=11), spec)
    return out


@pytest.fixture(scope="module")
def engines(models):
    made = {}

    def get(geom, dt):
        if (geom, dt) not in made:
            g, v, W, spec = models[geom]
            e = Engine(spec, dtype=dt, max_batch=8)
            e.load_state_dict(W)
            e.mel([syn.synth_audio(40 + i, 480000 - 16000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(8)])
            made[(geom, dt)] = e
        return made[(geom, dt)]

    yield get
    for e in made.values():
        e.close()


def _forced(v, spec, nb, seed):
    """text tokens only (bytes of the synthetic vocabulary), a different stream per row"""
    rng = np.random.default_rng(seed)
    f = np.full((nb, T), -1, np.int32)
    f[:, N_PROMPT:] = rng.integers(ord("a"), ord("z") + 1, size=(nb, N_NEW))
    return f


def _state(eng, spec, nb):
    L = spec.dec_layers
    return {"last_logits": eng.last_logits(nb).copy(), "align": eng.alignment(nb, T - 1).copy(), "qa": eng.test_decode_state("qa", nb),
            "k": np.stack([eng.test_decode_state("k", nb, l, T - 1) for l in range(L)]),
            "v": np.stack([eng.test_decode_state("v", nb, l, T - 1) for l in range(L)])}


def _decode(eng, v, spec, nb, forced, capture):
    """one forced decode of T tokens; capture: launch by launch with the logits of every step, else graph replays"""
    eng.encode(list(range(nb)), [0] * nb, [3000 - 100 * b for b in range(nb)])
    prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (nb, 1))
    cap = eng.capture_logits(nb, N_NEW) if capture else None
    try:
        seqs, lens, _ = eng.decode(prompt, max_length=T, min_new_tokens=N_NEW, forced=forced)
    finally:
        if capture:
            eng.stop_capture()
    assert lens.tolist() == [T] * nb and np.array_equal(seqs[:, N_PROMPT:T], forced[:, N_PROMPT:]), "the rows did not follow the forced tokens"
    st = _state(eng, spec, nb)
    st["ids"] = seqs[:, :T].copy()
    if capture:
        st["logits"] = cap[:N_NEW].copy()
    return st


def _same(a, b, what):
    for k in a:
        if k in b:
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape)
            assert x.tobytes() == y.tobytes(), f"{what}: {k} differs ({int((x != y).sum())} of {x.size} elements)"


def _set_xq(eng, on):
    eng._chk(eng.lib.cw_set_option(eng.ctx, b"no_xq_in_qkv", 0 if on else 1))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", GEOMS)
def test_switch_on_equals_off(models, engines, geom, dtype, rows):
    g, v, W, spec = models[geom]
    eng = engines(geom, dtype)
    forced = _forced(v, spec, rows, 100 * rows + len(geom))
    runs = {}
    try:
        for on in (True, False):
            _set_xq(eng, on)
            assert int(eng.test_decode_state("xq_plan", rows)[0]) == (1 if on else 0), "the switch does not select the launch plan"
            runs[on, "graph"] = _decode(eng, v, spec, rows, forced, capture=False)
            runs[on, "eager"] = _decode(eng, v, spec, rows, forced, capture=True)
    finally:
        _set_xq(eng, True)
    assert int(eng.lib.cw_handoff_fallbacks(eng.ctx)) == 0, "the context left qkv_self_kernel: the switch selected nothing"
    what = f"{geom} {dtype} rows={rows}"
    lg = runs[True, "eager"]["logits"]
    assert lg.shape == (N_NEW, rows, spec.vocab_size) and np.isfinite(lg).all() and np.isfinite(runs[True, "eager"]["qa"]).all()
    assert np.abs(runs[True, "eager"]["qa"]).max() > 0
    _same(runs[True, "eager"], runs[False, "eager"], what + " launches, switch on vs off")
    _same(runs[True, "graph"], runs[False, "graph"], what + " graph replay, switch on vs off")
    _same(runs[True, "graph"], runs[True, "eager"], what + " switch on, graph replay vs launches")
    _same(runs[False, "graph"], runs[False, "eager"], what + " switch off, graph replay vs launches")


@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_off_fallback_keeps_the_three_segment_launch(models, dtype):
    """qkv_self_kernel's item blocks give up at one position (test hook "handoff_fail_pos"): the call resumes there on the two-launch
    q/k/v path, whose fused stage is the three-segment launch; everything equals the undisturbed run with the switch in either
    position"""
    g, v, W, spec = models["tiny"]
    rows = 5
    forced = _forced(v, spec, rows, 77)
    eng = Engine(spec, dtype=dtype, max_batch=8)
    try:
        eng.load_state_dict(W)
        eng.mel([syn.synth_audio(40 + i, 480000 - 16000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)])
        _set_xq(eng, False)
        off = _decode(eng, v, spec, rows, forced, capture=False)
        _set_xq(eng, True)
        on = _decode(eng, v, spec, rows, forced, capture=False)
        assert int(eng.lib.cw_handoff_fallbacks(eng.ctx)) == 0
        eng._chk(eng.lib.cw_set_option(eng.ctx, b"handoff_fail_pos", 60))
        disturbed = _decode(eng, v, spec, rows, forced, capture=False)
        assert int(eng.lib.cw_handoff_fallbacks(eng.ctx)) == 1 and int(eng.lib.cw_handoff_resumes(eng.ctx)) == 1
        assert int(eng.test_decode_state("xq_plan", rows)[0]) == 0, "without qkv_self_kernel the stage keeps its three segments"
        after = _decode(eng, v, spec, rows, forced, capture=False)      # the context stays on the launch-per-stage kernels
        assert int(eng.lib.cw_handoff_fallbacks(eng.ctx)) == 1
    finally:
        eng.close()
    _same(on, off, f"{dtype} undisturbed, switch on vs off")
    _same(disturbed, off, f"{dtype} hand-off gave up at position 60")
    _same(after, off, f"{dtype} the call after the fallback")
