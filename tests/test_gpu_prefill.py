"""The decoder prompt prefill (csrc/prefill.hip) on the device: its GEMM and attention kernels against numpy in f32 through the
cw_test_prefill_* hooks, the whole prefill against the per-position loop it replaces (cw_set_option "prompt_prefill" = 0) at
1 .. 64 rows and prompts of 5 .. 200 positions, greedy and beam search, and unprompted calls, which must not engage it."""
import numpy as np
import pytest
import torch

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}      # unit roundoff of the 16-bit type


def _round16(x, dt):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return t.to(torch.bfloat16 if dt == "bf16" else torch.float16).to(torch.float32).numpy().astype(np.float64)


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    g, v, W, spec = tiny
    out = {}
    for dt in ["f32"] + DTYPES:
        e = Engine(spec, dtype=dt, max_batch=64)
        e.load_state_dict(W)
        out[dt] = e
    yield out
    for e in out.values():
        e.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K", [(1, 48, 64), (37, 64, 96), (130, 80, 128), (64, 3 * 128, 128)])
def test_prefill_gemm_vs_numpy(engines, dt, M, N, K):
    """prefill_gemm_kernel over packed weights, every epilogue, ragged M (rows past M never read or written): against
    numpy on the 16-bit-rounded operands.  Bound: 16-bit outputs within 2 roundoffs of the value + 1e-4 * sqrt(K) (f32
    accumulation order); the f32 residual add within 1e-4 * sqrt(K)."""
    rng = np.random.default_rng(M * 1000 + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    ref = _round16(A, dt) @ _round16(W, dt).T + bias
    e = engines[dt]
    acc_tol = 1e-4 * np.sqrt(K)
    got = e.test_prefill_gemm(0, A, W, bias)
    assert np.all(np.abs(got - ref) <= 2 * EPS[dt] * np.abs(ref) + acc_tol), np.abs(got - ref).max()
    gelu = 0.5 * ref * (1.0 + torch.erf(torch.from_numpy(ref / np.sqrt(2.0))).numpy())
    got = e.test_prefill_gemm(3, A, W, bias)
    assert np.all(np.abs(got - gelu) <= 2 * EPS[dt] * np.abs(gelu) + acc_tol), np.abs(got - gelu).max()
    got = e.test_prefill_gemm(2, A, W, bias, resid=resid)
    assert np.all(np.abs(got - (resid + ref)) <= acc_tol), np.abs(got - (resid + ref)).max()


def _attn_ref(q, k, v, n_keys, causal, kv_div, dt):
    q, k, v = _round16(q, dt), _round16(k, dt), _round16(v, dt)
    rows, n_q, D = q.shape
    H = k.shape[1]
    out = np.zeros((rows, n_q, D))
    for r in range(rows):
        for h in range(H):
            s = q[r, :, h * 64:(h + 1) * 64] @ k[r // kv_div, h, :n_keys].T          # [n_q][n_keys]
            if causal:
                s = np.where(np.arange(n_keys)[None, :] <= np.arange(n_q)[:, None], s, -np.inf)
            p = np.exp(s - s.max(-1, keepdims=True))
            out[r, :, h * 64:(h + 1) * 64] = (p / p.sum(-1, keepdims=True)) @ v[r // kv_div, h, :n_keys]
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows,n_q,H,cap,n_keys,causal,kv_div", [
    (2, 5, 2, 448, 5, True, 1), (3, 33, 2, 448, 33, True, 1), (1, 70, 2, 448, 70, True, 1), (2, 17, 3, 20, 17, True, 1),
    (2, 200, 1, 448, 200, True, 1),
    (4, 37, 2, 1500, 1500, False, 2), (1, 16, 1, 1500, 1500, False, 1), (5, 3, 2, 1500, 1500, False, 5)])
def test_prefill_attention_vs_numpy(engines, dt, rows, n_q, H, cap, n_keys, causal, kv_div):
    """prefill_attn_kernel against numpy softmax attention on the 16-bit-rounded operands: causal self mode over the row's own
    cache rows (several n_q, cap; ragged last query and key tiles), cross mode over 1500 keys (ragged last 32-key tile) with
    rows sharing a K/V row (kv_div, the beam layout).  Cache entries past the keys a query may see hold NaN: never read.
    Bound: P goes through the 16-bit type before the P V product, so 4 roundoffs of max |v| + 1e-4."""
    rng = np.random.default_rng(rows * 7 + n_q + cap)
    q = (rng.standard_normal((rows, n_q, H * 64)) * 0.3).astype(np.float32)
    k = rng.standard_normal((rows // kv_div, H, cap, 64)).astype(np.float32)
    v = rng.standard_normal((rows // kv_div, H, cap, 64)).astype(np.float32)
    k[:, :, n_keys:] = np.nan
    v[:, :, n_keys:] = np.nan
    got = engines[dt].test_prefill_attention(q, k, v, n_keys, causal, kv_div)
    want = _attn_ref(q, k, v, n_keys, causal, kv_div, dt)
    bound = 4 * EPS[dt] * np.abs(v[:, :, :n_keys]).max() + 1e-4
    assert np.isfinite(got).all() and np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)


def _prompt(v, n_prompt, rows, seed):
    rng = np.random.default_rng(seed)
    pre = [[v.startofprev] + rng.integers(32, 127, n_prompt - 4).tolist() for _ in range(rows)]
    return np.array([p + [v.sot, v.lang_id("en"), v.transcribe] for p in pre], np.int32)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows", [1, 8, 16, 40, 64])
@pytest.mark.parametrize("n_prompt", [5, 33, 70, 200])
def test_prefill_against_the_loop_first_step_logits(tiny, engines, dt, rows, n_prompt):
    """The first generated step's logits after a prefilled prompt against the same step after the per-position loop, both
    against the f32 engine.  Bound: the prefill's distance to f32 is at most twice the loop's plus 2 roundoffs of the logit
    range -- both are 16-bit roundings of the same forward, neither may be worse than the other by more than that.  The prefill
    must also have engaged: its logits are not bit-identical to the loop's."""
    g, v, W, spec = tiny
    n_items = min(rows, 4)
    clips = [syn.synth_audio(300 + i, 300000, "mixed") for i in range(n_items)]
    item = [i % n_items for i in range(rows)]
    prompt = _prompt(v, n_prompt, rows, seed=rows * 1000 + n_prompt)
    res = {}
    for name, dtype, pf in (("f32", "f32", True), ("prefill", dt, True), ("loop", dt, False)):
        e = engines[dtype]
        if dtype != "f32":
            e.set_prompt_prefill(pf)
        e.mel(clips)
        e.encode(item, [0] * rows, [3000] * rows)
        e.set_prompt_prefix(n_prompt - 3)
        e.decode(prompt, max_length=n_prompt + 1)
        e.set_prompt_prefix(0)
        res[name] = e.last_logits(rows).astype(np.float64)
    engines[dt].set_prompt_prefill(True)
    ref = res["f32"]
    d_pf, d_lp = np.abs(res["prefill"] - ref).max(), np.abs(res["loop"] - ref).max()
    span = np.abs(ref).max()
    print(f"{dt} rows {rows} prompt {n_prompt}: max |logit - f32| prefill {d_pf:.4g}, loop {d_lp:.4g} (max |logit| {span:.3g})")
    assert d_pf <= 2 * d_lp + 2 * EPS[dt] * span, (d_pf, d_lp, span)
    assert not np.array_equal(res["prefill"], res["loop"])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n_prompt", [5, 70])
def test_prefill_under_beam_search_against_the_loop(tiny, engines, dt, n_prompt):
    """8 items x 5 beams = 40 rows, the beam layout (cross K/V row = row / 5): the first beam step's best processed
    log-probabilities after cw_beam_begin with and without the prefill, against the f32 engine; bound as above."""
    g, v, W, spec = tiny
    items, K = 8, 5
    clips = [syn.synth_audio(400 + i, 250000, "noise") for i in range(items)]
    prompt = _prompt(v, n_prompt, items, seed=n_prompt)
    res = {}
    for name, dtype, pf in (("f32", "f32", True), ("prefill", dt, True), ("loop", dt, False)):
        e = engines[dtype]
        if dtype != "f32":
            e.set_prompt_prefill(pf)
        e.mel(clips)
        e.encode(list(range(items)), [0] * items, [3000] * items)
        e.set_prompt_prefix(n_prompt - 3)
        e.beam_begin(prompt, K, n_prompt + 4)
        e.set_prompt_prefix(0)
        vals, toks = e.beam_step(2 * K)
        res[name] = vals[:, 0].astype(np.float64)
    engines[dt].set_prompt_prefill(True)
    d_pf, d_lp = np.abs(res["prefill"] - res["f32"]).max(), np.abs(res["loop"] - res["f32"]).max()
    span = np.abs(res["f32"]).max()
    print(f"{dt} beam prompt {n_prompt}: max |logprob - f32| prefill {d_pf:.4g}, loop {d_lp:.4g}")
    assert d_pf <= 2 * d_lp + 2 * EPS[dt] * span, (d_pf, d_lp, span)


@pytest.mark.parametrize("dt", DTYPES)
def test_unprompted_decode_is_untouched_by_the_prefill_option(tiny, engines, dt):
    """A decode without prompt_ids must not engage the prefill, also with a 4-token input (<|0.00|> forced behind the init
    tokens): tokens, lengths, argmax and timestamps are bit-identical with prompt_prefill on and off."""
    g, v, W, spec = tiny
    clips = [syn.synth_audio(500 + i, 480000, "mixed") for i in range(8)]
    e = engines[dt]
    for init in ([v.sot, v.lang_id("en"), v.transcribe], [v.sot, v.lang_id("en"), v.transcribe, v.timestamp_begin]):
        n = len(init)
        prompt = np.tile(np.array([init], np.int32), (8, 1))
        outs = []
        for pf in (True, False):
            e.set_prompt_prefill(pf)
            e.mel(clips)
            e.encode(list(range(8)), [0] * 8, [3000] * 8)
            seqs, lens, amax = e.decode(prompt, max_length=n + 40, min_new_tokens=40, want_argmax=True)
            outs.append((seqs, lens, amax, e.alignment(8, n + 40 - 1), e.token_timestamps(8, n + 40 - 1, n, [3000] * 8)))
        e.set_prompt_prefill(True)
        for a, b in zip(*outs):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
