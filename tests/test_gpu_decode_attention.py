"""GPU tests of the decode self-attention (csrc/attention.hip: attn_decode_kernel<T, ANC, PRE>, attn_decode_anc_kernel, chosen by
cw_launch_attn_decode) against float64 softmax attention, and of the beam-search cache ancestry (beam_gather_kernel /
beam_commit_kernel) against a host model of transformers' cache reordering.

Every launch goes through cw_test_self_attention, which fills DecAttnParams the way decode_step does and calls the dispatcher,
so the kernel choice is under test too.

The reference.  K and V are rounded to the engine dtype (through torch) before they reach both the kernel and the reference;
q is f32 in both.  The kernel's only departure from float64 is then its f32 arithmetic, bounded per query row b by

    |out - ref| <= max|v| * u * (22 A + 2 R + 124),    u = 2^-24,

  A = max over the row's keys of sum_e |q_e k_e|, R = range of its scores.  The terms:
  * score: 8 chained fmas per lane + 3 butterfly adds, |ds_k| <= 11 u A_k (gamma_11);
  * s_k - max rounds once (u R) and expf is within 2 ulp: every probability carries a relative error
    |eps_k| <= 11 u A + u R + 2 u, and sum_k p_k (eps_k - mean eps) v_k moves the output by at most 2 max|eps| max|v|;
  * the probability sum (<= 3 terms per thread, 6 butterfly levels, 8 waves: <= 17 roundings) and the weighted sum of V
    (<= 24 fmas per 8-lane group at 1500 keys, then 64 groups added serially: <= 90 roundings), plus the 1 / sum and its
    product: <= 110 u max|v| together; 124 leaves 14 u of slack for the gamma_n ~ n u approximations.
At the scores used here (|s| <= ~30, A <= ~30) this is 2e-5 .. 5e-5 x max|v|, the same for the f32, bf16 and f16 engines.
An indexing error -- a key counted twice, a key dropped, a stale or wrong-ancestor row read -- is O(p_key) x |v|: the
inputs make it O(1) by giving some rows a sharp peak on a chosen key (q proportional to K[key]) at the boundaries where the
kernels change path (keys 0, 63 / 64, 127 / 128 / 129, the last key), and cache rows nobody may read hold NaN / Inf."""
import os

import numpy as np
import pytest
import torch

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = ["f32", "bf16", "f16"]
HISTS = [1, 2, 63, 64, 65, 127, 128, 129, 130, 255, 256, 383, 384, 385, 447, 448]
PEAKS = [0, 63, 64, 127, 128, 129, -1, None]     # key of a row's sharp peak (-1: its last key; None: no peak)
PEAK_SCORE = 10.0


@pytest.fixture(scope="module")
def engines():
    g, v, W, spec = Hh.tiny_setup()
    out = {dt: Engine(spec, dtype=dt, max_batch=64) for dt in DTYPES}
    yield out
    for e in out.values():
        e.close()


def round16(dt, x):
    """x rounded to the engine's storage type (round-to-nearest-even through torch; NaN / Inf stay), as float32"""
    if dt == "f32":
        return np.asarray(x, np.float32)
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return t.to(torch.bfloat16 if dt == "bf16" else torch.float16).float().numpy()


def histories(cap):
    return sorted({n for n in HISTS if n <= cap} | {cap, cap - 1} - {0})


def kv_inputs(rng, dt, R, H, cap):
    """K / V [R][H][cap][64], distinct per cache row; V with a column-dependent scale (a transposed row cannot pass)"""
    k = rng.standard_normal((R, H, cap, 64)).astype(np.float32)
    v = (rng.standard_normal((R, H, cap, 64)) * np.linspace(0.5, 2.0, 64)).astype(np.float32)
    return round16(dt, k), round16(dt, v)


def queries(rng, keys_of, B, H, peak_shift=0):
    """q [B][H][64] f32: moderate random scores, or a sharp peak (score PEAK_SCORE, the others ~N(0, 1.25^2)) on the key
    PEAKS picks for (b, h).  keys_of(b, h) -> the [n][64] keys row b attends over in head h."""
    q = (rng.standard_normal((B, H, 64)) * 0.35).astype(np.float32)
    for b in range(B):
        for h in range(H):
            kk = keys_of(b, h)
            pk = PEAKS[(b * H + h + peak_shift) % len(PEAKS)]
            if pk is None:
                continue
            pk = len(kk) - 1 if (pk < 0 or pk >= len(kk)) else pk
            kv = kk[pk].astype(np.float64)
            q[b, h] = (PEAK_SCORE * kv / (kv @ kv)).astype(np.float32)
    return q


def reference(q, keys_of, vals_of):
    """float64 softmax attention per row over its own keys; per-row bound of the module docstring"""
    B, H, _ = q.shape
    ref = np.zeros((B, H * 64))
    tol = np.zeros(B)
    for b in range(B):
        A = R = vmax = 0.0
        for h in range(H):
            kk = keys_of(b, h).astype(np.float64)
            vv = vals_of(b, h).astype(np.float64)
            qq = q[b, h].astype(np.float64)
            s = kk @ qq
            p = np.exp(s - s.max())
            p /= p.sum()
            ref[b, h * 64:(h + 1) * 64] = p @ vv
            A = max(A, float(np.abs(kk * qq).sum(-1).max()))
            R = max(R, float(s.max() - s.min()))
            vmax = max(vmax, float(np.abs(vv).max()))
        tol[b] = vmax * U * (22 * A + 2 * R + 124)
    return ref, tol


def check(got, ref, tol, what):
    assert np.isfinite(got).all(), f"{what}: non-finite output in rows {sorted(set(np.where(~np.isfinite(got))[0]))}"
    err = np.abs(got.astype(np.float64) - ref).max(-1)
    bad = np.where(err > tol)[0]
    assert bad.size == 0, f"{what}: rows {bad[:8].tolist()} err {err[bad[:8]].tolist()} > bound {tol[bad[:8]].tolist()}"


def plain_case(rng, dt, B, H, cap, n):
    """per-row histories n[b] over row b's own cache; positions >= n[b] poisoned: K = +-Inf with the signs of the row's query
    (an admitted stale score is +Inf, which no max can ignore the way it ignores a NaN), V = NaN / Inf"""
    k, v = kv_inputs(rng, dt, B, H, cap)
    keys_of = lambda b, h: k[b, h, :n[b]]
    vals_of = lambda b, h: v[b, h, :n[b]]
    q = queries(rng, keys_of, B, H, peak_shift=int(rng.integers(len(PEAKS))))
    for b in range(B):
        k[b, :, n[b]:] = np.copysign(np.float32(np.inf), q[b])[:, None, :]
        v[b, :, n[b]:] = np.nan if b % 2 else np.inf
    return q, k, v, keys_of, vals_of


def anc_case(rng, dt, B, H, cap, n, table="random"):
    """beam layout: key t of row b in cache row anc[b][t]; stale entries (t >= n[b]) stay inside [0, B) as
    beam_gather_kernel writes them; every (cache row, position) no row reads holds NaN / Inf"""
    k, v = kv_inputs(rng, dt, B, H, cap)
    if table == "identity":
        anc = np.tile(np.arange(B, dtype=np.int32)[:, None], (1, cap))
    else:
        anc = rng.integers(0, B, (B, cap)).astype(np.int32)
    used = np.zeros((B, cap), bool)
    for b in range(B):
        used[anc[b, :n[b]], np.arange(n[b])] = True
    k.transpose(0, 2, 1, 3)[~used] = np.nan          # [row][pos][head][64] view
    v.transpose(0, 2, 1, 3)[~used] = np.inf
    keys_of = lambda b, h: k[anc[b, :n[b]], h, np.arange(n[b])]
    vals_of = lambda b, h: v[anc[b, :n[b]], h, np.arange(n[b])]
    q = queries(rng, keys_of, B, H, peak_shift=int(rng.integers(len(PEAKS))))
    return q, k, v, anc, keys_of, vals_of


def row_histories(B, cap, launch):
    """histories of the B rows of launch `launch`: every history of the cap, different per row within one launch"""
    hs = histories(cap)
    return np.array([hs[(launch * B + b) % len(hs)] for b in range(B)], np.int32)


def n_launches(B, cap):
    return -(-len(histories(cap)) // B)


SHAPES = [(1, 1, 448), (5, 2, 448), (8, 20, 448), (40, 2, 448), (64, 2, 448), (64, 1, 100), (40, 20, 100), (5, 2, 20),
          (8, 2, 20)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,cap", SHAPES)
def test_self_attention_against_float64(engines, dt, B, H, cap):
    """Case 1: per-row histories 1 .. 448 (each launch mixes histories: the register path <= 128 keys, the on-demand loop
    above), cap 448 / 100 (not a multiple of 64) / 20 (below 128), against float64 within the derived bound."""
    rng = np.random.default_rng(B * 7919 + H * 31 + cap)
    for launch in range(n_launches(B, cap)):
        n = row_histories(B, cap, launch)
        q, k, v, keys_of, vals_of = plain_case(rng, dt, B, H, cap, n)
        ref, tol = reference(q, keys_of, vals_of)
        got = engines[dt].test_self_attention(q.reshape(B, -1), k, v, n - 1)
        check(got, ref, tol, f"{dt} B={B} H={H} cap={cap} histories {n.tolist()}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("anc", [False, True])
def test_a_single_key_returns_its_value_row_exactly(engines, dt, anc):
    """Case 2: one key: the softmax weight is exp(0) / 1 = 1, so the output is V[key] bit for bit (plain and ANC kernels,
    with and without the <= 64-key hint)."""
    rng = np.random.default_rng(3)
    B, H, cap = 9, 2, 448
    k, v = kv_inputs(rng, dt, B, H, cap)
    k[:, :, 1:] = np.nan
    v[:, :, 1:] = np.inf
    a = rng.integers(0, B, (B, cap)).astype(np.int32) if anc else None
    src = a[:, 0] if anc else np.arange(B)
    q = (rng.standard_normal((B, H * 64)) * 0.35).astype(np.float32)
    want = v[src, :, 0].reshape(B, H * 64)
    for sh in (False, True):
        got = engines[dt].test_self_attention(q, k, v, np.zeros(B, np.int32), anc=a, short_hist=sh)
        assert np.array_equal(got, want), (dt, anc, sh, np.abs(got - want).max())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("anc", [False, True])
def test_short_history_hint(engines, dt, anc):
    """Case 3: short_hist (PRE = 1, 64 history rows requested up front per (row, head)).  Rows of <= 64 keys: bit-identical
    to the hint being off (attention.hip: the PRE = 2 form masks its second key per group out).  A wrong hint (rows of
    65 .. 448 keys): within the bound -- the keys beyond 64 take the on-demand path."""
    rng = np.random.default_rng(11 + anc)
    B, H, cap = 24, 2, 448
    short = np.array([[1, 2, 17, 33, 63, 64][b % 6] for b in range(B)], np.int32)
    longer = np.array([[65, 100, 127, 128, 129, 255, 447, 448][b % 8] for b in range(B)], np.int32)
    for n, exact in ((short, True), (longer, False)):
        if anc:
            q, k, v, a, keys_of, vals_of = anc_case(rng, dt, B, H, cap, n)
        else:
            (q, k, v, keys_of, vals_of), a = plain_case(rng, dt, B, H, cap, n), None
        off = engines[dt].test_self_attention(q.reshape(B, -1), k, v, n - 1, anc=a, short_hist=False)
        on = engines[dt].test_self_attention(q.reshape(B, -1), k, v, n - 1, anc=a, short_hist=True)
        ref, tol = reference(q, keys_of, vals_of)
        check(on, ref, tol, f"{dt} anc={anc} short_hist on, histories {n.tolist()}")
        check(off, ref, tol, f"{dt} anc={anc} short_hist off, histories {n.tolist()}")
        if exact:
            assert np.array_equal(on, off), (dt, anc, np.abs(on - off).max())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("B", [5, 40])
@pytest.mark.parametrize("anc", [False, True])
def test_fragment_major_output(engines, dt, B, anc):
    """Case 4: out_frag -- the 16-bit MFMA fragment-major output the next GEMV reads -- equals the 16-bit rounding of the f32
    output of the same launch parameters, bit for bit, on all three write sites (register path, on-demand loop, serial ANC
    kernel); the padding rows B .. 16k of the fragment buffer stay untouched (B = 5 and 40 are not multiples of 16)."""
    rng = np.random.default_rng(B + 100 * anc)
    H, cap = 2, 448
    n = row_histories(B, cap, 0)
    if anc:
        q, k, v, a, keys_of, vals_of = anc_case(rng, dt, B, H, cap, n)
    else:
        (q, k, v, keys_of, vals_of), a = plain_case(rng, dt, B, H, cap, n), None
    ref, tol = reference(q, keys_of, vals_of)
    for sh in (False, True):
        f32 = engines[dt].test_self_attention(q.reshape(B, -1), k, v, n - 1, anc=a, short_hist=sh)
        check(f32, ref, tol, f"{dt} B={B} anc={anc}")
        frag, tail_ok = engines[dt].test_self_attention(q.reshape(B, -1), k, v, n - 1, anc=a, short_hist=sh, out_frag=True)
        assert tail_ok, "fragment rows >= B were written"
        assert np.array_equal(frag, round16(dt, f32)), (dt, B, anc, sh, np.abs(frag - round16(dt, f32)).max())


ANC_SHAPES = [(5, 2, 448), (8, 20, 448), (40, 2, 448), (64, 2, 448), (40, 2, 100), (5, 2, 20)]


def _anc_body(engines, dt, B, H, cap, table):
    rng = np.random.default_rng(B * 131 + H * 7 + cap + (table == "identity"))
    for launch in range(n_launches(B, cap)):
        n = row_histories(B, cap, launch)
        q, k, v, a, keys_of, vals_of = anc_case(rng, dt, B, H, cap, n, table)
        ref, tol = reference(q, keys_of, vals_of)
        got = engines[dt].test_self_attention(q.reshape(B, -1), k, v, n - 1, anc=a)
        check(got, ref, tol, f"{dt} B={B} H={H} cap={cap} {table} table, histories {n.tolist()}")
        if table == "identity":
            plain = engines[dt].test_self_attention(q.reshape(B, -1), k, v, n - 1)
            check(plain, ref, tol, f"{dt} plain kernel, histories {n.tolist()}")
            short = n <= 128                  # <= 128 keys: the same register-resident arithmetic, loads one table lookup deeper
            assert np.array_equal(got[short], plain[short]), (dt, B, np.abs(got[short] - plain[short]).max())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,cap", ANC_SHAPES)
@pytest.mark.parametrize("table", ["random", "identity"])
def test_ancestry_indexed_self_attention(engines, dt, B, H, cap, table):
    """Case 5: the beam layout.  Random ancestor tables within [0, B), K/V distinct per cache row, every history (beyond 128
    keys: attn_decode_anc), within the bound.  Identity table: bit-identical with the plain kernel for <= 128 keys."""
    if os.environ.get("CW_ANC_ATTN_V1"):
        pytest.skip("default kernel choice: the serial-kernel process runs test_ancestry_through_the_serial_kernel")
    _anc_body(engines, dt, B, H, cap, table)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,cap", [(5, 2, 448), (40, 2, 100), (8, 20, 448)])
def test_ancestry_through_the_serial_kernel(request, engines, dt, B, H, cap):
    """Case 5, CW_ANC_ATTN_V1=1 (attn_decode_anc_kernel for every history; the switch is read once per process, so the cases
    run in a child process): random tables within the same bound."""
    if not os.environ.get("CW_ANC_ATTN_V1"):
        return Hh.run_in_child(request, {"CW_ANC_ATTN_V1": "1"}, lambda p: True)
    _anc_body(engines, dt, B, H, cap, "random")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,kv_div,n_keys", [(4, 1, 1500), (10, 5, 1500), (10, 5, 1000), (3, 1, 77)])
def test_fixed_key_count_with_alignment_capture(engines, dt, B, kv_div, n_keys):
    """Case 6: the f32 engine's cross-attention form (and the non-fused path): a fixed n_keys over a 1500-row cache shared by
    kv_div rows, alignment capture on one head.  Output within the bound; the captured row pos[b] equals the float64
    probabilities to 1e-6 (q scaled so that no probability exceeds ~0.05: the bound times p stays below that); every other
    alignment row is untouched, and heads without a slot write none; short_hist is ignored while capture is on.  Keys
    n_keys .. 1499 are poisoned."""
    rng = np.random.default_rng(B * 10 + kv_div + n_keys)
    H, cap, rows = 2, 1500, 24
    Bk = B // kv_div
    k, v = kv_inputs(rng, dt, Bk, H, cap)
    keys_of = lambda b, h: k[b // kv_div, h, :n_keys]
    vals_of = lambda b, h: v[b // kv_div, h, :n_keys]
    q = (rng.standard_normal((B, H, 64)) * 0.2).astype(np.float32)
    k[:, :, n_keys:] = np.copysign(np.float32(np.inf), q[::kv_div])[:, :, None, :]
    v[:, :, n_keys:] = np.nan
    ref, tol = reference(q, keys_of, vals_of)
    pos = rng.permutation(rows)[:B].astype(np.int32)
    init = np.full((B, rows, n_keys), -7.0, np.float32)
    head = H - 1
    res = {}
    for sh in (False, True):
        res[sh] = engines[dt].test_self_attention(q.reshape(B, -1), k, v, pos, n_keys=n_keys, kv_div=kv_div, short_hist=sh,
                                                  align_head=head, align_rows=rows, align_init=init)
    (out, al), (out1, al1) = res[False], res[True]
    check(out, ref, tol, f"{dt} B={B} kv_div={kv_div} n_keys={n_keys}")
    assert np.array_equal(out, out1) and np.array_equal(al, al1), "short_hist changed a launch with alignment capture"
    for b in range(B):
        s = keys_of(b, head).astype(np.float64) @ q[b, head].astype(np.float64)
        p = np.exp(s - s.max()); p /= p.sum()
        assert np.abs(al[b, pos[b]] - p).max() < 1e-6, (dt, b, np.abs(al[b, pos[b]] - p).max())
        other = np.ones(rows, bool); other[pos[b]] = False
        assert (al[b, other] == -7.0).all(), f"row {b}: alignment rows other than pos[b] = {pos[b]} written"
    # without capture: the plain form of the same launch, same bound
    plain = engines[dt].test_self_attention(q.reshape(B, -1), k, v, pos, n_keys=n_keys, kv_div=kv_div)
    check(plain, ref, tol, f"{dt} B={B} kv_div={kv_div} n_keys={n_keys} no capture")


# ------------------------------------------------------------------------------------------------ beam ancestry end to end

def _parents(rng, step, items, K):
    kind = step % 4 if step < 8 else int(rng.integers(4))
    par = np.zeros(items * K, np.int32)
    for i in range(items):
        base = i * K
        if kind == 0:                                    # identity
            par[base:base + K] = base + np.arange(K)
        elif kind == 1:                                  # every hypothesis from one beam
            par[base:base + K] = base + int(rng.integers(K))
        elif kind == 2:                                  # rotation
            par[base:base + K] = base + (np.arange(K) + 1 + i) % K
        else:                                            # random within the item
            par[base:base + K] = base + rng.integers(0, K, K)
    return par


@pytest.mark.parametrize("dt", DTYPES)
def test_beam_ancestry_end_to_end(dt):
    """Case 7: cw_beam_begin on 3 items x 5 beams, then 200 scripted cw_beam_advance calls (identity, all from one beam,
    rotation, random within the item), so histories cross 128 keys.  After every step the device state read back by
    cw_test_beam_state equals a host model of transformers' reorder_cache exactly:
        ids'[r] = ids[p][:t] ++ [token] ++ ids[r][t+1:],  anc'[r] = anc[p][:t-1] ++ [p] ++ [r]*,  pos' = pos + 1.
    At several steps the read-back table drives cw_test_self_attention over K/V in which cache row c at position k holds what
    the hypothesis in slot c wrote at step k, against float64 attention over a PHYSICALLY reordered host copy of the cache
    (every step: rows copied from their parents, as HF's cache.reorder_cache does).
    The advances then go on to the end of the position table (446 in all, the same state checks after each).  At a handful of
    steps, the first and the last among them, the next-step embedding rows beam_commit_kernel wrote (cw_test_beam_x) are held
    bit for bit to embed[token[r]] + pos_embed[t] from the loaded weights: the f32 sum on the f32 engine; on the 16-bit engines
    the embedding row rounded to the 16-bit type, the f32 sum, then the 2^-12 residual grid (tests/beam_refs.py: resid_grid,
    shown exact on the CPU by tests/test_beam_refs.py).  The advance to t == max_target_positions leaves the rows untouched."""
    from tests.beam_refs import resid_grid
    g, v, W, spec = Hh.tiny_setup()
    embed = round16(dt, W["model.decoder.embed_tokens.weight"])
    pos_embed = np.asarray(W["model.decoder.embed_positions.weight"], np.float32)
    items, K, H = 3, 5, 2
    R, TGT = items * K, spec.max_target_positions
    rng = np.random.default_rng(17)
    eng = Engine(spec, dtype=dt, max_batch=R)
    try:
        eng.load_state_dict(W)
        eng.mel([syn.synth_audio(60 + i, 160000, "mixed") for i in range(items)])
        eng.encode(list(range(items)), [0] * items, [3000] * items)
        prompt = np.array([[v.sot, v.lang_id("en"), v.transcribe]] * items, np.int32)
        n_prompt = prompt.shape[1]
        eng.beam_begin(prompt, K, TGT)
        ids = np.full((R, TGT), spec.pad_token_id, np.int32)
        ids[:, :n_prompt] = np.repeat(prompt, K, axis=0)
        anc = np.tile(np.arange(R, dtype=np.int32)[:, None], (1, TGT))
        pos = n_prompt - 1
        kdev, vdev = kv_inputs(rng, dt, R, H, TGT)       # what slot c writes at position k
        kphys, vphys = kdev.copy(), vdev.copy()           # host caches, reordered by copying rows
        d_ids, d_anc, d_pos = eng.test_beam_state(R)
        assert np.array_equal(d_ids, ids) and np.array_equal(d_anc, anc) and (d_pos == pos).all()
        checks = x_checks = 0
        x_prev = None
        n_steps = TGT - n_prompt + 1                      # the last advance has t == max_target_positions
        for step in range(n_steps):
            par = _parents(rng, step, items, K)
            tok = rng.integers(0, v.size, R).astype(np.int32)
            kphys[:, :, pos] = kdev[:, :, pos]            # the decode step at `pos` writes every row's own slot
            vphys[:, :, pos] = vdev[:, :, pos]
            eng.beam_advance(par, tok)
            t = pos + 1
            new_ids = ids.copy()
            new_anc = np.empty_like(anc)
            for r in range(R):
                p = par[r]
                new_ids[r, :t] = ids[p, :t]
                if t < TGT:
                    new_ids[r, t] = tok[r]
                new_anc[r, :t - 1] = anc[p, :t - 1]
                new_anc[r, t - 1] = p
                new_anc[r, t:] = r
            ids, anc, pos = new_ids, new_anc, t
            kphys, vphys = kphys[par], vphys[par]
            d_ids, d_anc, d_pos = eng.test_beam_state(R)
            assert (d_pos == pos).all(), (step, d_pos.tolist(), pos)
            assert np.array_equal(d_anc, anc), (step, np.argwhere(d_anc != anc)[:5].tolist())
            assert np.array_equal(d_ids, ids), (step, np.argwhere(d_ids != ids)[:5].tolist())
            if step in (0, 1, 40, 128, 199, n_steps - 3, n_steps - 2, n_steps - 1):
                x_checks += 1
                x = eng.test_beam_x(R)
                if t < TGT:
                    s64 = embed[tok].astype(np.float64) + pos_embed[t].astype(np.float64)
                    want = embed[tok] + pos_embed[t]                      # the f32 sum is the float64 sum rounded once
                    assert want.dtype == np.float32 and np.array_equal(want, s64.astype(np.float32))
                    if dt != "f32":
                        want = resid_grid(want)
                    assert x.tobytes() == want.tobytes(), (dt, step, np.argwhere(x != want)[:5].tolist())
                else:                                     # nothing to feed at a position the table does not have
                    assert step == n_steps - 1 and x.tobytes() == x_prev.tobytes(), (dt, step)
                x_prev = x
            if step == 199:
                assert checks == 5 and pos == n_prompt - 1 + 200
            if step in (40, 125, 126, 127, 128, 199):
                checks += 1
                kc, vc = kphys.copy(), vphys.copy()
                kc[:, :, pos] = kdev[:, :, pos]           # key `pos` is the row's own, written by the coming step
                vc[:, :, pos] = vdev[:, :, pos]
                # rows attend over the full history or a prefix of it (the table's prefix is the prefix's ancestry)
                n = np.array([[pos + 1, pos + 1, min(pos + 1, 128), min(pos + 1, 129), min(pos + 1, 64)][r % 5]
                              for r in range(R)], np.int32)
                keys_of = lambda b, h: kc[b, h, :n[b]]
                vals_of = lambda b, h: vc[b, h, :n[b]]
                kd, vd = kdev.copy(), vdev.copy()
                used = np.zeros((R, TGT), bool)
                for b in range(R):
                    used[d_anc[b, :n[b]], np.arange(n[b])] = True
                kd.transpose(0, 2, 1, 3)[~used] = np.nan
                vd.transpose(0, 2, 1, 3)[~used] = np.inf
                q = queries(rng, keys_of, R, H, peak_shift=step)
                ref, tol = reference(q, keys_of, vals_of)
                got = eng.test_self_attention(q.reshape(R, -1), kd, vd, n - 1, anc=d_anc)
                check(got, ref, tol, f"{dt} step {step} histories {n.tolist()}")
        assert checks == 6 and x_checks == 8 and pos == TGT
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ ABI

def test_self_attention_hook_rejects_what_would_address_outside_the_buffers(engines):
    """Case 8: the hook validates on the host before any launch: n_keys > cap, pos outside [0, cap), ancestors (at
    positions <= pos[b]) outside [0, B), anc with kv_div > 1 / a fixed n_keys / alignment capture, capture without a fixed
    key count or with pos[b] >= align_rows; cw_test_beam_state before cw_beam_begin."""
    e = engines["f32"]
    B, H, cap = 4, 1, 16
    q = np.zeros((B, 64), np.float32)
    kv = np.zeros((B, H, cap, 64), np.float32)
    pos = np.full(B, 3, np.int32)
    anc = np.zeros((B, cap), np.int32)
    assert np.isfinite(e.test_self_attention(q, kv, kv, pos, anc=anc)).all()      # the valid call the variants below break
    bad = [dict(pos=pos, n_keys=cap + 1), dict(pos=np.array([3, 3, cap, 3])), dict(pos=np.array([3, -1, 3, 3])),
           dict(pos=pos, anc=np.where(np.arange(cap) == 3, B, 0).astype(np.int32)[None].repeat(B, 0)),
           dict(pos=pos, anc=np.full((B, cap), -1, np.int32)),
           dict(pos=pos, anc=anc, n_keys=8), dict(pos=pos, anc=anc, align_head=0, align_rows=8),
           dict(pos=pos, align_head=0, align_rows=8), dict(pos=pos, n_keys=8, align_head=0, align_rows=3),
           dict(pos=pos, n_keys=8, align_head=H, align_rows=8)]
    for kw in bad:
        p = kw.pop("pos")
        with pytest.raises(EngineError):
            e.test_self_attention(q, kv, kv, p, **kw)
    kv2 = np.zeros((B // 2, H, cap, 64), np.float32)
    with pytest.raises(EngineError):
        e.test_self_attention(q, kv2, kv2, pos, anc=anc, kv_div=2)
    with pytest.raises(EngineError):
        e.test_beam_state(4)
