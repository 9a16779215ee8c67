"""Per-head forced alignment on the device (cw_align_heads, Engine.align_heads) and its similarity kernel.

The differential tests use no tolerance: row (l, h) of align_heads must equal, bit for bit, align_tokens of an engine of the
same dtype whose only alignment head is (l, h) -- the same launches record the same rows, and the timestamp stage of one head
runs on the same bytes.  The similarity kernel is held to the float64 definition within the bound derived in
tests/align_heads_refs.py."""
import dataclasses

import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import align_heads_models as M
from tests import align_heads_refs as R

pytestmark = pytest.mark.gpu

_SETUPS = {}


def _setup(name):
    if name not in _SETUPS:
        _SETUPS[name] = M.setup(name)
    return _SETUPS[name]


def _engine(spec, W, dtype, rows=4, heads=None):
    if heads is not None:
        spec = dataclasses.replace(spec, alignment_heads=[list(h) for h in heads])
    e = Engine(spec, dtype=dtype, max_batch=rows)
    e.load_state_dict(W)
    return e


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# batches: (clip seconds, row lengths).  Ragged rows of 5 .. 40 ids, 1 and 3 rows, clips of 4 s and 30 s (n_cols 200 / 1500),
# equal and unequal num_frames in a batch
_BATCHES = [([30.0, 4.0, 30.0], [40, 5, 17]), ([4.0, 4.0, 4.0], [9, 40, 9]), ([4.0], [23])]


def _clips(secs, seed=500):
    return [syn.synth_audio(seed + i, int(s * 16000), "mixed") for i, s in enumerate(secs)]


@pytest.mark.parametrize("dtype,prefill", [("f32", True), ("bf16", True), ("f16", True), ("bf16", False)])
@pytest.mark.parametrize("geom", ["tiny", "mid"])
def test_every_head_equals_the_single_head_engine(geom, dtype, prefill):
    g, v, W, spec = _setup(geom)
    heads = M.all_heads(g)
    eng = _engine(spec, W, dtype)
    try:
        eng.set_align_prefill(prefill)
        got, nfs, seqs = [], [], []
        for bi, (secs, lengths) in enumerate(_BATCHES):
            _, nf = eng.mel(_clips(secs))
            s = M.rows(v, lengths, 10 + bi)
            runs = eng.align_prefill_runs()
            got.append(eng.align_heads(nf, s, 3, heads))
            assert eng.align_prefill_runs() - runs == (1 if prefill and dtype != "f32" else 0)
            nfs.append(nf); seqs.append(s)
        assert sorted(nfs[0].tolist())[0] == 400 and sorted(nfs[0].tolist())[-1] == 3000
    finally:
        eng.close()
    for k, head in enumerate(heads):
        one = _engine(spec, W, dtype, heads=[head])
        try:
            one.set_align_prefill(prefill)
            for bi, (secs, lengths) in enumerate(_BATCHES):
                _, nf = one.mel(_clips(secs))
                assert np.array_equal(nf, nfs[bi])
                want = one.align_tokens(nf, seqs[bi], 3)
                for b in range(len(lengths)):
                    assert _same(got[bi][k][b], want[b]), (head, bi, b)
                    assert len(want[b]) == lengths[b]
        finally:
            one.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_subset_order_and_refusals(dtype):
    g, v, W, spec = _setup("mid")
    heads = M.all_heads(g)
    eng = _engine(spec, W, dtype)
    try:
        secs, lengths = _BATCHES[0]
        _, nf = eng.mel(_clips(secs))
        s = M.rows(v, lengths, 10)
        full = eng.align_heads(nf, s, 3, heads)
        pick = [7, 2, 11, 0, 5]                                  # shuffled: neither slot order nor layer order
        sub = eng.align_heads(nf, s, 3, [heads[i] for i in pick])
        for j, i in enumerate(pick):
            for b in range(len(s)):
                assert _same(sub[j][b], full[i][b]), (i, b)
        before = eng.align_tokens(nf, s, 3)
        for bad, word in (([[0, 1], [2, 3], [0, 1]], "twice"), ([[0, 0], [3, 0]], "outside"), ([[0, 4]], "outside"),
                          ([[-1, 0]], "outside")):
            with pytest.raises(EngineError, match=word):
                eng.align_heads(nf, s, 3, bad)
            after = eng.align_tokens(nf, s, 3)                    # the context stays usable, and unchanged
            assert all(_same(a, b) for a, b in zip(before, after))
        with pytest.raises(ValueError, match="pairs"):
            eng.align_heads(nf, s, 3, [])
        import ctypes as C
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        n, stride, table = eng._token_table(s)
        nfa = np.asarray(nf, np.int32)
        l0 = np.zeros(1, np.int32)
        ts = np.zeros((1, len(s), stride), np.float32)
        rb = np.zeros((len(s), stride), np.float32)
        assert eng.lib.cw_align_heads(eng.ctx, len(s), p(nfa), p(table), stride, p(n), 3, 0, p(l0), p(l0), p(ts), None, None, 200, None) != 0
        assert b"n_heads" in eng.lib.cw_last_error(eng.ctx)
        assert eng.lib.cw_align_heads(eng.ctx, len(s), p(nfa), p(table), stride, p(n), 3, 1, p(l0), p(l0), p(ts), p(rb), None, 200, None) != 0
        assert b"go together" in eng.lib.cw_last_error(eng.ctx)
        assert all(_same(a, b) for a, b in zip(before, eng.align_tokens(nf, s, 3)))
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,prefill", [("f32", True), ("bf16", True), ("bf16", False)])
def test_nothing_left_behind(dtype, prefill):
    g, v, W, spec = _setup("mid")
    eng = _engine(spec, W, dtype)
    try:
        eng.set_align_prefill(prefill)
        secs, lengths = _BATCHES[0]
        _, nf = eng.mel(_clips(secs))
        s = M.rows(v, lengths, 10)
        init = np.tile(np.asarray(s[0][:3], np.int32), (3, 1))

        def snapshot():
            ts = eng.align_tokens(nf, s, 3)
            eng.encode([0, 1, 2], [0] * 3, [3000] * 3)
            seq, lens, _ = eng.decode(init, max_length=24)
            gts = eng.token_timestamps(3, int(lens.max()) - 1, 3, nf)
            return ts, seq.copy(), lens.copy(), gts

        a = snapshot()
        eng.align_heads(nf, s, 3, M.all_heads(g))
        with pytest.raises(EngineError, match="retained"):        # no stale rows: refused, not answered from the wrong buffer
            eng.token_timestamps(3, lengths[0] - 1, 3, nf)
        b = snapshot()
        with pytest.raises(EngineError):
            eng.align_heads(nf, s, 3, [[0, 0], [0, 0]])
        with pytest.raises(EngineError):
            eng.align_heads(nf, [np.array(list(s[0][:3]) + [5, v.eos, 6, v.eos])] * 3, 3, [[0, 0]])
        c = snapshot()
        for x in (b, c):
            assert all(_same(p, q) for p, q in zip(a[0], x[0]))
            assert np.array_equal(a[1], x[1]) and np.array_equal(a[2], x[2])
            assert _same(a[3], x[3])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------- similarity kernel
def _softmax_rows(rng, shape, sharp=4.0):
    x = rng.standard_normal(shape) * sharp
    x = np.exp(x - x.max(axis=-1, keepdims=True))
    return (x / x.sum(axis=-1, keepdims=True)).astype(np.float32)


def _similarity_cases():
    """(name, attn [B][Ha][N][S], n_cols [B], ref_begin, ref_end [B][N], clip)"""
    S = 1500
    rng = np.random.default_rng(2024)
    f32 = lambda x: np.asarray(x, np.float32)
    cases = []
    for M_ in (1, 3, 200, 1500):                                  # random softmax rows at every n_cols, all three clips
        B, Ha, N = 2, 3, 5
        attn = np.zeros((B, Ha, N, S), np.float32)
        attn[..., :M_] = _softmax_rows(rng, (B, Ha, N, M_))
        attn[..., M_:] = 7.0                                      # frames beyond n_cols must not be read into the sums
        hi = M_ * 0.02
        rb = f32(rng.uniform(0, hi, (B, N)))
        re = f32(rb + rng.uniform(0, 0.5, (B, N)))
        for clip in (0, 200, -1):
            cases.append((f"random n_cols={M_} clip={clip}", attn, [M_] * B, rb, re, clip))
    # edges, one row each: B = 1, Ha = 1, N = 12, n_cols 200
    M_, N = 200, 12
    attn = np.zeros((1, 1, N, S), np.float32)
    attn[0, 0, :, :M_] = _softmax_rows(rng, (N, M_), 2.0)
    attn[..., M_:] = 7.0
    nan = np.float32("nan")
    rb = [0.0, 3.5, 4.5, 1.0, 1.0, nan, 1.0, float("inf"), 3.99, 0.013, 2.0, 3.9]
    re = [0.1, 4.0, 5.0, 1.0, 0.5, 1.0, nan, 2.0, 4.07, 0.013, 2.3, 4.2]
    #     0: at frame 0   1: ends at n_cols   2: wholly beyond n_cols (NaN)   3: zero length   4: end before begin (one frame)
    #     5..7: NaN / inf references   8: begins inside, ends beyond n_cols   9: zero length inside frame 0
    attn[0, 0, 10, :M_] = 0.0                                     # 10: an all-zero row (NaN)
    for clip in (0, 200, -1):
        cases.append((f"edges clip={clip}", attn, [M_], f32([rb]), f32([re]), clip))
    # clipping: all of a row's mass on single frames just inside / just outside the window of the interval [2.0, 2.19] s
    # (frames 100 .. 109), and ramps that overlap the clip edge (clip 0 and 2 cut the 4-frame ramp)
    N = 8
    attn = np.zeros((1, 1, N, S), np.float32)
    for t, frames in enumerate([[100 - 1], [100], [109], [110], [100 - 3, 105], [100 - 2, 105], [110 + 1, 105], [110 + 2, 96]]):
        for f in frames:
            attn[0, 0, t, f] = 1.0 / len(frames)
    rb, re = f32([[2.0] * N]), f32([[2.19] * N])
    assert R.interval_frames(rb[0, 0], re[0, 0]) == (100, 110)
    for clip in (0, 1, 2, 3, 200, -1):
        cases.append((f"window clip={clip}", attn, [1500], rb, re, clip))
    return cases


def test_similarity_kernel_vs_float64():
    g, v, W, spec = _setup("tiny")
    eng = _engine(spec, W, "f32", rows=1)
    worst_all = 0.0
    try:
        for name, attn, n_cols, rb, re, clip in _similarity_cases():
            got = eng.test_align_similarity(attn, n_cols, rb, re, clip)
            want, bound = R.similarity_table(attn, n_cols, rb, re, clip)
            ok, worst, msg = R.compare_similarity(got, want, bound)
            print(f"{name}: {msg or 'all NaN'}; finite {int(np.isfinite(want).sum())} of {want.size}")
            worst_all = max(worst_all, worst)
            assert ok, (name, msg)
            if name.startswith("edges"):
                nanrow = np.isnan(want[0, 0])
                assert nanrow[[2, 5, 6, 7, 10]].all() and not nanrow[[0, 1, 3, 4, 8, 9]].any(), nanrow
            if name.startswith("window clip=0"):                  # mass one frame outside the interval: clipped to nothing
                assert np.isnan(want[0, 0, 0]) and np.isnan(want[0, 0, 3]) and want[0, 0, 1] > 0 and want[0, 0, 2] > 0
        print(f"similarity kernel: worst |err| / bound over all cases = {worst_all:.3f}")
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_similarity_of_the_call_equals_the_hook_on_the_rows(dtype):
    g, v, W, spec = _setup("mid")
    heads = [[2, 3], [0, 1], [1, 2]]
    secs, lengths = _BATCHES[0]
    s = M.rows(v, lengths, 10)
    rng = np.random.default_rng(5)
    begin, end = [], []
    for b, n in enumerate(lengths):
        t0 = np.sort(rng.uniform(0, secs[b], n)).astype(np.float32)
        t1 = (t0 + rng.uniform(0.0, 0.4, n)).astype(np.float32)
        t0[5 % n] = np.nan                                        # a token without a reference
        begin.append(t0); end.append(t1)
    eng = _engine(spec, W, dtype)
    try:
        _, nf = eng.mel(_clips(secs))
        ts, sim = eng.align_heads(nf, s, 3, heads, ref=(begin, end), clip_frames=50)
        plain = eng.align_heads(nf, s, 3, heads)
        assert all(_same(ts[k][b], plain[k][b]) for k in range(len(heads)) for b in range(len(s)))
    finally:
        eng.close()
    n_cols = R.ncols_of(nf)
    Lmax = max(lengths) - 1
    hook = _engine(spec, W, "f32", rows=1)                        # any engine runs the hook
    try:
        for k, head in enumerate(heads):
            one = _engine(spec, W, dtype, heads=[head])
            try:
                one.mel(_clips(secs))
                one.align_tokens(nf, s, 3)
                rows = one.alignment(len(s), Lmax)                # [B][1][Lmax][1500], normalised
            finally:
                one.close()
            for b, n in enumerate(lengths):
                L = n - 1
                rb = np.full((1, L), np.nan, np.float32)
                re = rb.copy()
                rb[0, 3:L] = begin[b][3:L]
                re[0, 3:L] = end[b][3:L]
                want = hook.test_align_similarity(rows[b:b + 1, :, :L], [n_cols[b]], rb, re, 50)[0, 0]
                got = sim[k][b]
                assert len(got) == n
                assert np.isnan(got[:3]).all() and np.isnan(got[L])           # init tokens and eos: no row of their own
                if 5 % n >= 3:
                    assert np.isnan(got[5 % n])
                assert _same(got[:L], want), (head, b)
                assert np.isfinite(want[3:L]).sum() >= (L - 3) // 2, (head, b)   # the comparison is not one of NaNs
    finally:
        hook.close()


def test_wide_geometry_slots_beyond_a_small_layer():
    """4 decoder layers x 20 heads, d_model 1280, 2 rows of 40 ids: 80 heads x 2 x 39 rows x 6000 bytes = 37 MB of capture, more
    than the 2-row context's own 3 heads x 2 x 448 rows (16 MB)."""
    g, v, W, spec = _setup("wide")
    secs, lengths = [30.0, 4.0], [40, 40]
    s = M.rows(v, lengths, 77)
    for dtype in ("bf16", "f32"):
        eng = _engine(spec, W, dtype, rows=2)
        try:
            _, nf = eng.mel(_clips(secs))
            full = eng.align_heads(nf, s, 3, M.all_heads(g))
            assert len(full) == 80
        finally:
            eng.close()
        for head in ([0, 0], [1, 19], [3, 7], [3, 19]):
            one = _engine(spec, W, dtype, rows=2, heads=[head])
            try:
                one.mel(_clips(secs))
                want = one.align_tokens(nf, s, 3)
            finally:
                one.close()
            k = head[0] * g.heads + head[1]
            for b in range(2):
                assert _same(full[k][b], want[b]), (dtype, head, b)
