"""Host-side proof that the comparisons of tests/test_gpu_decode_stages.py bite (no GPU): "kernel outputs" with one planted fault,
made in numpy from the GPU tests' own inputs, must fail the comparators of tests/decode_stage_refs.py; the float32 restatement of
the right formula must pass them; and the exact-operand builders are exact -- float32 in two summation orders and float64 agree
bit for bit."""
import numpy as np
import pytest

from tests import decode_stage_refs as R
from tests import test_gpu_decode_stages as G

DTS = G.DTS
F = np.float32


def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


# ---- folds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", R.FOLD_LN_SCALES)
@pytest.mark.parametrize("N,K", R.FOLD_LN_SHAPES)
def test_fold_layernorm_dyadic_is_exact_and_gauss_restatement_passes(N, K, scale):
    W, g, beta, b0 = R.fold_ln_inputs("dyadic", N, K)
    ref_w, ref_b = R.fold_layernorm64(W, g, beta, scale, b0)
    for dt in DTS:
        assert np.array_equal(R.round16(dt, ref_w), ref_w)
    p = (W.astype(F) * beta.astype(F)).astype(F)
    for order in (p, p[:, ::-1]):                                           # the bias sum in f32, two orders
        assert np.array_equal(b0.astype(F) + F(scale) * np.cumsum(order, -1, dtype=F)[:, -1], ref_b)
    W, g, beta, b0 = R.fold_ln_inputs("gauss", N, K)
    ref_w, ref_b = R.fold_layernorm64(W, g, beta, scale, b0)
    w32 = ((F(scale) * W.astype(F)).astype(F) * g.astype(F)).astype(F)      # the kernel's scale * w * gamma
    b32 = b0.astype(F) + F(scale) * np.cumsum((W.astype(F) * beta.astype(F)).astype(F), -1, dtype=F)[:, -1]
    for dt in DTS:
        R.assert_fold16(dt, R.round16(dt, w32), ref_w, R.fold_ulp_cap(dt, 2))
        R.assert_within(b32, ref_b, R.fold_ln_bias_bound(W, beta, scale, ref_b))


@pytest.mark.parametrize("with_s", [False, True])
@pytest.mark.parametrize("N,J,K", R.FOLD_PRODUCT_SHAPES)
def test_fold_product_dyadic_is_exact_and_gauss_restatement_passes(N, J, K, with_s):
    def chain32(A, s, scale, B):                                            # the kernel's order: one f32 accumulator over j
        a = (A.astype(F) * (F(1) if s is None else s.astype(F))).astype(F) * F(scale)
        acc = np.zeros((N, K), F)
        for j in range(J):
            acc = (acc + (a[:, j:j + 1] * B[j].astype(F)).astype(F)).astype(F)
        return acc
    A, s, B, scale = R.fold_product_inputs("dyadic", N, J, K, with_s)
    ref = R.fold_product64(A, s, scale, B)
    assert np.abs(ref).max() > 0
    for dt in DTS:
        assert np.array_equal(R.round16(dt, ref), ref)
    assert np.array_equal(chain32(A, s, scale, B), ref)
    assert np.array_equal((A.astype(F) * (F(1) if s is None else s.astype(F)) * F(scale)) @ B.astype(F), ref)
    A, s, B, scale = R.fold_product_inputs("gauss", N, J, K, with_s)
    ref = R.fold_product64(A, s, scale, B)
    c32 = chain32(A, s, scale, B)
    for dt in DTS:
        R.assert_fold16(dt, R.round16(dt, c32), ref, R.fold_ulp_cap(dt, np.sqrt(J) + 2))


@pytest.mark.parametrize("kind", ["dyadic", "gauss"])
def test_fold_without_scale_is_rejected(kind):
    for dt in DTS:
        N, K = R.FOLD_LN_SHAPES[1]
        W, g, beta, b0 = R.fold_ln_inputs(kind, N, K)
        ref_w, ref_b = R.fold_layernorm64(W, g, beta, 0.125, b0)
        bad_w, bad_b = R.fold_layernorm64(W, g, beta, 0.125, b0, fault="no_scale")
        if kind == "dyadic":
            _fails(R.assert_equal, R.round16(dt, bad_w), ref_w)
            _fails(R.assert_equal, bad_b, ref_b)
        else:
            _fails(R.assert_fold16, dt, R.round16(dt, bad_w), ref_w, R.fold_ulp_cap(dt, 2))
            _fails(R.assert_within, bad_b, ref_b, R.fold_ln_bias_bound(W, beta, 0.125, ref_b))
        N, J, K = R.FOLD_PRODUCT_SHAPES[1]
        A, s, B, scale = R.fold_product_inputs(kind, N, J, K, True)
        ref, bad = R.fold_product64(A, s, scale, B), R.fold_product64(A, s, scale, B, fault="no_scale")
        if kind == "dyadic":
            _fails(R.assert_equal, R.round16(dt, bad), ref)
        else:
            _fails(R.assert_fold16, dt, R.round16(dt, bad), ref, R.fold_ulp_cap(dt, np.sqrt(J) + 2))
        v = np.random.default_rng(3).standard_normal(J)
        ref, bad = R.fold_rowvec64(A, s, scale, v), R.fold_rowvec64(A, s, scale, v, fault="no_scale")
        _fails(R.assert_within, bad, ref, (J // 64 + 10) * R.U32 * (np.abs(A * s * scale) @ np.abs(v)))


def test_fold16_comparator_counts_positions():
    for dt in DTS:
        x = R.round16(dt, np.linspace(0.3, 3.0, 4096))
        R.assert_fold16(dt, x, x, 0.0)
        up = x + R.ulp16(dt, x)
        _fails(R.assert_fold16, dt, up, x, 0.01)                                # every element one position off: beyond any cap
        two = x.copy()
        two[7] += 2 * R.ulp16(dt, two[7])
        _fails(R.assert_fold16, dt, two, x, 1.0)                                # a single element two positions off
        few = x.copy()
        few[:3] = up[:3]
        R.assert_fold16(dt, few, x, 1e-3)


# ---- fragment-major image ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", R.PACK_SHAPES)
def test_packed_image_formula_and_pad_rows(N, K):
    Np = (N + 15) & ~15
    n, k = np.meshgrid(np.arange(Np), np.arange(K), indexing="ij")
    assert np.array_equal(np.sort(R.frag_index(n, k, K).ravel()), np.arange(Np * K))        # a bijection onto the image
    bits = R.pack_source_bits(N, K)
    for dt in DTS:                                                              # finite, normal, and the value survives f32 -> 16 bit
        v = R.bits16_to_f64(dt, bits)
        assert np.isfinite(v).all() and np.array_equal(R.round16(dt, v), v) and (np.abs(v) >= 2.0 ** (-126 if dt == "bf16" else -14)).all()
    assert (bits[:-1] != bits[1:]).all() and (bits[:, :-1] != bits[:, 1:]).all()
    want = R.wfrag_image(bits, N, K)
    # the wave's view: lane (n & 15) + 16 * ((k & 31) >> 3) of (tile n >> 4, k step k >> 5) holds eight consecutive k
    img = want.reshape(Np // 16, K // 32, 4, 16, 8)
    assert np.array_equal(img[0, 0, 1, min(3, N - 1)], bits[min(3, N - 1), 8:16])
    if N % 16:
        assert np.array_equal(img[-1, -1, 3, 15], bits[N - 1, K - 8:])           # a pad row repeats the last row
        assert (want != R.wfrag_image(bits, N, K, fault="pad_row_zero")).any()
    else:
        assert np.array_equal(want, R.wfrag_image(bits, N, K, fault="pad_row_zero"))


# ---- the stacked GEMV ----------------------------------------------------------------------------------------------------------------
CASES = [(K, "x1") for K in sorted(R.STACK_K)] + [(K, "x2") for K in sorted(R.STACK_X2_TILES)]


def _case(K, layout):
    W, segs, outs = G.exact_case(K, layout)
    return W, segs, outs, outs[0].shape[0]


@pytest.mark.parametrize("K,layout", CASES)
def test_stack_exact_operands_are_exact(K, layout):
    W, segs, outs, rows = _case(K, layout)
    tiles = R.STACK_K[K] if layout == "x1" else R.STACK_X2_TILES[K]
    _, _, extra = R.stack_exact_case(K, tiles, layout, rows=rows)
    for dt in DTS:
        assert np.array_equal(R.round16(dt, W), W)
        for s in segs:
            cen = R.centred_rows(rows) if s.get("wsum") is not None else np.zeros(rows, bool)
            assert np.array_equal(R.round16(dt, s["x"][~cen]), s["x"][~cen])
            if cen.any():                                                       # the offset rows are NOT 16-bit numbers; x - mean is
                assert (R.round16(dt, s["x"][cen]) != s["x"][cen]).mean() > 0.5
                d = s["x"][cen] - R.CENTRE_OFFSET
                assert np.array_equal(R.round16(dt, d), d) and (d.sum(-1) == 0).all() and (np.abs(d) <= 4).all()
        assert R.stack_exactness_margins(dt, W, segs, rows) < 2 ** 24
    r = R.switch_ratio(segs[0]["x"])
    assert ((r < 0.8) | (r > 1.25)).all() and (r > 1.25).sum() == R.centred_rows(rows).sum() and (r < 0.8).any()
    c_w = R.CENTRE_OFFSET * segs[0]["wsum"]
    assert np.array_equal(c_w.astype(F), c_w) and np.array_equal(segs[0]["wsum"], W[:len(c_w)].sum(-1))
    # ties of the residual grid in both directions, resolved onto the 1 / 16 grid
    t0 = (len(W) // 16 - segs[2]["n_tiles"]) * 16
    t = (segs[2]["x"] @ W[t0:].T + segs[2]["bias"]) * 4096
    tie = np.abs(t - np.floor(t) - 0.5) == 0
    assert np.array_equal(tie.any(0), extra["tie_columns"]) and tie.any()
    assert (np.rint(t[tie]) > t[tie]).any() and (np.rint(t[tie]) < t[tie]).any() and (np.rint(t[tie]) % 256 == 0).all()
    for nt in (1, 3):
        ref = R.stack_ref("bf16", W, segs, rows, nt=nt)
        for order in (0, 1):
            got = R.stack_f32_restatement("bf16", W, segs, rows, nt, order)
            for a, b in zip(got, ref):
                assert a["out"].dtype == F and np.array_equal(a["out"], b["out"])
                if "pstats" in b:
                    assert np.array_equal(a["pstats"], b["pstats"])
    assert all((o != R.SENTINEL).all() for o in outs)                           # a sentinel left behind cannot pass for a result


def _differs(a, b):
    return not np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("fault", ["tail_clamped", "pstats_group_stride_16", "wsum_neighbour_tile", "no_centring", "grid_half_away"])
@pytest.mark.parametrize("K", sorted(R.STACK_K))
def test_stack_mutants_are_rejected_by_the_exact_comparison(K, fault):
    W, segs, outs, rows = _case(K, "x1")
    for dt in DTS[:1]:                                                          # the operands are numbers of both types: one answer
        for Mb in (R.STACK_MB if K < 1280 else [1, 9, 17, 64]):
            for nt in (1, 2, 3):
                ref = R.stack_ref(dt, W, segs, Mb, nt=nt)
                bad = R.stack_ref(dt, W, segs, Mb, nt=nt, fault=fault)
                _, snt, _ = R.stack_blocks(nt, [s["n_tiles"] for s in segs], [0, 0, 0])
                hit = {"tail_clamped": segs[2]["n_tiles"] % snt[2] != 0, "pstats_group_stride_16": Mb > 16,
                       "no_centring": Mb > 1, "wsum_neighbour_tile": Mb > 1}.get(fault, True)
                which = 0 if fault in ("wsum_neighbour_tile", "no_centring") else 2
                key = "pstats" if fault == "pstats_group_stride_16" or (fault == "tail_clamped" and Mb == 1) else "out"
                if hit:
                    _fails(R.assert_equal, bad[which][key], ref[which][key])
                    assert _differs(bad[which][key], ref[which][key])
                else:
                    R.assert_equal(bad[which][key], ref[which][key])
    assert any(segs[2]["n_tiles"] % n for n in (2, 3))                          # every K has a tail tile at some nt


@pytest.mark.parametrize("Mb", R.STACK_GAUSS_MB)
@pytest.mark.parametrize("dt", DTS)
def test_stack_gauss_bound_rejects_uncentred_rows_and_passes_float32(dt, Mb):
    W, segs = R.stack_gauss_case(dt, Mb)
    ref = R.stack_ref(dt, W, segs, Mb, nt=1, round_x=False)
    n = segs[0]["n_tiles"] * 16
    bound = R.stack_elem_bound(dt, W[:n], segs[0], Mb, ref[0]["out"])
    cen = R.centred_rows(Mb)
    r = R.switch_ratio(segs[0]["x"])
    assert (r[cen] > 1.25).all() and (r[~cen] < 0.8).all()
    # without centring: x itself rounded to 16 bits
    bad = R.stack_ref(dt, W, segs, Mb, nt=1, fault="no_centring")[0]["out"]
    over = (np.abs(bad - ref[0]["out"]) > bound).any(-1)
    assert over[cen].mean() >= 0.9, (dt, Mb, over[cen].mean())
    assert not over[~cen].any()
    # the neighbouring tile's wsum
    bad = R.stack_ref(dt, W, segs, Mb, nt=1, fault="wsum_neighbour_tile", round_x=False)[0]["out"]
    assert (np.abs(bad - ref[0]["out"]) > bound).any(-1)[cen].all()
    # float32 restatement of the right formula: f32 mean, f32 subtraction, 16-bit rounding, f32 sums in 64-wide pieces
    got = R.stack_f32_restatement(dt, W, segs, Mb, 1, 0)
    for i, (g, rf, s) in enumerate(zip(got, ref, segs)):
        b = R.stack_elem_bound(dt, W[i * n:(i + 1) * n], s, Mb, rf["out"])
        R.assert_within(g["out"], rf["out"], b, f"segment {i}")
        if s["epi"] == 1:
            R.assert_within(g["pstats"], R.planes_of(rf["out"], 16), R.pstats_bound(rf["out"], b, 1, s["n_tiles"], Mb))
            half_away = R.stack_ref(dt, W, segs, Mb, nt=1, fault="grid_half_away", round_x=False)[i]
            R.assert_within(half_away["out"], rf["out"], b)                      # Gaussian sums meet no tie: the exact cases test them


def test_stack_blocks_follow_the_launcher():
    assert R.stack_blocks(0, [80, 80, 80], [0, 0, 0]) == (1, [1, 1, 1], [80, 80, 80])
    assert R.stack_blocks(0, [320, 320, 80], [0, 0, 0]) == (3, [3, 3, 3], [107, 107, 27])
    assert R.stack_blocks(0, [100, 100, 80], [0, 0, 0]) == (2, [2, 2, 2], [50, 50, 40])
    assert R.stack_blocks(3, [80, 80, 80], [0, 1, 2]) == (3, [3, 1, 2], [27, 80, 40])
    assert R.stack_blocks(2, [8, 5, 7], [3, 0, 1]) == (2, [2, 2, 1], [4, 3, 7])


# ---- the finished query --------------------------------------------------------------------------------------------------------------
def _as_readout(q, H):
    B = q.shape[0]
    return np.broadcast_to(q.reshape(B, H, 1, 64), (B, H, 6, 64)).copy()


def test_readout_inverts_the_one_hot_attention():
    rng = np.random.default_rng(5)
    B, H = 3, 2
    q = rng.uniform(-4, 4, (B, H * 64))
    kv = R.onehot_cache(1, H)[0].astype(np.float64)                            # [H][S][64]
    po, ml = np.zeros((6, B, H * 64)), np.zeros((B, H, 6, 2))
    for b in range(B):
        for h in range(H):
            for sp in range(6):
                k = kv[h, sp * 64:(sp + 1) * 64]
                s = k @ q[b, h * 64:(h + 1) * 64]
                p = np.exp(s - s.max())
                po[sp, b, h * 64:(h + 1) * 64] = p @ k
                ml[b, h, sp] = (s.max(), p.sum())
    assert np.abs(R.readout_query(po, ml) - q.reshape(B, H, 1, 64)).max() < 1e-14


CUT_CASES = [("split", B, H, n, cut) for B, H in [(17, 2), (64, 6)] for n, cut in [(65, 64), (80, 64), (128, 64), (128, 96)]] + \
            [("beam", 15, 6, n, 64) for n in (65, 80, 96)] + [("e4m3", B, 6, n, cut) for B in (16, 40) for n, cut in [(65, 64), (128, 64), (128, 96)]]


@pytest.mark.parametrize("path,B,H,n,cut", CUT_CASES)
def test_query_finished_from_too_few_planes_is_rejected(path, B, H, n, cut):
    qa, qb, qw, qbias, ps = R.fused_query_case(B, H, n)
    q64, (mean, var, ex2) = R.finish_query64(qa, qb, qw, qbias, ps, n)
    bad, _ = R.finish_query64(qa, qb, qw, qbias, ps, n, cut=cut)
    for dt in DTS:
        tol = R.fused_query_tol(G.XQ_YARDSTICK[(path, dt)], q64, qbias, var, ex2)
        R.assert_query(_as_readout(q64, H), q64, tol)
        _fails(R.assert_query, _as_readout(bad, H), q64, tol)


@pytest.mark.parametrize("B,H,n", [(1, 2, 1), (17, 2, 65), (64, 20, 80), (48, 6, 96)])
def test_query_case_and_float32_restatement(B, H, n):
    qa, qb, qw, qbias, ps = R.fused_query_case(B, H, n)
    D = H * 64
    q64, (mean, var, ex2) = R.finish_query64(qa, qb, qw, qbias, ps, n)
    assert np.abs(q64).max() <= R.XQ_QMAX
    std = np.sqrt(var)
    off = np.abs(mean) / std
    assert abs(off[B // 2] - 30) < 0.5 and (np.delete(off, B // 2) < 0.06).all()
    assert np.isnan(ps.reshape(-1, n, 16, 2)[-1, :, B % 16 or 16:]).all() and np.isnan(ps).sum() == (-B % 16) * n * 2
    # a wrong group stride, the neighbouring row of the plane, a wrong column's qw: all far outside the tolerance
    tol = R.fused_query_tol(max(G.XQ_YARDSTICK[("split", dt)] for dt in DTS), q64, qbias, var, ex2)
    if B > 1:
        wrong_row, _ = R.finish_query64(qa, qb, qw, qbias, np.roll(ps, 1, axis=2), n)
        _fails(R.assert_query, _as_readout(wrong_row, H), q64, tol)
        wrong_qw, _ = R.finish_query64(qa, qb, np.roll(qw, 1), qbias, ps, n)
        _fails(R.assert_query, _as_readout(wrong_qw, H), q64, tol)
    # the finishing formula in f32, plane sums in two orders: inside the tolerance that a yardstick of 3e-7 (the rounding of a query
    # of magnitude 4 and of its exponential) gives
    f = F
    b = np.arange(B)
    rows = ps.reshape(-1, n, 16, 2)[b >> 4, :, b & 15]                          # [B][n][2]
    for order in (rows, rows[:, ::-1]):
        s = np.cumsum(order, 1, dtype=f)[:, -1]
        m = (s[:, 0] * f(1.0 / D)).astype(f)
        v = np.maximum((s[:, 1] * f(1.0 / D)).astype(f) - (m * m).astype(f), f(0))
        rstd = (f(1) / np.sqrt((v + f(1e-5)).astype(f))).astype(f)
        q32 = ((((qa + qb).astype(f) - (m[:, None] * qw).astype(f)).astype(f) * rstd[:, None]).astype(f) + qbias).astype(f)
        R.assert_query(_as_readout(q32.astype(np.float64), H), q64, R.fused_query_tol(3e-7, q64, qbias, var, ex2))
