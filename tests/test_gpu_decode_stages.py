"""GPU tests of what the fused layer of the 16-bit decode step stands on, each against a float64 reference of the documented operation
(tests/decode_stage_refs.py; tests/test_decode_stage_refs.py shows on the CPU that every comparison used here rejects a subtly wrong
kernel and that the exact operands are exact):

  * the load-time rewrites fold_layernorm / fold_product / fold_rowvec / wfrag_pack through cw_test_fold;
  * gemv_stack_kernel (csrc/decfuse.hip) through cw_test_gemv_stack, which fills StackParams the way decode_step does: exact operands
    (bit equality on out, out2, the (sum, sum of squares) planes and the cleared buffer, row-major against packed weights included)
    over the three K variants, 2 and 4 rows per wave, row groups, every nt, tail tiles, lighter segments, centred rows and grid ties;
    Gaussian operands within a derived bound;
  * the query the cross-attention kernels finish from those planes (attn_cross_split FUSED, the beam-search matrix-core kernel, the
    e4m3 kernel's two forms) through cw_test_cross_attention_fused, read back exactly through one-hot caches.

Measured readout yardsticks: see XQ_YARDSTICK."""
import functools

import numpy as np
import pytest

from crisperwhisper_amd.engine import Engine, EngineError
from tests import decode_stage_refs as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]
F = np.float32


@pytest.fixture(scope="module")
def engines():
    g, v, W, spec = Hh.tiny_setup()
    out = {dt: Engine(spec, dtype=dt, max_batch=64) for dt in DTS}
    out["f32"] = Engine(spec, dtype="f32", max_batch=2)
    for dt in DTS:
        out[dt + "+e4m3"] = Engine(spec, dtype=dt, max_batch=64, cross_kv_dtype="fp8")
    yield out
    for e in out.values():
        e.close()


def sent(*shape):
    return np.full(shape, R.SENTINEL, F)


# ---- load-time folds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", R.FOLD_LN_SCALES)
@pytest.mark.parametrize("N,K", R.FOLD_LN_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_fold_layernorm(engines, dt, N, K, scale):
    for kind in ("dyadic", "gauss"):
        W, g, beta, b0 = R.fold_ln_inputs(kind, N, K)
        w16, bias = sent(N, K), b0.astype(F)
        engines[dt].test_fold(0, n=N, k=K, scale=scale, a=W, s=g, v=beta, out16=w16, c_out=bias)
        ref_w, ref_b = R.fold_layernorm64(W, g, beta, scale, b0)
        what = f"fold_layernorm {kind} {dt} N={N} K={K} scale={scale}"
        if kind == "dyadic":
            assert np.array_equal(R.round16(dt, ref_w), ref_w)
            R.assert_equal(w16, ref_w, what)
            R.assert_equal(bias, ref_b, what + " bias")
        else:
            R.assert_fold16(dt, w16, ref_w, R.fold_ulp_cap(dt, 2), what)
            R.assert_within(bias, ref_b, R.fold_ln_bias_bound(W, beta, scale, ref_b), what + " bias")


@pytest.mark.parametrize("with_s", [False, True])
@pytest.mark.parametrize("N,J,K", R.FOLD_PRODUCT_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_fold_product(engines, dt, N, J, K, with_s):
    for kind in ("dyadic", "gauss"):
        A, s, B, scale = R.fold_product_inputs(kind, N, J, K, with_s)
        c16 = sent(N, K)
        engines[dt].test_fold(1, n=N, j=J, k=K, scale=scale, a=A, s=s, v=B, out16=c16)
        ref = R.fold_product64(A, s, scale, B)
        what = f"fold_product {kind} {dt} N={N} J={J} K={K} s={with_s}"
        if kind == "dyadic":
            assert np.array_equal(R.round16(dt, ref), ref)
            R.assert_equal(c16, ref, what)
        else:
            R.assert_fold16(dt, c16, ref, R.fold_ulp_cap(dt, np.sqrt(J) + 2), what)


@pytest.mark.parametrize("dt", DTS)
def test_fold_refusals(engines, dt):
    e = engines[dt]
    z = lambda *s: np.zeros(s, F)
    for N, J, K in [(32, 16, 64), (64, 16, 32), (64, 8, 64), (96, 16, 64), (64, 16, 96), (64, 24, 64)]:
        with pytest.raises(EngineError, match="fold_product"):
            e.test_fold(1, n=N, j=J, k=K, a=z(N, J), v=z(J, K), out16=z(N, K))
    with pytest.raises(EngineError, match="fold_layernorm"):
        e.test_fold(0, n=4, k=130, a=z(4, 130), s=z(130), v=z(130), out16=z(4, 130), c_out=z(4))
    with pytest.raises(EngineError, match="wfrag_pack"):
        e.test_fold(3, n=16, k=48, a=z(16, 48), image=np.zeros(16 * 48, np.uint16))
    with pytest.raises(EngineError, match="null buffer"):
        e.test_fold(2, n=4, j=64, a=z(4, 64), v=z(64))                  # no output at all
    with pytest.raises(EngineError, match="null buffer"):
        e.test_fold(2, n=4, j=64, a=z(4, 64), c_out=z(4))               # c without v
    with pytest.raises(EngineError, match="op 7"):
        e.test_fold(7, n=4, j=64)
    with pytest.raises(EngineError, match="16-bit engines only"):
        engines["f32"].test_fold(3, n=16, k=32, a=z(16, 32), image=np.zeros(16 * 32, np.uint16))


@pytest.mark.parametrize("mode", ["c", "w", "cw"])
@pytest.mark.parametrize("J", R.FOLD_ROWVEC_J)
@pytest.mark.parametrize("dt", DTS)
def test_fold_rowvec(engines, dt, J, mode):
    for N in R.FOLD_ROWVEC_N:
        for kind in ("dyadic", "gauss"):
            rng = np.random.default_rng([53, N, J, len(mode), kind == "gauss"])
            if kind == "dyadic":
                A, s, v, w16 = R.dyadic(rng, (N, J)), 2.0 ** rng.integers(-1, 2, J), rng.integers(-8, 9, J) / 4.0, R.dyadic(rng, (N, J))
            else:
                A, s, v, w16 = (rng.standard_normal(sh).astype(F).astype(np.float64) for sh in ((N, J), (J,), (J,), (N, J)))
            if N % 2:
                s = None                                                  # as the row-sum-only calls of load_state_dict
            c, w = (sent(N) if "c" in mode else None), (sent(N) if "w" in mode else None)
            kw = dict(a=A, s=s, v=v) if "c" in mode else {}
            engines[dt].test_fold(2, n=N, j=J, scale=0.125 if "c" in mode else 1.0, w16=w16 if "w" in mode else None, c_out=c, w_out=w, **kw)
            what = f"fold_rowvec {kind} {dt} N={N} J={J} {mode}"
            steps = -(-J // 64) + 10                                      # a lane's chain, the six-level butterfly, the products
            if "c" in mode:
                ref = R.fold_rowvec64(A, s, 0.125, v)
                a_abs = np.abs(A * (1.0 if s is None else s) * 0.125) @ np.abs(v)
                R.assert_equal(c, ref, what) if kind == "dyadic" else R.assert_within(c, ref, steps * R.U32 * a_abs, what)
            if "w" in mode:
                ref = R.rowsum64(dt, w16)
                R.assert_equal(w, ref, what) if kind == "dyadic" else R.assert_within(w, ref, steps * R.U32 * np.abs(R.round16(dt, w16)).sum(-1), what)


@pytest.mark.parametrize("N,K", R.PACK_SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_wfrag_pack_image(engines, dt, N, K):
    bits = R.pack_source_bits(N, K)
    image = np.full(((N + 15) // 16) * 16 * K, 0xA5A5, np.uint16)
    engines[dt].test_fold(3, n=N, k=K, a=R.bits16_to_f64(dt, bits), image=image)
    want = R.wfrag_image(bits, N, K)
    bad = np.flatnonzero(image != want)
    assert bad.size == 0, f"{bad.size} of {image.size} image elements differ, first at {bad[:4].tolist()}"


# ---- the stacked GEMV, exact operands ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def exact_case(K, layout):
    """operands and the float64 results of all 64 rows (rows are independent: a launch of Mb rows gives the first Mb)"""
    tiles = R.STACK_K[K] if layout == "x1" else R.STACK_X2_TILES[K]
    rows = 64 if layout == "x1" else 17
    W, segs, _ = R.stack_exact_case(K, tiles, layout, rows=rows)
    outs = [r["out"] for r in R.stack_ref("bf16", W, segs, rows, nt=1)]       # the operands are exact in both types
    return W, segs, outs


def launch_stack(e, W, segs, Mb, K, nt, wpk, seg_nt=(0, 0, 0), zero_n4=0):
    """-> per segment (out, out2, pstats) as the device left them, the cleared buffer, (snt, blocks)"""
    _, snt, blocks = R.stack_blocks(nt, [s["n_tiles"] for s in segs], list(seg_nt[:len(segs)]))
    groups = (Mb + 15) // 16
    shared, args = {}, []
    for i, s in enumerate(segs):
        n = s["n_tiles"] * 16
        a = {"x": s["x"][:Mb], "bias": s.get("bias"), "wsum": s.get("wsum"), "n_tiles": s["n_tiles"], "nt": seg_nt[i], "epi": s["epi"]}
        if s["epi"] == 2:
            if s["acc"] not in shared:
                shared[s["acc"]] = np.ascontiguousarray(s["out0"][:Mb], F)
            a["out"] = shared[s["acc"]]
        else:
            a["out"] = sent(Mb, n)
        if s["epi"] == 1:
            a["resid"] = s["resid"][:Mb]
            a["out2"] = sent(Mb, n) if s.get("out2") else None
            a["pstats"] = sent(groups, blocks[i], 16, 2) if s.get("planes", True) else None
        args.append(a)
    zero = sent(zero_n4 * 4) if zero_n4 else None
    e.test_gemv_stack(W, args, Mb=Mb, K=K, nt=nt, wpk=wpk, zero=zero)
    return args, zero, (snt, blocks)


def check_exact(args, zero, plan, segs, outs, Mb, what):
    snt, _ = plan
    for i, (a, s) in enumerate(zip(args, segs)):
        R.assert_equal(a["out"], outs[i][:Mb], f"{what} segment {i} out")
        if a.get("out2") is not None:
            R.assert_equal(a["out2"], outs[i][:Mb], f"{what} segment {i} out2")
        if a.get("pstats") is not None:
            R.assert_equal(a["pstats"], R.planes_of(outs[i][:Mb], snt[i] * 16), f"{what} segment {i} pstats")
    if zero is not None:
        R.assert_equal(zero, np.zeros_like(zero), f"{what} zero")


@pytest.mark.parametrize("Mb", R.STACK_MB)
@pytest.mark.parametrize("K", sorted(R.STACK_K))
@pytest.mark.parametrize("dt", DTS)
def test_stack_exact_x1(engines, dt, K, Mb):
    """the engine's X1 layout [W'q ; W'q Wo ; Wo] (epilogues 0, 0, 1): every nt, both weight layouts, and lighter segments"""
    W, segs, outs = exact_case(K, "x1")
    assert (R.switch_ratio(segs[0]["x"]) < 0.8).any() and (R.switch_ratio(segs[0]["x"][:max(Mb, 2)]) > 1.25).any()
    for nt, seg_nt in [(n, (0, 0, 0)) for n in R.STACK_NT] + [(3, (0, 1, 2)), (2, (1, 0, 1)), (3, (2, 2, 2))]:
        got = {}
        for wpk in (False, True):
            args, zero, plan = launch_stack(engines[dt], W, segs, Mb, K, nt, wpk, seg_nt)
            check_exact(args, zero, plan, segs, outs, Mb, f"x1 {dt} K={K} Mb={Mb} nt={nt} seg_nt={seg_nt} wpk={wpk}")
            got[wpk] = args
        for a, b in zip(got[False], got[True]):                          # bit-identical to each other as well
            assert np.array_equal(a["out"], b["out"])
            assert a.get("pstats") is None or np.array_equal(a["pstats"], b["pstats"])


@pytest.mark.parametrize("Mb", [8, 17])
@pytest.mark.parametrize("K", sorted(R.STACK_X2_TILES))
@pytest.mark.parametrize("dt", DTS)
def test_stack_exact_x2(engines, dt, K, Mb):
    """the X2 layout [W'1 ; W'1 Wo_c ; Wo_c] (epilogues 2, 2, 1): two segments accumulate into one buffer, a second copy of the residual
    rows, no planes, and a buffer to clear whose length is no multiple of a block's 256 float4.  720 tiles at K = 1280: nt = 0 is 3."""
    W, segs, outs = exact_case(K, "x2")
    segs = [dict(s) for s in segs]
    segs[2].update(out2=True, planes=False)
    for nt in (0, 2):
        nt_eff, _, blocks = R.stack_blocks(nt, [s["n_tiles"] for s in segs], [0, 0, 0])
        assert nt_eff == (nt or (3 if K == 1280 else 1))
        for wpk in (False, True):
            args, zero, plan = launch_stack(engines[dt], W, segs, Mb, K, nt, wpk, zero_n4=sum(blocks) * 256 - 3)
            check_exact(args, zero, plan, segs, outs, Mb, f"x2 {dt} K={K} Mb={Mb} nt={nt} wpk={wpk}")


@pytest.mark.parametrize("Mb", [8, 33])
@pytest.mark.parametrize("dt", DTS)
def test_stack_exact_one_and_two_segments(engines, dt, Mb):
    K = 384
    W, segs, outs = exact_case(K, "x1")
    t = [s["n_tiles"] * 16 for s in segs]
    for nt in (2, 3):
        for wpk in (False, True):
            args, zero, plan = launch_stack(engines[dt], W[:t[0]], segs[:1], Mb, K, nt, wpk)
            check_exact(args, zero, plan, segs[:1], outs[:1], Mb, f"nseg=1 {dt} Mb={Mb} nt={nt} wpk={wpk}")
            args, zero, plan = launch_stack(engines[dt], W[t[0]:], segs[1:], Mb, K, nt, wpk)
            check_exact(args, zero, plan, segs[1:], outs[1:], Mb, f"nseg=2 {dt} Mb={Mb} nt={nt} wpk={wpk}")


@pytest.mark.parametrize("dt", DTS)
def test_stack_refusals(engines, dt):
    e = engines[dt]
    K = 128
    W, segs, _ = exact_case(K, "x1")
    ok = lambda **kw: launch_stack(e, W, segs, kw.pop("Mb", 4), kw.pop("K", K), kw.pop("nt", 1), False, **kw)
    for bad in (dict(Mb=0), dict(Mb=65), dict(nt=4), dict(nt=-1), dict(seg_nt=(0, 4, 0)), dict(zero_n4=20 * 256 + 1)):
        with pytest.raises(EngineError, match="test_gemv_stack"):
            ok(**bad)
    x = np.zeros((4, K), F)
    seg = lambda **kw: dict({"x": x, "n_tiles": 1, "epi": 0, "out": np.zeros((4, 16), F)}, **kw)
    Wz = np.zeros((16, K), F)
    for bad in (seg(epi=3), seg(epi=1), seg(epi=1, resid=np.zeros((4, 16), F), wsum=np.zeros(16, F)), seg(out2=np.zeros((4, 16), F)),
                seg(n_tiles=0), seg(epi=1, resid=np.zeros((4, 16), F), pstats=np.zeros((1, 2, 16, 2), F))):
        with pytest.raises(EngineError, match="test_gemv_stack"):
            e.test_gemv_stack(Wz, [bad], Mb=4, K=K)
    with pytest.raises(EngineError, match="test_gemv_stack"):
        e.test_gemv_stack(np.zeros((16, 192), F), [seg(x=np.zeros((4, 192), F))], Mb=4, K=192)     # K % 128
    with pytest.raises(EngineError, match="test_gemv_stack"):
        e.test_gemv_stack(np.zeros((16, 1408), F), [seg(x=np.zeros((4, 1408), F))], Mb=4, K=1408)   # K > 1280
    with pytest.raises(EngineError, match="16-bit engines only"):
        engines["f32"].test_gemv_stack(Wz, [seg()], Mb=4, K=K)


# ---- the stacked GEMV, Gaussian operands ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mb", R.STACK_GAUSS_MB)
@pytest.mark.parametrize("dt", DTS)
def test_stack_gauss_x1(engines, dt, Mb):
    """K = 1280, 80 tiles per segment; every element within the derived bound of stack_elem_bound, centred rows against the reference
    on the unrounded x - mean; the planes within what those bounds leave them"""
    W, segs = R.stack_gauss_case(dt, Mb)
    ref = R.stack_ref(dt, W, segs, Mb, nt=1, round_x=False)
    nt = 1 if Mb <= 16 else 2                                            # decode_step's choice
    args, _, (snt, blocks) = launch_stack(engines[dt], W, segs, Mb, 1280, nt, True)
    for i, (a, s, r) in enumerate(zip(args, segs, ref)):
        n = s["n_tiles"] * 16
        bound = R.stack_elem_bound(dt, W[i * n:(i + 1) * n], s, Mb, r["out"])
        R.assert_within(a["out"], r["out"], bound, f"gauss {dt} Mb={Mb} segment {i}")
        if s["epi"] == 1:
            R.assert_within(a["pstats"], R.planes_of(r["out"], snt[i] * 16), R.pstats_bound(r["out"], bound, snt[i], blocks[i], Mb),
                            f"gauss {dt} Mb={Mb} planes")


# ---- the query finished by the cross-attention kernels -------------------------------------------------------------------------------
# Yardstick: the largest error of q_j = m + log(part_o[j]) when a float64-finished query (|q| <= 4, as f32) goes through the existing
# hook cw_test_cross_attention on the same one-hot caches -- the split kernel (kv_div = 1), the beam-search matrix-core kernel
# (kv_div = 5) and the e4m3 kernel (option cross_test_fp8).  Measured on MI355X (test_readout_yardstick re-measures and holds the
# record to it); the fused kernels have to stay within 4 x this + the derived variance term (R.fused_query_tol).
XQ_YARDSTICK = {
    ("split", "bf16"): 4.2e-7, ("split", "f16"): 4.2e-7,    # measured 4.080e-07 / 4.080e-07: the f32 rounding of q, expf and logf
    ("beam", "bf16"): 4.2e-7, ("beam", "f16"): 2.6e-5,      # measured 4.034e-07 / 2.512e-05: the query rides as three 16-bit terms
    ("e4m3", "bf16"): 1.5e-4, ("e4m3", "f16"): 1.5e-4,      # measured 1.488e-04 / 1.488e-04: three e4m3 terms of query and probabilities
}
XQ_CAL = {"split": (16, 1), "beam": (15, 5), "e4m3": (16, 1)}   # path -> (B, kv_div) of the calibration launch (H = 6, 40 plane slots)


def calibrate(engines, path, dt):
    B, kv_div = XQ_CAL[path]
    H = 6
    qa, qb, qw, qbias, ps = R.fused_query_case(B, H, 40, seed=9)
    q64, _ = R.finish_query64(qa, qb, qw, qbias, ps, 40)
    kv = R.onehot_cache(B // kv_div, H)
    e = engines[dt]
    if path == "e4m3":
        assert e.lib.cw_test_set_option(b"cross_test_fp8", 1) == 0
    try:
        po, ml = e.test_cross_attention_raw(q64.astype(F), kv, kv, kv_div=kv_div)
    finally:
        e.lib.cw_test_set_option(b"cross_test_fp8", 0)
    return float(np.abs(R.readout_query(po, ml) - q64.reshape(B, H, 1, 64)).max())


@pytest.mark.parametrize("path", sorted(XQ_CAL))
@pytest.mark.parametrize("dt", DTS)
def test_readout_yardstick(engines, dt, path):
    err = calibrate(engines, path, dt)
    print(f"readout yardstick {path} {dt}: {err:.3e} (recorded {XQ_YARDSTICK[(path, dt)]:.3e})")
    assert err <= XQ_YARDSTICK[(path, dt)]


def check_fused(e, path, dt, B, H, n_pstats, kv_div=1, log=None):
    qa, qb, qw, qbias, ps = R.fused_query_case(B, H, n_pstats)
    q64, (mean, var, ex2) = R.finish_query64(qa, qb, qw, qbias, ps, n_pstats)
    assert np.abs(q64).max() <= R.XQ_QMAX and np.isnan(ps).any() == (B % 16 != 0)
    kv = R.onehot_cache(B // kv_div, H)
    po, ml = e.test_cross_attention_fused(qa, qb, qw, qbias, ps, kv, kv, kv_div=kv_div, fill=np.nan)
    got = R.readout_query(po, ml)
    tol = R.fused_query_tol(XQ_YARDSTICK[(path, dt)], q64, qbias, var, ex2)
    if log is not None:                                                     # (offset row, the other rows): largest error / tolerance
        ratio = (np.abs(got - q64.reshape(B, H, 1, 64)) / tol.reshape(B, H, 1, 64)).reshape(B, -1).max(-1)
        log.append((float(ratio[B // 2]), float(np.delete(ratio, B // 2).max()) if B > 1 else 0.0))
    R.assert_query(got, q64, tol, f"{path} {dt} B={B} H={H} n_pstats={n_pstats} kv_div={kv_div}")


@pytest.mark.parametrize("H", R.XQ_SPLIT_H)
@pytest.mark.parametrize("dt", DTS)
def test_fused_query_split(engines, dt, H):
    """attn_cross_split_kernel<T, 1, true>: one and several row groups, every plane count on both sides of a wave's 64 lanes.
    Largest error / tolerance measured on MI355X (bf16 = f16): 0.49 / 0.81 / 0.93 at H = 2 / 6 / 20, set by the offset row; 0.55 elsewhere"""
    cases = {2: [(B, n) for B in R.XQ_SPLIT_B for n in R.XQ_SPLIT_NP],
             6: [(B, n) for B in R.XQ_SPLIT_B for n in (27, 65)],
             20: [(1, 128), (17, 80), (64, 80)]}[H]
    log = []
    for B, n in cases:
        check_fused(engines[dt], "split", dt, B, H, n, log=log)
    print(f"fused split {dt} H={H}: largest error / tolerance {max(a for a, _ in log):.3f} (offset row) {max(b for _, b in log):.3f} (others)")


@pytest.mark.parametrize("kv_div", R.XQ_BEAM_DIV)
@pytest.mark.parametrize("dt", DTS)
def test_fused_query_beam(engines, dt, kv_div):
    """attn_cross_mfma_kernel<true, true>: the hypotheses of an item in one block, up to 96 plane slots, 97 refused.
    Largest error / tolerance measured on MI355X: bf16 0.90 / 0.66 / 0.81, f16 0.65 / 0.49 / 0.57 at kv_div = 2 / 5 / 16"""
    log = []
    for items in (1, 3):
        for n in R.XQ_BEAM_NP:
            check_fused(engines[dt], "beam", dt, kv_div * items, 20 if (items, n) == (3, 80) else 6, n, kv_div=kv_div, log=log)
    print(f"fused beam {dt} kv_div={kv_div}: largest error / tolerance {max(a for a, _ in log):.3f} (offset row) {max(b for _, b in log):.3f} (others)")
    with pytest.raises(EngineError, match="launch rejected"):
        check_fused(engines[dt], "beam", dt, kv_div, 6, 97, kv_div=kv_div)


@pytest.mark.parametrize("B", [8, 16, 17, 40])
@pytest.mark.parametrize("dt", DTS)
def test_fused_query_e4m3(engines, dt, B):
    """attn_cross_mfma8_kernel FUSED = 1 (<= 16 rows: every wave finishes the query) and 2 (17..64 rows: wave 0 does); the one-hot K / V
    quantise exactly.  Largest error / tolerance measured on MI355X: 0.25 .. 0.35 in both engines"""
    log = []
    for n in (40, 65, 128):
        check_fused(engines[dt + "+e4m3"], "e4m3", dt, B, 6, n, log=log)
    print(f"fused e4m3 {dt} B={B}: largest error / tolerance {max(a for a, _ in log):.3f} (offset row) {max(b for _, b in log):.3f} (others)")


@pytest.mark.parametrize("dt", DTS)
def test_fused_query_refusals(engines, dt):
    e = engines[dt]
    for B, H, n, kv_div in [(65, 2, 8, 1), (4, 2, 0, 1), (4, 2, 129, 1), (6, 2, 8, 4), (4, 21, 8, 1), (34, 2, 8, 17)]:
        qa, qb, qw, qbias, ps = R.fused_query_case(B, H, min(max(n, 1), 128))
        kv = R.onehot_cache(max(B // kv_div, 1), H)
        with pytest.raises(EngineError, match="test_cross_attention_fused"):
            e.test_cross_attention_fused(qa, qb, qw, qbias, ps, kv, kv, kv_div=kv_div, n_pstats=n)
    qa, qb, qw, qbias, ps = R.fused_query_case(4, 2, 8)
    kv = R.onehot_cache(2, 2)
    with pytest.raises(EngineError, match="e4m3 cache"):
        engines[dt + "+e4m3"].test_cross_attention_fused(qa, qb, qw, qbias, ps, kv, kv, kv_div=2)
    with pytest.raises(EngineError, match="16-bit engines only"):
        engines["f32"].test_cross_attention_fused(qa, qb, qw, qbias, ps, R.onehot_cache(4, 2), R.onehot_cache(4, 2))
