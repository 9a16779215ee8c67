"""GPU parity tests, kernel level: every HIP kernel family against the oracle (numpy) on seeded
inputs, through the C ABI.  Integer outputs (DTW paths) must match exactly; floating point within the
tolerance written next to each check."""
import os

import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from oracle import mel as OM
from oracle import model as OMOD
from oracle import pauses as OP
from oracle import timestamps as OT
from tests import helpers as Hh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    g, v, W, spec = Hh.tiny_setup()
    out = {}
    for dt in ("f32", "bf16", "f16"):
        out[dt] = Engine(spec, dtype=dt, max_batch=4)
    yield out
    for e in out.values():
        e.close()


def _round16(dt, *arrs):
    """inputs rounded to the engine's 16-bit type, so the comparison isolates the kernel's own arithmetic"""
    if dt == "bf16":
        return tuple((t.view(np.uint32) & 0xFFFF0000).view(np.float32) for t in arrs)
    if dt == "f16":
        return tuple(t.astype(np.float16).astype(np.float32) for t in arrs)
    return arrs


def rel_err(a, b):
    e = float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))
    log = os.environ.get("CW_TEST_ERRLOG")                       # tolerance audit: CW_TEST_ERRLOG=<file> records every measured error
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{e:.3e}\n")
    return e


# tolerances: 2-3 x the largest error these seeded cases measure on MI355X (CW_TEST_ERRLOG audit, round 5: bf16 3.5e-3 -- the bf16
# rounding of the stored output, 2^-9 of the largest element and up --, f16 4.1e-4, f32 5.9e-7); round 4 carried 2e-2 / 2.5e-3 / 2e-5
@pytest.mark.parametrize("dt,tol", [("f32", 2e-6), ("bf16", 8e-3), ("f16", 1.2e-3)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 200, 128), (1000, 384, 256), (77, 51, 64)])
def test_gemm(engines, dt, tol, M, N, K):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    A, W = _round16(dt, A, W)   # compare against the same 16-bit-rounded operands
    for gelu in (False, True):
        ref = A.astype(np.float64) @ W.astype(np.float64).T + b
        if gelu:
            ref = OMOD.gelu(ref.astype(np.float32)).astype(np.float64)
        got = engines[dt].test_gemm(A, W, b, gelu)
        assert rel_err(got, ref) < tol, (dt, M, N, K, gelu, rel_err(got, ref))


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (1000, 384, 256), (77, 51, 64), (700, 515, 128), (3333, 1280, 1280)])
def test_gemm_256_tile_kernel(engines, M, N, K):
    """The 256x256x64 LDS-DMA GEMM (used from 200 tiles up) forced on for small shapes: interior tiles, M / N edge
    tiles, a row length that is not a multiple of 4 (scalar epilogue), K = 64 (single K-tile) .. 1280."""
    eng = engines["bf16"]
    rng = np.random.default_rng(M * 3 + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    A = (A.view(np.uint32) & 0xFFFF0000).view(np.float32); W = (W.view(np.uint32) & 0xFFFF0000).view(np.float32)
    assert eng.lib.cw_test_set_option(b"gemm256_min_tiles", 1) == 0
    try:
        for gelu in (False, True):
            ref = A.astype(np.float64) @ W.astype(np.float64).T + b
            if gelu:
                ref = OMOD.gelu(ref.astype(np.float32)).astype(np.float64)
            got = eng.test_gemm(A, W, b, gelu)
            assert rel_err(got, ref) < 8e-3, (M, N, K, gelu, rel_err(got, ref))   # measured 2.8e-3 (bf16 output rounding)
    finally:
        eng.lib.cw_test_set_option(b"gemm256_min_tiles", 200)


_e4m3_round = Hh.e4m3_round


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (300, 512, 256), (777, 256, 1280), (1500, 768, 5120)])
def test_gemm_fp8_exact_on_representable_inputs_and_quantisation_model_otherwise(engines, M, N, K):
    """The e4m3 ping-pong GEMM (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales, row scales applied in the epilogue):
    (1) integer operands whose row maximum is 14 quantise without error (scale 2^-5), so the result must equal the integer GEMM
    exactly -- any fragment / k-order / schedule mistake shows; (2) on Gaussian operands the result equals, to f32 accumulation
    accuracy, the f64 GEMM of the operands after the documented quantisation (x -> e4m3(x / s) * s, s = rowmax / 448), i.e. the
    kernel adds nothing beyond the quantisation it is specified to do; 1, 2, 10 and 40 K-tiles, M edge tiles, repeated runs."""
    eng = engines["bf16"]
    rng = np.random.default_rng(M + N + K)
    A = rng.integers(-14, 15, size=(M, K)).astype(np.float32); A[:, 0] = 14
    W = rng.integers(-14, 15, size=(N, K)).astype(np.float32); W[:, 1] = -14
    want = (A.astype(np.int64) @ W.astype(np.int64).T).astype(np.float64)
    for rep in range(3):
        got = eng.test_gemm_fp8(A, W)
        bf = lambda t: (np.asarray(t, np.float32).view(np.uint32) + 0x7FFF + ((np.asarray(t, np.float32).view(np.uint32) >> 16) & 1) & 0xFFFF0000).view(np.float32)
        assert np.array_equal(got, bf(want.astype(np.float32))), (M, N, K, rep, float(np.abs(got - want).max()))   # output is stored in bf16
    A = rng.standard_normal((M, K)).astype(np.float32); W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    (A, W) = _round16("bf16", A, W)
    def q(x):
        s = np.abs(x).max(axis=1, keepdims=True).astype(np.float32) / np.float32(448.0)
        inv = (np.float32(1.0) / s).astype(np.float32)
        return _e4m3_round((x * inv).astype(np.float32)) * s.astype(np.float64)
    ref = q(A) @ q(W).T + b
    got = eng.test_gemm_fp8(A, W, b)
    assert rel_err(got, ref) < 1e-2, (M, N, K, rel_err(got, ref))                       # bf16 output rounding
    exact = A.astype(np.float64) @ W.astype(np.float64).T + b
    assert rel_err(got, exact) < 0.12                                                   # what e4m3 operands cost on N(0, 1) data


@pytest.mark.parametrize("sched", ["pingpong", "8phase", "w128"])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (300, 256, 128), (513, 768, 192), (2000, 512, 5120), (3333, 1280, 1280), (1500, 3840, 1280),
                                   (777, 512, 256), (12000, 1280, 320)])
def test_gemm_pingpong_schedule_is_bit_identical_to_lockstep(request, engines, M, N, K, sched):
    """The staggered 256-tile GEMM schedules -- ping-pong (two wave groups half a K-tile apart, LDS-DMA two tiles ahead) and
    the quarter-tile "8-phase" one (half-tile DMA every phase, counted vmcnt, round 3) -- accumulate in exactly the order of the
    lockstep kernel: same bits, run after run (a half tile overwritten early or read late shows up here), for 1, 2, 3, 4, 5, 20
    and 80 K-tiles, with and without an M-edge tile, also with every CU holding a block (12000 rows).  "w128" (round 4): four
    waves of 128 x 128 per block, self-pipelined in half steps of 32 MFMAs (csrc/gemm_w128.hip)."""
    if sched in ("w128", "pingpong") and not Hh.has_experiments():   # superseded / rejected schedules: -DCW_EXPERIMENTS builds
        return Hh.run_in_child(request, Hh.experiments_env(), lambda p: p["sched"] in ("w128", "pingpong"))
    eng = engines["bf16"]
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    A = (A.view(np.uint32) & 0xFFFF0000).view(np.float32); W = (W.view(np.uint32) & 0xFFFF0000).view(np.float32)
    assert eng.lib.cw_test_set_option(b"gemm256_min_tiles", 1) == 0
    try:
        assert eng.lib.cw_test_set_option(b"gemm_w128", 0) == 0
        assert eng.lib.cw_test_set_option(b"gemm_pp", 0) == 0
        want = eng.test_gemm(A, W, b, True)
        ref = OMOD.gelu((A.astype(np.float64) @ W.astype(np.float64).T + b).astype(np.float32))
        assert rel_err(want, ref) < 8e-3                            # measured 3.8e-3
        assert eng.lib.cw_test_set_option(b"gemm_pp", 1) == 0
        assert eng.lib.cw_test_set_option(b"gemm_8ph", 1 if sched == "8phase" else 0) == 0
        assert eng.lib.cw_test_set_option(b"gemm_w128", 1 if sched == "w128" else 0) == 0
        for rep in range(6):
            got = eng.test_gemm(A, W, b, True)
            assert np.array_equal(got, want), (M, N, K, rep, int((got != want).sum()))
    finally:
        eng.lib.cw_test_set_option(b"gemm256_min_tiles", 200)
        eng.lib.cw_test_set_option(b"gemm_pp", 1)
        eng.lib.cw_test_set_option(b"gemm_8ph", 1)
        eng.lib.cw_test_set_option(b"gemm_w128", 0)


# measured (same audit): bf16 1.9e-3, f16 2.4e-4, f32 2.1e-7
@pytest.mark.parametrize("dt,tol", [("f32", 1e-6), ("bf16", 6e-3), ("f16", 8e-4)])
@pytest.mark.parametrize("Mb,N,K", [(1, 128, 128), (3, 200, 256), (8, 1769, 128), (16, 64, 1280), (20, 128, 512), (40, 96, 1280), (64, 80, 256),
                                     (8, 5120, 1280), (5, 4160, 256), (12, 5120, 1280)])   # the last three: two column tiles per block (wide LayerNorm GEMV)
def test_gemv_with_layernorm(engines, dt, tol, Mb, N, K):
    rng = np.random.default_rng(Mb * 7 + N + K)
    x = (rng.standard_normal((Mb, K)) * 2 + 0.5).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    gam = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32); bet = (0.1 * rng.standard_normal(K)).astype(np.float32)
    (W,) = _round16(dt, W)
    for ln in (None, (gam, bet)):
        for gelu in (False, True):
            xin = x if ln is None else OMOD.layer_norm(x, gam, bet)
            ref = xin.astype(np.float64) @ W.astype(np.float64).T + b
            if gelu:
                ref = OMOD.gelu(ref.astype(np.float32)).astype(np.float64)
            got = engines[dt].test_gemv(x, W, b, ln, gelu)
            assert rel_err(got, ref) < tol, (dt, Mb, N, K, ln is not None, gelu, rel_err(got, ref))

def _ln_plain(x):
    x = x.astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + 1e-5)


@pytest.mark.parametrize("dt,tol", [("bf16", 2e-2), ("f16", 2.5e-3)])
@pytest.mark.parametrize("Mb,N,K,nks", [(17, 384, 128, 0), (20, 128, 512, 4), (33, 256, 256, 2), (40, 1280, 1280, 0), (48, 3840, 1280, 10),
                                         (64, 5120, 1280, 0), (64, 1280, 5120, 16), (64, 1280, 1280, 5), (25, 80, 64, 1), (64, 176, 1280, 8)])
def test_skinny_projections_17_to_64_rows(request, engines, dt, tol, Mb, N, K, nks):
    """Decoder projections of the 17..64-row path (csrc/skinny.hip) against float64: LayerNorm by linearity through K-split
    planes + finish (plain and GELU epilogues) and the residual projection by grid atomics, every supported K split shape,
    ragged row counts, column counts that leave waves / lanes without a tile.  The rows carry a mean 40x their spread (a
    kernel that rounded x to 16 bits before removing the mean loses those 5 bits) and every other row an outlier channel."""
    if not Hh.has_experiments():   # csrc/skinny.hip is an A/B build (measured slower in the step): -DCW_EXPERIMENTS builds
        return Hh.run_in_child(request, Hh.experiments_env(), lambda p: True)
    rng = np.random.default_rng(Mb * 13 + N + K)
    x = (rng.standard_normal((Mb, K)) * 0.5 + rng.uniform(-20, 20, (Mb, 1))).astype(np.float32)
    x[1::2, 7] *= 30.0
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    (W,) = _round16(dt, W)
    eng = engines[dt]
    ref = _ln_plain(x) @ W.astype(np.float64).T + b
    got, _ = eng.test_skinny(0, x, W, b, nks=nks)
    assert rel_err(got, ref) < tol, (dt, Mb, N, K, "ln", rel_err(got, ref))
    S_ = (K // 32) // (nks if nks else 1)
    if nks and S_ <= 16:                                   # LayerNorm statistics combined from the GEMM's K-slice records
        got, _ = eng.test_skinny(4, x, W, b, nks=nks)
        assert rel_err(got, ref) < tol, (dt, Mb, N, K, "ln, slice statistics", rel_err(got, ref))
    if N % 32 == 0:                                         # the GELU epilogue writes MFMA fragments of the next projection (K' = N)
        got, _ = eng.test_skinny(1, x, W, b, nks=nks)
        refg = OMOD.gelu(ref.astype(np.float32)).astype(np.float64)
        assert rel_err(got, refg) < tol, (dt, Mb, N, K, "gelu", rel_err(got, refg))
    # residual projection: activations are 16-bit rows, result on the 2^-12 grid, bit-reproducible
    a = (rng.standard_normal((Mb, K)) * 2).astype(np.float32)
    (a16,) = _round16(dt, a)
    r0 = (np.round(rng.standard_normal((Mb, N)) * 3 * 4096) / 4096).astype(np.float32)
    ref2 = r0 + a16.astype(np.float64) @ W.astype(np.float64).T + b
    got2, _ = eng.test_skinny(2, a16, W, b, out0=r0, nks=nks)
    S = (K // 32) // (nks if nks else 1)
    assert np.abs(got2 - ref2).max() < 2.0 ** -13 * (S + 2) + 1e-5 * np.abs(ref2).max(), (dt, Mb, N, K, np.abs(got2 - ref2).max())
    assert np.all(got2 * 4096 == np.round(got2 * 4096))
    again, _ = eng.test_skinny(2, a16, W, b, out0=r0, nks=nks)
    assert np.array_equal(got2, again)


@pytest.mark.parametrize("dt,tol", [("f32", 2e-5), ("bf16", 2e-2), ("f16", 2.5e-3)])
@pytest.mark.parametrize("B,H,S", [(1, 1, 64), (2, 2, 200), (1, 2, 1500), (2, 3, 257), (1, 1, 1), (3, 5, 511)])
def test_encoder_attention(engines, dt, tol, B, H, S):
    rng = np.random.default_rng(B + H + S)
    q = (rng.standard_normal((B, H, S, 64)) * 0.3).astype(np.float32)
    k = rng.standard_normal((B, H, S, 64)).astype(np.float32)
    v = rng.standard_normal((B, H, S, 64)).astype(np.float32)
    k[0, 0, S // 2] *= 6.0     # one dominant key: forces a running-max jump mid-stream
    q, k, v = _round16(dt, q, k, v)
    s = np.einsum("bhqd,bhkd->bhqk", q.astype(np.float64), k.astype(np.float64))
    p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhqk,bhkd->bhqd", p, v.astype(np.float64)).transpose(0, 2, 1, 3).reshape(B, S, H * 64)
    got = engines[dt].test_attention(q, k, v)
    assert rel_err(got, ref) < tol, (dt, B, H, S, rel_err(got, ref))


@pytest.mark.parametrize("dt,tol", [("bf16", 5e-6), ("f16", 5e-6), ("f32", 5e-6)])
@pytest.mark.parametrize("B,H,S,kv_div,path", [(10, 3, 1500, 5, "mfma"), (10, 3, 1500, 5, "valu"), (4, 2, 1500, 1, "valu"),
                                                (6, 2, 1500, 2, "mfma"), (16, 1, 1500, 16, "mfma"), (9, 2, 750, 3, "mfma"),
                                                (5, 2, 50, 5, "mfma"), (12, 2, 1499, 6, "mfma"), (12, 2, 1499, 6, "valu")])
def test_cross_attention_decode_kernels(engines, dt, tol, B, H, S, kv_div, path):
    """Key-split cross-attention of the decode step: the matrix-core kernel the 16-bit engines use for 2..16 hypotheses per
    K/V and the 8-lane-group kernel (one row per K/V; f32 engine; CW_CROSS_VALU) against float64 softmax attention on the same
    16-bit K/V.  The f32 engine has no matrix-core kernel: with either setting it runs the 8-lane-group kernel, kv_div rows per
    block for 2..6 rows per K/V, one row per block above that (K/V of row b at b / kv_div) -- its "mfma" cases are checked
    against float64 and must be bit-identical to a launch with the switch on.  The query stays f32: the
    matrix-core kernel carries it (and the probabilities) as three 16-bit halves, so
    both kernels are held to an f32 tolerance (5e-6), not a 16-bit one.  S = 50: splits with 9 keys, seven of the eight waves of a block without a key."""
    from crisperwhisper_amd import _native
    if path == "valu" and kv_div > 6:
        pytest.skip("8-lane-group kernel: up to 6 rows per K/V")
    rng = np.random.default_rng(B * 1000 + S + kv_div)
    q = (rng.standard_normal((B, H, 64)) * 0.35).astype(np.float32)
    k = rng.standard_normal((B // kv_div, H, S, 64)).astype(np.float32)
    v = rng.standard_normal((B // kv_div, H, S, 64)).astype(np.float32)
    k[0, 0, S // 3] *= 4.0                       # a dominant key in one split
    v *= np.linspace(0.5, 2.0, 64, dtype=np.float32)    # column-dependent scale: a transposed V fragment cannot pass
    k, v = _round16(dt, k, v)
    kk = np.repeat(k, kv_div, axis=0).astype(np.float64); vv = np.repeat(v, kv_div, axis=0).astype(np.float64)
    s = np.einsum("bhd,bhkd->bhk", q.astype(np.float64), kk)
    p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhk,bhkd->bhd", p, vv).reshape(B, H * 64)
    lib = _native.load()
    assert lib.cw_test_set_option(b"cross_valu", 1 if path == "valu" else 0) == 0
    try:
        got, al = engines[dt].test_cross_attention(q, k, v, kv_div=kv_div, align_head=H - 1)
    finally:
        lib.cw_test_set_option(b"cross_valu", 0)
    assert rel_err(got, ref) < tol, (dt, path, rel_err(got, ref))
    assert np.abs(al - p[:, H - 1]).max() < tol, (dt, path, np.abs(al - p[:, H - 1]).max())
    if dt == "f32" and path == "mfma":               # the f32 engine's kernel selection does not depend on the switch
        assert lib.cw_test_set_option(b"cross_valu", 1) == 0
        try:
            got1, al1 = engines[dt].test_cross_attention(q, k, v, kv_div=kv_div, align_head=H - 1)
        finally:
            lib.cw_test_set_option(b"cross_valu", 0)
        assert np.array_equal(got1, got) and np.array_equal(al1, al)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("path", ["mfma8", "valu"])
@pytest.mark.parametrize("B,H,S,kv_div", [(4, 2, 1500, 1), (10, 3, 1500, 5), (3, 2, 750, 1), (2, 2, 50, 1), (6, 1, 1499, 2)])
def test_cross_attention_over_the_e4m3_cache(request, engines, dt, path, B, H, S, kv_div):
    """Opt-in e4m3 cross-attention cache: quantiser (one scale per (item, head, K|V), amax / 448) + the cross-attention kernel
    over it, against float64 softmax attention on the DEQUANTISED cache -- i.e. the kernels add nothing beyond the quantisation
    they are specified to do.  mfma8: v_mfma_f32_16x16x32_fp8_fp8 with the query and the probabilities carried as three e4m3 terms
    (12 significant bits: tolerance 2e-4 on outputs and alignment probabilities), V read in the fragment-major order the
    quantiser writes; valu (CW_CROSS8_VALU=1 in the process): conversions + f32 FMAs, f32 tolerance.  Column-
    dependent V scale: a transposed or permuted V fragment cannot pass; S = 50: splits of 9 keys, seven waves without a key;
    kv_div: beam rows sharing one cache.  The kernel is chosen once per process: cases of the other kernel run in a child process."""
    import os
    from crisperwhisper_amd import _native
    valu_proc = bool(os.environ.get("CW_CROSS8_VALU"))
    if (path == "valu") != valu_proc:        # the e4m3 kernel / cache layout is chosen once per process (CW_CROSS8_VALU)
        return Hh.run_in_child(request, {"CW_CROSS8_VALU": "1" if path == "valu" else None}, lambda p: p["path"] == path)
    rng = np.random.default_rng(B * 1000 + S + kv_div + 7)
    q = (rng.standard_normal((B, H, 64)) * 0.35).astype(np.float32)
    k = rng.standard_normal((B // kv_div, H, S, 64)).astype(np.float32)
    v = rng.standard_normal((B // kv_div, H, S, 64)).astype(np.float32)
    k[0, 0, S // 3] *= 4.0
    v *= np.linspace(0.5, 2.0, 64, dtype=np.float32)
    k, v = _round16(dt, k, v)
    def deq(x):
        s = (np.abs(x).max(axis=(2, 3), keepdims=True).astype(np.float32) / np.float32(448.0)).astype(np.float32)
        inv = (np.float32(1.0) / s).astype(np.float32)
        return _e4m3_round((x * inv).astype(np.float32)) * s.astype(np.float64)
    kk = np.repeat(deq(k), kv_div, axis=0); vv = np.repeat(deq(v), kv_div, axis=0)
    s = np.einsum("bhd,bhkd->bhk", q.astype(np.float64), kk)
    pr = np.exp(s - s.max(-1, keepdims=True)); pr /= pr.sum(-1, keepdims=True)
    ref = np.einsum("bhk,bhkd->bhd", pr, vv).reshape(B, H * 64)
    lib = _native.load()
    assert lib.cw_test_set_option(b"cross_test_fp8", 1) == 0
    try:
        got, al = engines[dt].test_cross_attention(q, k, v, kv_div=kv_div, align_head=H - 1)
    finally:
        lib.cw_test_set_option(b"cross_test_fp8", 0)
    tol = 2e-4 if path == "mfma8" else 5e-6
    assert rel_err(got, ref) < tol, (dt, path, rel_err(got, ref))
    assert np.abs(al - pr[:, H - 1]).max() < tol, (dt, path, np.abs(al - pr[:, H - 1]).max())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nq,H,S", [(5, 3, 1500), (2, 2, 1499), (3, 1, 50), (4, 2, 750), (8, 2, 1500), (7, 1, 301)])
def test_e4m3_cache_beam_rows_equal_one_row_blocks(engines, dt, nq, H, S):
    """Beam search over the e4m3 cache: attn_cross_mfma8_rows_kernel takes the nq hypotheses of an item in ONE block per (item,
    head, key split) -- four queries x three e4m3 terms per 16-row A tile, a query = a 16-lane row of the C fragment.  Per row it
    is the one-row kernel's arithmetic operation for operation, so the outputs and the captured alignment rows must be
    BIT-identical to a launch in which every row owns a private copy of the cache (kv_div = 1)."""
    import os
    from crisperwhisper_amd import _native
    if os.environ.get("CW_CROSS8_VALU") or os.environ.get("CW_CROSS_PER_ROW"):
        pytest.skip("the rows kernel is the matrix-core path of the default process")
    items = 2
    B = items * nq
    rng = np.random.default_rng(nq * 100 + S + H)
    q = (rng.standard_normal((B, H, 64)) * 0.35).astype(np.float32)
    q[1] *= 6.0                                                   # per-query e4m3 scales differ inside one tile
    k = rng.standard_normal((items, H, S, 64)).astype(np.float32)
    v = (rng.standard_normal((items, H, S, 64)) * np.linspace(0.5, 2.0, 64, dtype=np.float32)).astype(np.float32)
    k, v = _round16(dt, k, v)
    lib = _native.load()
    assert lib.cw_test_set_option(b"cross_test_fp8", 1) == 0
    try:
        got, al = engines[dt].test_cross_attention(q, k, v, kv_div=nq, align_head=H - 1)
        one, al1 = engines[dt].test_cross_attention(q, np.repeat(k, nq, axis=0), np.repeat(v, nq, axis=0), kv_div=1, align_head=H - 1)
    finally:
        lib.cw_test_set_option(b"cross_test_fp8", 0)
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got, one), (dt, nq, S, float(np.abs(got - one).max()))
    assert np.array_equal(al, al1), (dt, nq, S, float(np.abs(al - al1).max()))


def test_cross_attention_rejects_key_counts_that_leave_a_split_empty(engines):
    """7 keys over 6 splits of ceil(7 / 6) = 2: splits 4 and 5 would own no key (the kernels clamp loads to the split's last key);
    the launcher refuses instead of reading in front of the cache."""
    from crisperwhisper_amd.engine import EngineError
    z = np.zeros((2, 1, 64), np.float32)
    kv = np.zeros((2, 1, 7, 64), np.float32)
    with pytest.raises(EngineError):
        engines["bf16"].test_cross_attention(z, kv, kv)


@pytest.mark.parametrize("kind,n", [("noise", 480000), ("mixed", 320000), ("chirp", 480000), ("noise_short", 12345)])
def test_mel_vs_golden_and_oracle(engines, kind, n):
    g = Hh.gold_npz("mel_golden.npz")
    x = syn.synth_audio(1, n, kind.split("_")[0])
    feats, nf = engines["f32"].mel([x], return_features=True)
    assert int(nf[0]) == int(g[f"{kind}_nframes"])
    assert np.abs(feats[0][:, ::5] - g[f"{kind}_feats_sub"]).max() < 1e-4          # vs transformers (golden)
    xp, _ = OM.pad_or_trim(x)
    assert np.abs(feats[0] - OM.log_mel(xp[None], 128)[0]).max() < 1e-4               # vs oracle, full tensor


def test_mel_batch_and_linearity_property(engines):
    """Batch of ragged clips == each clip alone; scaling the waveform by 10 shifts log-mel by 2*log10(10)/4
    away from the floor (size-independent property)."""
    e = engines["f32"]
    clips = [syn.synth_audio(s, n, "noise") for s, n in ((3, 480000), (4, 100000), (5, 1))]
    fb, nfb = e.mel(clips, return_features=True)
    for i, c in enumerate(clips):
        f1, nf1 = e.mel([c], return_features=True)
        assert np.array_equal(f1[0], fb[i]) and nf1[0] == nfb[i]
    f10, _ = e.mel([clips[0] * 10.0], return_features=True)
    d = (f10[0] - fb[0])
    assert np.abs(d - 0.5).max() < 2e-4


def test_align_matrix_vs_golden(engines):
    g = Hh.gold_npz("align_golden.npz")
    for ci in range(4):
        a, w = g[f"am{ci}_a"], int(g[f"am{ci}_w"])
        got = engines["f32"].align_matrix(a[None], [a.shape[-1]], w)[0]
        assert np.allclose(got, g[f"am{ci}_mat"], rtol=1e-5, atol=2e-5), ci


def test_dtw_exact_vs_golden_and_oracle(engines):
    g = Hh.gold_npz("align_golden.npz")
    e = engines["f32"]
    for ci in range(6):
        ti, tj = e.dtw(g[f"dtw{ci}_m"])
        assert np.array_equal(ti, g[f"dtw{ci}_ti"]) and np.array_equal(tj, g[f"dtw{ci}_tj"]), ci
    ti, tj = e.dtw(np.zeros((3, 4), np.float32))
    assert ti.tolist() == [0, 1, 2, 2, 2, 2] and tj.tolist() == [0, 0, 0, 1, 2, 3]
    rng = np.random.default_rng(5)
    for N, M in ((128, 1500), (445, 1500), (1, 1), (64, 3), (445, 2)):
        m = rng.standard_normal((N, M)).astype(np.float32)
        if N == 64:
            m = np.round(m)                      # heavy ties
        ti, tj = e.dtw(m)
        oi, oj = OT.dtw(-m.astype(np.float64))
        assert np.array_equal(ti, oi) and np.array_equal(tj, oj), (N, M)
        assert ti[0] == 0 and tj[0] == 0 and ti[-1] == N - 1 and tj[-1] == M - 1          # path properties
        assert (np.diff(ti) >= 0).all() and (np.diff(tj) >= 0).all() and ((np.diff(ti) + np.diff(tj)) >= 1).all()


def test_pauses_vs_reference_golden(engines):
    from crisperwhisper_amd import utils
    for case in Hh.gold_json("pauses_golden.json"):
        inp = {"text": "x", "chunks": [{"text": c["text"], "timestamp": tuple(c["timestamp"])} for c in case["in"]]}
        out = utils.adjust_pauses_for_hf_pipeline_output(inp, split_threshold=case["thr"], engine=engines["f32"])
        assert out is inp
        assert [list(c["timestamp"]) for c in out["chunks"]] == [c["timestamp"] for c in case["out"]]


def test_dtw_property_gpu_vs_oracle(engines):
    """Random shapes / heavy ties / degenerate sizes: the wavefront DTW path equals the oracle exactly."""
    from hypothesis import given, settings, strategies as st
    e = engines["f32"]

    @settings(max_examples=40, deadline=None)
    @given(st.integers(1, 445), st.integers(1, 1500), st.integers(0, 2 ** 31 - 1), st.sampled_from([0, 1, 3]))
    def check(N, M, seed, quant):
        rng = np.random.default_rng(seed)
        m = rng.standard_normal((N, M)).astype(np.float32)
        if quant:
            m = (np.round(m * quant) / quant).astype(np.float32)
        ti, tj = e.dtw(m)
        oi, oj = OT.dtw(-m.astype(np.float64))
        assert np.array_equal(ti, oi) and np.array_equal(tj, oj), (N, M, seed, quant)

    check()


def test_align_matrix_property_gpu_vs_oracle(engines):
    """z-score + median + head-mean on ragged column counts (incl. M <= 3: the median filter's early return)."""
    rng = np.random.default_rng(17)
    e = engines["f32"]
    for (B, Ha, N, M, w) in [(2, 3, 5, 40, 7), (1, 15, 128, 1500, 7), (3, 2, 9, 3, 7), (2, 4, 7, 64, 5), (1, 1, 2, 1, 7)]:
        a = rng.random((B, Ha, N, M)).astype(np.float32)
        a /= a.sum(-1, keepdims=True)
        ncols = [M] + [max(1, M - 1 - 2 * b) for b in range(1, B)]
        got = e.align_matrix(a, ncols, w)
        for b in range(B):
            want = OT.normalise_filter_mean(a[b][:, :, :ncols[b]], w)
            assert np.allclose(got[b][:, :ncols[b]], want, rtol=2e-5, atol=5e-5, equal_nan=True), (B, Ha, N, M, w, b)  # std == 0 -> NaN on both sides, like the reference


def test_c_abi_error_behaviour(engines):
    """Negative errno-style codes + messages instead of crashes (include/crisperwhisper.h conventions)."""
    from crisperwhisper_amd.engine import EngineError
    e = engines["f32"]
    with pytest.raises(EngineError, match="unknown tensor name"):
        e.load_tensor("model.encoder.not_a_tensor", np.zeros(4, np.float32))
    with pytest.raises(EngineError, match="expected"):
        e.load_tensor("model.encoder.conv1.bias", np.zeros(7, np.float32))
    with pytest.raises(EngineError, match="bad window"):
        e.encode([0], [2900], [500])                       # seek + n_frames beyond the 3000-frame window
    with pytest.raises(EngineError):
        e.encode(list(range(9)), [0] * 9, [3000] * 9)      # more windows than max_batch
    g, v, W, spec = Hh.tiny_setup()
    fresh = Engine(spec, dtype="f32", max_batch=2)
    try:
        with pytest.raises(EngineError, match="windows encoded"):
            fresh.decode(np.array([[v.sot, v.lang_id("en"), v.transcribe]]), max_length=8)   # nothing encoded yet
        with pytest.raises(EngineError):
            fresh.mel([np.zeros(480001, np.float32)])       # longer than one 30 s window
        # an incomplete checkpoint must not run on the zero-filled device buffers
        fresh.mel([np.zeros(16000, np.float32)])
        with pytest.raises(EngineError, match="never loaded"):
            fresh.encode([0], [0], [3000])
        partial = {k: W[k] for k in W if not k.endswith("layers.1.fc2.bias")}
        with pytest.raises(EngineError, match="fc2.bias"):
            fresh.load_state_dict(partial)
        fresh.load_state_dict(W)
        fresh.encode([0], [0], [3000])
    finally:
        fresh.close()
    bad = syn.model_spec(*syn.tiny_geometry(), 3)
    bad.alignment_heads = [[99, 0]]
    with pytest.raises(EngineError, match="alignment head"):
        Engine(bad, dtype="f32", max_batch=1)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sample_kernel_vs_oracle_processors(engines, dt):
    """sample_kernel (all logits processors collapsed into one predicate + rewritten logsumexp rule + argmax) against
    oracle/logits.py (pinned to transformers' processor objects on the same rows in tests/test_oracle_vs_golden.py):
    the chosen token must be identical on every crafted and random row, one row per launch and batched."""
    from oracle import logits as OL
    from tests import sampler_cases as SC
    g, v = syn.tiny_geometry()
    eng = engines[dt]
    cs = SC.cases(v, v.size)
    want = []
    for name, ids, lg, mn in cs:
        spec = OL.ProcessorSpec(eos=v.eos, no_timestamps=v.notimestamps, suppress=v.suppress_tokens(),
                                begin_suppress=v.begin_suppress_tokens(), max_initial_timestamp_index=50, min_new_tokens=mn)
        with np.errstate(invalid="ignore"):
            o = OL.process(spec, ids[None], lg[None], SC.N_PROMPT, SC.N_PROMPT)
        want.append(int(np.argmax(o[0])))
        got = eng.test_sample(lg[None], ids[None], SC.N_PROMPT, min_new_tokens=mn)
        assert int(got[0]) == want[-1], (name, int(got[0]), want[-1])
    # batched launch: rows sharing (t, min_new_tokens) go through one call
    groups = {}
    for i, (name, ids, lg, mn) in enumerate(cs):
        groups.setdefault((len(ids), mn), []).append(i)
    for (t, mn), idx in groups.items():
        for lo in range(0, len(idx), 4):
            sel = idx[lo:lo + 4]
            got = eng.test_sample(np.stack([cs[i][2] for i in sel]), np.stack([cs[i][1] for i in sel]), SC.N_PROMPT, min_new_tokens=mn)
            assert got.tolist() == [want[i] for i in sel], [cs[i][0] for i in sel]


def test_sample_kernel_large_vocab_vs_oracle():
    """Same differential at the BASELINE vocabulary (51866 columns: padded row stride, 4-deep load loop, 1024-thread
    block reductions): random rows + exact ties at the far end of the row."""
    from oracle import logits as OL
    g, v = syn.large_v3_geometry()
    g.enc_layers = g.dec_layers = 1
    spec = syn.model_spec(g, v, n_align=1)
    spec.alignment_heads = [[0, 0]]
    eng = Engine(spec, dtype="bf16", max_batch=8)
    try:
        rng = np.random.default_rng(5)
        tb = v.timestamp_begin
        prompt = [v.sot, v.lang_id("en"), v.transcribe]
        ospec = OL.ProcessorSpec(eos=v.eos, no_timestamps=v.notimestamps, suppress=v.suppress_tokens(),
                                 begin_suppress=v.begin_suppress_tokens(), max_initial_timestamp_index=50)
        for gen in ([], [tb], [tb, 300], [tb, 300, tb + 7], [tb, 300, tb + 7, tb + 7], [tb, 300, tb + 7, tb + 7, 41000]):
            ids = np.tile(np.asarray(prompt + gen, np.int64), (8, 1))
            lg = (rng.standard_normal((8, g.vocab)) * 3).astype(np.float32)
            lg[0, g.vocab - 1] = lg[0, tb + 100] = 40.0                  # tie between two timestamps, last column
            lg[1, 50000] = lg[1, 49999] = 41.0                           # tie between two text tokens
            lg[2, tb:] -= 100.0
            lg[3, :tb] -= 100.0
            with np.errstate(invalid="ignore"):
                o = OL.process(ospec, ids, lg, 3, 3)
            got = eng.test_sample(lg, ids, 3)
            assert got.tolist() == np.argmax(o, -1).tolist(), gen
    finally:
        eng.close()
