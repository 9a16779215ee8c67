"""GPU parity tests of the encoder's front end, one launch at a time (cw_test_gemm_epi / cw_test_rownorm): the implicit conv1d
gather of the tile GEMMs, every GEMM epilogue layout, LayerNorm and the row-wise e4m3 quantisation, each against plain numpy
float64 (tests/encoder_refs.py).  Operands are small integers times a power of two wherever the operation allows it, so that the
result is exact in f32 and the comparison is bit for bit; the GELU epilogues and LayerNorm go through the measured-tolerance
audit (rel_err / CW_TEST_ERRLOG).  Every output starts as a sentinel, so an element the kernel did not write -- or wrote where
it should not -- shows.

Which kernel body a case reaches (read off launch_gemm_epi in csrc/gemm.hip): f32 engine -> gemm_f32_kernel; 16-bit engines ->
gemm_bf16_glds_kernel (128 tiles) by default, with gemm256_min_tiles = 1 gemm_bf16_256_kernel (conv gather, N % 256 != 0, or
gemm_8ph = 0) and gemm_bf16_8ph_kernel (plain A, N % 256 == 0); CW_NO_GLDS=1 (child process) -> gemm_bf16_kernel; the
experiments build's ping-pong / w128 schedules in its child process; fp8 -> quant_rows_fp8_kernel + gemm_fp8_pp_kernel."""
import os

import numpy as np
import pytest

from crisperwhisper_amd.engine import Engine, EngineError
from tests import encoder_refs as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

EPI_STORE, EPI_GELU, EPI_RESID_F32, EPI_GELU_POS_F32, EPI_HEADS, EPI_STORE_F32 = 0, 1, 2, 3, 4, 5
DTS = ("f32", "bf16", "f16")


@pytest.fixture(scope="module")
def engines():
    g, v, W, spec = Hh.tiny_setup()
    out = {}
    for dt in DTS:
        out[dt] = Engine(spec, dtype=dt, max_batch=4)
    yield out
    for e in out.values():
        e.close()


def rel_err(a, b):
    e = R.rel_err_plain(a, b)
    log = os.environ.get("CW_TEST_ERRLOG")                       # tolerance audit: CW_TEST_ERRLOG=<file> records every measured error
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{e:.3e}\n")
    return e


def _sent(*shape):
    return np.full(shape, R.SENTINEL, np.float32)


def _tilings(dt, N=1):
    """tile choices of a 16-bit engine: the default (128 tiles at these sizes), the 256-tile kernels forced on and, where that
    selects the 8-phase kernel (plain A, N % 256 == 0), also the lockstep 256 kernel (gemm_8ph = 0)"""
    if dt == "f32":
        return ("default",)
    return ("default", "tile256") + (("tile256_lockstep",) if N % 256 == 0 else ())


class _tiling:
    def __init__(self, eng, mode, **opts):
        self.eng, self.mode, self.opts = eng, mode, opts

    def __enter__(self):
        if self.mode.startswith("tile256"):
            assert self.eng.lib.cw_test_set_option(b"gemm256_min_tiles", 1) == 0
        if self.mode == "tile256_lockstep":
            assert self.eng.lib.cw_test_set_option(b"gemm_8ph", 0) == 0
        for k, v in self.opts.items():
            assert self.eng.lib.cw_test_set_option(k.encode(), v) == 0

    def __exit__(self, *exc):
        lib = self.eng.lib
        lib.cw_test_set_option(b"gemm256_min_tiles", 200)
        lib.cw_test_set_option(b"gemm_pp", 1)
        lib.cw_test_set_option(b"gemm_8ph", 1)
        lib.cw_test_set_option(b"gemm_w128", 0)


GELU_TOL, GELU_POS_TOL, LN_F32_TOL = R.GELU_TOL, R.GELU_POS_TOL, R.LN_F32_TOL      # measured tolerances: tests/encoder_refs.py

# ---- a / b: the conv gather --------------------------------------------------------------------------------------------------
# (C_in, T_in, T_out, stride, N, [(items, seeks, valids), ...]): three input items; between the window sets row_valid takes 0, 1,
# 2, 3, an odd value mid-window and T_in - seek with an odd seek; row_off is not monotonic; two batch rows share an item
CONV_A = (64, 150, 150, 1, 128, [((2, 0, 0), (7, 0, 101), (143, 0, 1)),
                                 ((1, 2, 1), (0, 33, 40), (2, 3, 77))])
CONV_B = (128, 150, 75, 2, 192, [((2, 0, 0, 1), (7, 0, 100, 5), (143, 1, 0, 3)),
                                 ((1, 1, 0, 2), (0, 21, 0, 148), (150, 77, 2, 2))])


def _run_conv(eng, dt, case, seed):
    C_in, T_in, T_out, stride, N, windows = case
    K = 3 * C_in
    for wi, (items, seeks, valids) in enumerate(windows):
        rng = np.random.default_rng(seed + wi)
        inp, ro, rv = R.conv_case(rng, C_in, T_in, 3, items, seeks, valids)
        M = len(ro) * T_out
        _, W, bias = R.int_operands(rng, M, N, K)
        c = R.gemm64(R.conv_operand(inp, T_out, stride, ro, rv), W, bias)
        conv = (T_out, stride, ro, rv)
        got = eng.test_gemm_epi(EPI_STORE_F32, inp, W, bias, out=_sent(M, N), conv=conv, ldo=N)
        R.assert_exact(got, c, (dt, "conv", stride, wi, "store_f32"))
        if stride == 1:      # conv1's epilogue
            got = eng.test_gemm_epi(EPI_GELU, inp, W, bias, out=_sent(M, N), conv=conv, ldo=N)
            e = rel_err(got, R.gelu64(c))
            assert e < GELU_TOL[dt], (dt, "conv1 gelu", wi, e)                      # measured: f32 1.7e-8, bf16 2.7e-3, f16 4.1e-5
        else:                # conv2's: GELU + positions, T = T_out, f32 out
            pos = rng.integers(-32, 33, (T_out, N)) / 16.0
            got = eng.test_gemm_epi(EPI_GELU_POS_F32, inp, W, bias, out=_sent(M, N), conv=conv, pos=pos, ldo=N, T=T_out)
            e = rel_err(got, R.pos_epilogue(c, pos, T_out))
            assert e < GELU_POS_TOL[dt], (dt, "conv2 gelu + pos", wi, e)            # measured: f32 1.2e-8, 16-bit 1.5e-8


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("which", ["conv1", "conv2"])
def test_conv_gather(engines, dt, which):
    """conv1's form (stride 1, M = 450: 128-row tiles straddle the three batch rows) and conv2's (stride 2, M = 300, K = 384: two
    K-tiles per tap), windows of 0 .. 3 rows, odd seeks, a shared item: a_row_ptr (f32) and the hoisted copies of the 128- and
    256-tile LDS-DMA kernels, each with interior and M / N edge tiles."""
    for mode in _tilings(dt):
        with _tiling(engines[dt], mode):
            _run_conv(engines[dt], dt, CONV_A if which == "conv1" else CONV_B, 11 if which == "conv1" else 23)


@pytest.mark.parametrize("kernel", ["register_staged"])
def test_conv_gather_fallback_kernel(request, engines, kernel):
    """gemm_bf16_kernel (CW_NO_GLDS=1, read once per process): both conv forms through a_row_ptr<bf16_t>, in a child process."""
    if not os.environ.get("CW_NO_GLDS"):
        return Hh.run_in_child(request, {"CW_NO_GLDS": "1"}, lambda p: True)
    for dt in ("bf16", "f16"):
        _run_conv(engines[dt], dt, CONV_A, 11)
        _run_conv(engines[dt], dt, CONV_B, 23)


# ---- c: EPI_HEADS --------------------------------------------------------------------------------------------------------------
def _heads_case(M, T, H, D, K, S_pad, n_which=3):
    rng = np.random.default_rng(M + T + H + D + K)
    A, W, bias = R.int_operands(rng, M, n_which * D, K)
    mag = np.abs(bias) + 1.0                                   # q rows +, k rows -, v rows + and larger: a swapped `which` shows
    bias = np.concatenate([mag[:D], -mag[D:2 * D], mag[2 * D:] + 4.0])
    return A, W, bias, R.heads_epilogue(R.gemm64(A, W, bias), T, H, S_pad, D)


def _run_heads(eng, A, W, bias, T, H, D, S_pad, fp8=False):
    B, nw = A.shape[0] // T, W.shape[0] // D
    outs = [_sent(B, H, S_pad, 64) for _ in range(nw)]
    eng.test_gemm_epi(EPI_HEADS, A, W, bias, out=outs[0], out1=outs[1], out2=outs[2] if nw == 3 else None, T=T, S_pad=S_pad, H=H,
                      d_model=D, fp8=fp8)
    return outs


HEADS_SHAPES = [(300, 150, 2, 128, 128, 192), (300, 50, 2, 128, 64, 64), (77, 77, 1, 64, 64, 80), (300, 150, 4, 256, 128, 160)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,T,H,D,K,S_pad", HEADS_SHAPES)
def test_heads_epilogue(engines, dt, M, T, H, D, K, S_pad):
    """q / k / v head split, exact: item boundaries inside a tile (T = 150 and 50 against 64- / 128- / 256-row tiles), a single
    M- and N-edge tile (77 x 192), rows s >= T of every (b, h) untouched; N = 768 with the 256 tiles forced on: the 8-phase
    kernel, and the lockstep 256 kernel under gemm_8ph = 0 gives the same bits."""
    eng = engines[dt]
    A, W, bias, want = _heads_case(M, T, H, D, K, S_pad)
    seen = {}
    for mode in _tilings(dt, 3 * D):
        with _tiling(eng, mode):
            seen[mode] = got = _run_heads(eng, A, W, bias, T, H, D, S_pad)
        for w in range(3):
            R.assert_exact16(dt, got[w], want[w], (dt, mode, "which", w))
    if "tile256_lockstep" in seen:
        for w in range(3):
            assert np.array_equal(seen["tile256_lockstep"][w], seen["tile256"][w]), (dt, "8-phase on / off", w)


@pytest.mark.parametrize("sched", ["pingpong", "w128"])
def test_heads_epilogue_experiment_schedules(request, engines, sched):
    """The ping-pong and w128 schedules (experiments build, child process) on the N = 768 head split: exact, and the lockstep
    kernel's bits."""
    if not Hh.has_experiments():
        return Hh.run_in_child(request, Hh.experiments_env(), lambda p: True)
    M, T, H, D, K, S_pad = HEADS_SHAPES[3]
    A, W, bias, want = _heads_case(M, T, H, D, K, S_pad)
    for dt in ("bf16", "f16"):
        eng = engines[dt]
        with _tiling(eng, "tile256", gemm_pp=0, gemm_w128=0):
            lock = _run_heads(eng, A, W, bias, T, H, D, S_pad)
        with _tiling(eng, "tile256", gemm_pp=1, gemm_8ph=0, gemm_w128=1 if sched == "w128" else 0):
            got = _run_heads(eng, A, W, bias, T, H, D, S_pad)
        for w in range(3):
            R.assert_exact16(dt, got[w], want[w], (dt, sched, "which", w))
            assert np.array_equal(got[w], lock[w]), (dt, sched, w)


# ---- d: the f32 epilogues, plain A ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,ldo", [(300, 200, 128, 200), (77, 51, 64, 51), (300, 256, 128, 320)])
def test_f32_epilogues(engines, dt, M, N, K, ldo):
    """EPI_STORE_F32 and EPI_RESID_F32 (in place, as the engine calls it) exact; EPI_GELU_POS_F32 with T = 75 (m % T wraps inside a
    tile) to tolerance; an N-edge tile, ldo % 4 != 0 (scalar stores) and ldo > N (columns N .. ldo keep the sentinel)."""
    eng = engines[dt]
    rng = np.random.default_rng(M + N + K + ldo)
    A, W, bias = R.int_operands(rng, M, N, K)
    c = R.gemm64(A, W, bias)
    T = 75
    resid = rng.integers(-64, 65, (M, N)) / 16.0
    pos = rng.integers(-32, 33, (T, ldo)) / 16.0
    pad = np.full((M, ldo), R.SENTINEL)

    def padded(x):
        o = pad.copy(); o[:, :N] = x
        return o
    for mode in _tilings(dt, N):
        with _tiling(eng, mode):
            got = eng.test_gemm_epi(EPI_STORE_F32, A, W, bias, out=_sent(M, ldo), ldo=ldo)
            R.assert_exact(got, padded(c), (dt, mode, "store_f32"))
            io = padded(resid).astype(np.float32)
            got = eng.test_gemm_epi(EPI_RESID_F32, A, W, bias, out=io, ldo=ldo)
            R.assert_exact(got, padded(resid + c), (dt, mode, "resid_f32"))
            got = eng.test_gemm_epi(EPI_GELU_POS_F32, A, W, bias, out=_sent(M, ldo), pos=pos, ldo=ldo, T=T)
            R.assert_exact(got[:, N:], pad[:, N:], (dt, mode, "gelu_pos: columns beyond N"))
            e = rel_err(got[:, :N], R.pos_epilogue(c, pos, T))
            assert e < GELU_POS_TOL[dt], (dt, mode, "gelu_pos", e)                  # measured: 2.6e-8 at most (77 x 51), all engines


# ---- e: the e4m3 GEMM's other epilogues -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fp8_gemm_heads_and_residual_epilogues(engines, dt):
    """gemm_fp8_pp_kernel<EPI_HEADS> in the two-output form of the cross-K/V projection (the kernel takes N % 256 == 0: with d_model
    = 128 that is N = 2 d_model) and <EPI_RESID_F32>, exact on operands the quantisation represents (ints in [-14, 14], +-14 in
    every row: scale 2^-5); M = 300: one interior and one M-edge tile."""
    eng = engines[dt]
    M, T, H, D, K, S_pad = 300, 150, 2, 128, 128, 192
    rng = np.random.default_rng(5)
    A, W = R.fp8_operands(rng, M, 2 * D, K)
    mag = rng.integers(1, 33, 2 * D) / 16.0
    bias = np.concatenate([mag[:D], -mag[D:]])
    want = R.heads_epilogue(R.gemm64(A, W, bias), T, H, S_pad, D)
    got = _run_heads(eng, A, W, bias, T, H, D, S_pad, fp8=True)
    for w in range(2):
        R.assert_exact16(dt, got[w], want[w], (dt, "fp8 heads", w))
    M, N, K = 300, 256, 256
    A, W = R.fp8_operands(rng, M, N, K)
    bias = rng.integers(-32, 33, N) / 16.0
    resid = rng.integers(-64, 65, (M, N)) / 16.0
    got = eng.test_gemm_epi(EPI_RESID_F32, A, W, bias, out=resid.astype(np.float32), ldo=N, fp8=True)
    R.assert_exact(got, resid + R.gemm64(A, W, bias), (dt, "fp8 resid"))


# ---- f: LayerNorm -----------------------------------------------------------------------------------------------------------------
LN_D = (4, 128, 384, 1280, 2048, 2052)       # 2052: the d > 2048 loop branch of layernorm_kernel, which no model geometry takes
LN_ROWS = (1, 5, 8)                          # 5: the fourth wave of the second block has no row
LN_KINDS = ("normal", "offset", "constant")


def ln_seed(kind, d):
    return 100000 + 1000 * LN_KINDS.index(kind) + d      # chosen on the CPU: tests/test_encoder_stage_refs.py


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("d", LN_D)
def test_layernorm(engines, dt, d):
    """layernorm_kernel<float | 16-bit> against float64.  f32 output: measured tolerance.  16-bit output: the float64 result
    rounded once to the engine's type; no element further than one unit in the last place, at most 1 % at one unit (a rounding
    boundary crossed by the f32 arithmetic: tests/test_encoder_stage_refs.py counts at most 0.07 % for the f32 restatement of the
    formula on these inputs).  Rows beyond `rows` of the output buffer keep the sentinel."""
    eng = engines[dt]
    for kind in LN_KINDS:
        x8, g, b = R.ln_inputs(kind, 8, d, ln_seed(kind, d))
        for rows in LN_ROWS:
            x = x8[:rows]
            ref = R.layer_norm64(x, g, b)
            got = eng.test_rownorm(0, x, g, b, out=_sent(rows, d))
            if dt == "f32":
                e = rel_err(got, ref)
                assert e < LN_F32_TOL, (kind, rows, d, e)                          # measured: 1.0e-7 .. 1.44e-7 over d (largest at 2052)
            else:
                R.assert_ln16(dt, got, ref, (kind, rows, d))
            if kind == "constant" and dt != "f32":
                R.assert_exact16(dt, got, np.broadcast_to(b.astype(np.float64), (rows, d)), ("constant row -> beta", dt, d))


# ---- g: the e4m3 row kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rows,d", [(5, 128), (8, 1280), (3, 2048)])
def test_layernorm_fp8(engines, dt, rows, d):
    """layernorm_fp8_kernel: scale = max|y| / 448 and bytes within half an e4m3 step of the float64 LayerNorm, both loosened only
    by the f32 LayerNorm error measured in test_layernorm; a constant row with beta = 0 gives scale 1 and zero bytes."""
    eng = engines[dt]
    for kind in ("normal", "offset"):
        x, g, b = R.ln_inputs(kind, rows, d, ln_seed(kind, d))
        ref = R.layer_norm64(x, g, b)
        tol = LN_F32_TOL * np.abs(ref).max()
        codes, scale = eng.test_rownorm(1, x, g, b, out8=np.full((rows, d), 0x7F, np.uint8), scale=_sent(rows))
        R.assert_fp8_rows(codes, scale, ref, tol, tol, (dt, kind, rows, d))
    x, g, _ = R.ln_inputs("constant", rows, d, 7)
    codes, scale = eng.test_rownorm(1, x, g, np.zeros(d, np.float32), out8=np.full((rows, d), 0x7F, np.uint8), scale=_sent(rows))
    assert np.all(scale == 1.0) and np.all((codes & 0x7F) == 0), (dt, rows, d, scale.tolist())


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rows,K", [(5, 8), (8, 128), (3, 1280)])
def test_quant_rows_fp8(engines, dt, rows, K):
    """quant_rows_fp8_kernel on 16-bit rows: scales and bytes exactly those of the documented quantisation; a zero row gives
    scale 1 and zero bytes; rows of very different magnitude."""
    rng = np.random.default_rng(rows * 31 + K)
    x = (rng.standard_normal((rows, K)) * np.logspace(-2, 2, rows)[:, None]).astype(np.float32)
    x[rows // 2] = 0.0
    codes, scale = engines[dt].test_rownorm(2, x, out8=np.full((rows, K), 0x7F, np.uint8), scale=_sent(rows))
    want, want_s = R.quant_rows_ref(dt, x)
    assert np.array_equal(scale, want_s), (dt, scale.tolist(), want_s.tolist())
    R.assert_exact(R.e4m3_table()[codes], want, (dt, rows, K, "bytes"))
    assert scale[rows // 2] == 1.0 and np.all((codes[rows // 2] & 0x7F) == 0)


# ---- h: refusals ---------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_bad_arguments_before_launch(engines):
    """Argument checks only: every combination the header lists returns CW_ERR_INVALID and the context stays usable."""
    e = engines["bf16"]
    rng = np.random.default_rng(3)
    A, W, bias = R.int_operands(rng, 128, 128, 64)
    inp, ro, rv = R.conv_case(rng, 64, 50, 2, (0, 1), (0, 3), (50, 47))
    Wc = W[:, :1].repeat(192, axis=1)
    S = lambda *s: _sent(*s)
    hd = dict(T=64, S_pad=64, H=1, d_model=64)
    W3 = np.tile(W[:64], (3, 1))
    bad = [
        lambda: e.test_gemm_epi(EPI_STORE, A[:, :32], W[:, :32], out=S(128, 128), ldo=128),                       # K % 64
        lambda: e.test_gemm_epi(EPI_STORE, A, W, out=S(128, 128), ldo=64),                                         # ldo < N
        lambda: e.test_gemm_epi(9, A, W, out=S(128, 128), ldo=128),                                                # no such epilogue
        lambda: e.test_gemm_epi(EPI_STORE_F32, inp[:, :32], Wc[:, :128], out=S(100, 128), conv=(50, 1, ro, rv), ldo=128, K=128),  # C_in % 64
        lambda: e.test_gemm_epi(EPI_STORE_F32, inp, Wc, out=S(100, 128), conv=(50, 1, ro, [50, 48]), ldo=128),     # window past the input
        lambda: e.test_gemm_epi(EPI_STORE_F32, inp, Wc, out=S(100, 128), conv=(50, 1, [-1, 50], rv), ldo=128),     # window before the input
        lambda: e.test_gemm_epi(EPI_STORE_F32, inp, Wc, out=S(100, 128), conv=(50, 3, ro, rv), ldo=128),           # stride
        lambda: e.test_gemm_epi(EPI_HEADS, A[:100], W3, out=S(2, 1, 64, 64), out1=S(2, 1, 64, 64), out2=S(2, 1, 64, 64), **hd),         # M % T
        lambda: e.test_gemm_epi(EPI_HEADS, A, W3, out=S(2, 1, 64, 64), out1=S(2, 1, 64, 64), out2=S(2, 1, 64, 64), **dict(hd, d_model=96)),   # d_model % 64
        lambda: e.test_gemm_epi(EPI_HEADS, A, W, out=S(2, 1, 64, 64), out1=S(2, 1, 64, 64), out2=S(2, 1, 64, 64), **dict(hd, d_model=128, H=2)),  # N != 2 / 3 d_model
        lambda: e.test_gemm_epi(EPI_HEADS, A, W3, out=S(2, 1, 64, 64), out1=S(2, 1, 64, 64), out2=S(2, 1, 64, 64), **dict(hd, S_pad=63)),     # S_pad < T
        lambda: e.test_gemm_epi(EPI_HEADS, A, W3, out=S(2, 1, 64, 64), out1=S(2, 1, 64, 64), **hd),               # third output missing
        lambda: e.test_gemm_epi(EPI_GELU_POS_F32, A, W, out=S(128, 128), ldo=128, T=64),                           # pos missing
        lambda: e.test_gemm_epi(EPI_STORE, A, W, out=S(128, 128), ldo=128, fp8=True),                              # fp8: N % 256, K % 128
        lambda: e.test_gemm_epi(EPI_STORE_F32, np.tile(A, (1, 2)), np.tile(W, (2, 2)), out=S(128, 256), ldo=256, fp8=True),   # fp8: epilogue
        lambda: engines["f32"].test_gemm_epi(EPI_STORE, np.tile(A, (1, 2)), np.tile(W, (2, 2)), out=S(128, 256), ldo=256, fp8=True),   # fp8 on the f32 engine
        lambda: e.test_rownorm(0, np.zeros((2, 6), np.float32), np.ones(6, np.float32), np.zeros(6, np.float32)),  # d % 4
        lambda: e.test_rownorm(1, np.zeros((2, 2052), np.float32), np.ones(2052, np.float32), np.zeros(2052, np.float32)),   # fp8 LayerNorm: d > 2048
        lambda: e.test_rownorm(2, np.zeros((2, 12), np.float32)),                                                  # quantiser: K % 8
        lambda: e.test_rownorm(3, np.zeros((2, 8), np.float32)),                                                   # no such mode
        lambda: engines["f32"].test_rownorm(1, np.zeros((2, 8), np.float32), np.ones(8, np.float32), np.zeros(8, np.float32)),
        lambda: engines["f32"].test_rownorm(2, np.zeros((2, 8), np.float32)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(EngineError, match=r"\(-22\)"):
            call()
            pytest.fail(f"refusal case {i} was accepted")
        got = e.test_gemm_epi(EPI_STORE_F32, A, W, bias, out=S(128, 128), ldo=128)          # the context still works
        R.assert_exact(got, R.gemm64(A, W, bias), ("after refusal", i))
