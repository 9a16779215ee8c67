"""Float64 / numpy references and comparators of the encoder-stage kernel tests (tests/test_gpu_encoder_stages.py) -- the conv
gather, the GEMM epilogue layouts, LayerNorm and the row-wise e4m3 quantisation -- kept apart from the GPU module so that
tests/test_encoder_stage_refs.py can show on a CPU-only machine that each comparator rejects a subtly wrong kernel output."""
import math

import numpy as np

from tests import helpers as Hh

SENTINEL = 49152.0          # 1.5 * 2^15: exact in bf16 / f16 / f32 and beyond anything the test operands can produce
LN_ULP_CAP = 0.01           # share of 16-bit LayerNorm outputs that may sit one unit in the last place from the rounded float64 value
# Tolerances of the comparisons that cannot be exact, 2-3 x the largest error measured on MI355X (CW_TEST_ERRLOG audit of
# tests/test_gpu_encoder_stages.py; the figures are written next to the checks there).  GELU: 16-bit figures are the rounding of the
# stored output.  GELU + positions stores f32 in every engine; the 16-bit engines evaluate erf by the rational form of gelu_fast.
GELU_TOL = {"f32": 4e-8, "bf16": 7e-3, "f16": 1e-4}            # measured 1.7e-8 / 2.7e-3 / 4.1e-5
GELU_POS_TOL = {"f32": 6.5e-8, "bf16": 6.5e-8, "f16": 6.5e-8}  # measured 2.6e-8 in every engine (the f32 rounding of the stored sum)
LN_F32_TOL = 3.5e-7         # layernorm_kernel<float> against float64, relative to the largest element: measured 1.44e-7 (d = 2052)
_erf = np.vectorize(math.erf, otypes=[np.float64])


# ---- number formats -------------------------------------------------------------------------------------------------------
def round16(dt, x):
    """float64 -> the engine's storage type with ONE round-to-nearest-even (f32: to float32), returned as float64"""
    x = np.asarray(x, np.float64)
    if dt == "f32":
        return x.astype(np.float32).astype(np.float64)
    sig, emin = (8, -125) if dt == "bf16" else (11, -13)      # significand bits, frexp exponent of the smallest normal
    _, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e, emin) - sig)
    return np.round(x / q) * q                                 # np.round: half to even


def ordinal16(dt, x):
    """position of every (16-bit representable) value on the engine type's number line: neighbours differ by 1"""
    x = np.asarray(x, np.float32)
    bits = (x.view(np.uint32) >> 16).astype(np.int64) if dt == "bf16" else x.astype(np.float16).view(np.uint16).astype(np.int64)
    return np.where(bits & 0x8000, -(bits & 0x7FFF), bits & 0x7FFF)


def e4m3_table():
    """the 256 OCP e4m3 codes as float64 (0x7f / 0xff: NaN)"""
    b = np.arange(256)
    ex, man = (b >> 3) & 15, b & 7
    v = np.where(ex == 0, man * 2.0 ** -9, (1 + man / 8.0) * 2.0 ** (ex.astype(np.float64) - 7))
    v = np.where((b & 0x7F) == 0x7F, np.nan, v)
    return np.where(b & 0x80, -v, v)


def e4m3_encode(v):
    """codes of values that lie on the e4m3 grid (float64 in, uint8 out)"""
    v = np.asarray(v, np.float64)
    pos = e4m3_table()[:127]
    i = np.searchsorted(pos, np.abs(v))
    assert np.all(pos[np.minimum(i, 126)] == np.abs(v))
    return (i | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


# ---- operands ---------------------------------------------------------------------------------------------------------------
def int_operands(rng, M, N, K, ldo=None):
    """A ints in [-4, 4], W ints / 16, bias / resid / pos ints / 16: every product, partial sum and epilogue sum of a K <= 384
    GEMM is exact in f32 and the operands are exact in bf16 / f16, so the result does not depend on the summation order."""
    ldo = N if ldo is None else ldo
    A = rng.integers(-4, 5, (M, K)).astype(np.float64)
    W = rng.integers(-4, 5, (N, K)) / 16.0
    bias = rng.integers(-32, 33, N) / 16.0
    return A, W, bias


def fp8_operands(rng, M, N, K):
    """ints in [-14, 14] with a +-14 in every row: the row scale is 2^-5 and the e4m3 quantisation is exact"""
    A = rng.integers(-14, 15, (M, K)).astype(np.float64); A[:, 0] = 14
    W = rng.integers(-14, 15, (N, K)).astype(np.float64); W[:, 1] = -14
    return A, W


def conv_case(rng, C_in, T_in, n_items, items, seeks, valids, fill=3.0):
    """Time-major input [n_items * T_in][C_in]: ints in [-4, 4] inside the windows, the non-zero constant `fill` everywhere else
    (a row read from beyond a window changes the result); row_off[b] = items[b] * T_in + seeks[b], row_valid[b] = valids[b]."""
    inp = np.full((n_items * T_in, C_in), fill, np.float64)
    row_off = np.asarray([it * T_in + s for it, s in zip(items, seeks)], np.int32)
    row_valid = np.asarray(valids, np.int32)
    for o, n in zip(row_off, row_valid):
        assert o + n <= (o // T_in + 1) * T_in                # a window stays inside its item
        inp[o:o + n] = rng.integers(-4, 5, (n, C_in))
    return inp, row_off, row_valid


# ---- float64 references -------------------------------------------------------------------------------------------------------
def gelu64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + _erf(x * 0.7071067811865476))


def conv_operand(inp, T_out, stride, row_off, row_valid):
    """The A operand of the implicit conv1d(k = 3, pad = 1): x[b * T_out + t] = concat over tap of
    inp[row_off[b] + t * stride + tap - 1], zeros unless 0 <= t * stride + tap - 1 < row_valid[b]."""
    inp = np.asarray(inp, np.float64)
    nb, C = len(row_off), inp.shape[1]
    x = np.zeros((nb, T_out, 3, C))
    t = np.arange(T_out)
    for b in range(nb):
        for tap in range(3):
            t_in = t * stride + tap - 1
            ok = (t_in >= 0) & (t_in < row_valid[b])
            x[b, ok, tap] = inp[row_off[b] + t_in[ok]]
    return x.reshape(nb * T_out, 3 * C)


def gemm64(A, W, bias=None):
    c = np.asarray(A, np.float64) @ np.asarray(W, np.float64).T
    return c if bias is None else c + np.asarray(bias, np.float64)


def pos_epilogue(c, pos, T):
    """EPI_GELU_POS_F32: gelu(c[m]) + pos[m % T]"""
    return gelu64(c) + np.asarray(pos, np.float64)[np.arange(c.shape[0]) % T, :c.shape[1]]


def heads_epilogue(c, T, H, S_pad, d_model, fill=SENTINEL):
    """EPI_HEADS: column n = which * d_model + h * 64 + dd of row m = b * T + s goes to outs[which][b][h][s][dd]; rows s >= T of every
    (b, h) keep `fill`"""
    M, N = c.shape
    nw, B = N // d_model, M // T
    outs = []
    for w in range(nw):
        o = np.full((B, H, S_pad, 64), fill, np.float64)
        o[:, :, :T] = c[:, w * d_model:(w + 1) * d_model].reshape(B, T, H, 64).transpose(0, 2, 1, 3)
        outs.append(o)
    return outs


def layer_norm64(x, g, b, eps=1e-5):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def layer_norm_f32(x, g, b):
    """float32 restatement of layernorm_kernel's formula (two passes, rstd = 1 / sqrt(var + eps), (x - mean) * rstd * g + b)"""
    f = np.float32
    x, g, b = (np.asarray(t, f) for t in (x, g, b))
    d = f(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=f) / d
    c = x - mean
    rstd = f(1.0) / np.sqrt((c * c).sum(-1, keepdims=True, dtype=f) / d + f(1e-5))
    return c * rstd * g + b


def ln_inputs(kind, rows, d, seed):
    """x [rows][d] f32, gamma, beta.  "normal": N(0, 1) rows.  "offset": unit spread about a common offset of 50 -- on a 2^-6
    grid with every row summing to 50 d exactly, so the mean is 50 in any summation order and in any precision and what the
    comparison sees is the variance pass (a one-pass E[x^2] - mean^2 loses 2500 : 1 there).  "constant": constant rows, gamma
    = 1 + noise, beta != 0 -- the result is beta."""
    rng = np.random.default_rng(seed)
    g = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.5 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    if kind == "normal":
        x = rng.standard_normal((rows, d))
    elif kind == "offset":
        z = np.round(rng.standard_normal((rows, d)) * 64)
        z[:, 0] -= z.sum(-1)                                   # sum to zero; d >= 4: element 0 stays a few units wide
        x = 50.0 + z / 64.0
    else:
        x = np.repeat(np.asarray([3.25, -7.5, 0.0, 50.0, 1.0, -0.125, 100.0, 2.0])[:rows, None], d, axis=1)
    return x.astype(np.float32), g, b


# ---- comparators (raise AssertionError) -----------------------------------------------------------------------------------
def assert_exact(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, f"{len(bad)} of {got.size} elements differ; first at {bad[:4].tolist()}: "
                                 f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def assert_exact16(dt, got, want64, what=""):
    """equal to the float64 reference after one rounding to the engine's type (the sentinel is representable: untouched stays)"""
    assert_exact(got, round16(dt, want64), what)


def rel_err_plain(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-12))


def ln16_ulp_counts(dt, got, ref64):
    """(elements one unit in the last place from round16(ref), elements further away)"""
    d = np.abs(ordinal16(dt, got) - ordinal16(dt, round16(dt, ref64)))
    return int((d == 1).sum()), int((d > 1).sum())


def assert_ln16(dt, got, ref64, what=""):
    one, more = ln16_ulp_counts(dt, got, ref64)
    assert more == 0, (what, dt, f"{more} elements more than one unit in the last place from the rounded float64 LayerNorm")
    assert one <= LN_ULP_CAP * np.asarray(got).size, (what, dt, f"{one} of {np.asarray(got).size} elements off by one unit (cap {LN_ULP_CAP:.0%})")


def assert_fp8_rows(codes, scale, y_ref, y_tol, scale_tol, what=""):
    """Row-wise e4m3 quantisation of y_ref [rows][d] (float64): scale = max|y| / 448 to within scale_tol (absolute, on scale *
    448), 1 for an all-zero row; every decoded byte times the scale within half an e4m3 step of y_ref's binade plus y_tol."""
    y_ref = np.asarray(y_ref, np.float64)
    scale = np.asarray(scale, np.float64)
    amax = np.abs(y_ref).max(-1)
    want_s = np.where(amax > 0, amax / 448.0, 1.0)
    assert np.all(np.abs(scale - want_s) * 448.0 <= scale_tol + 1e-7 * amax), (what, "scale", scale.tolist(), want_s.tolist())
    val = e4m3_table()[np.asarray(codes, np.uint8)]
    assert not np.isnan(val).any(), (what, "NaN code")
    s = scale[:, None]
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(y_ref / s)))
    half = 2.0 ** (np.maximum(e, -6.0) - 4) * s
    err = np.abs(val * s - y_ref)
    bad = np.argwhere(err > half + y_tol)
    assert len(bad) == 0, (what, f"{len(bad)} bytes off; first {bad[:4].tolist()}: err {err[tuple(bad[0])]:.3e} > {half[tuple(bad[0])]:.3e} + {y_tol:.1e}")


def quant_rows_ref(dt, x):
    """quant_rows_fp8_kernel on x rounded to the engine's type: s = f32(max|x|) / 448 in f32 (1 for a zero row), inv = 1 / s in
    f32, value = e4m3(f32(x * inv)) -> (decoded values [rows][K] float64, scale [rows] float32)"""
    x16 = round16(dt, x).astype(np.float32)
    amax = np.abs(x16).max(-1)
    s = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    inv = (np.float32(1.0) / s).astype(np.float32)
    return Hh.e4m3_round((x16 * inv[:, None]).astype(np.float32)), s
