"""Float64 / numpy references and comparators of the encoder-stage kernel tests (tests/test_gpu_encoder_stages.py) -- the conv
gather, the GEMM epilogue layouts, LayerNorm and the row-wise e4m3 quantisation -- kept apart from the GPU module so that
tests/test_encoder_stage_refs.py can show on a CPU-only machine that each comparator rejects a subtly wrong kernel output.  The
same for encoder self-attention (tests/test_gpu_encoder_attention.py, tests/test_encoder_attention_refs.py): float64 softmax
attention, the input builders, the per-row error and a numpy restatement of the 64-queries-per-wave kernel that takes faults."""
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


# ---- encoder self-attention (tests/test_gpu_encoder_attention.py, tests/test_encoder_attention_refs.py) ------------------------------
ATTN_MARGIN = 120.0         # one-hot cases: every other score lies at least this far below the selected one (576)
ATTN_RESCALE_THR = 8.0      # RESCALE_THR of csrc/attention.hip
_COL_SCALE = 2.0 ** (np.arange(64) % 7 - 3)


def attention64(q, k, v):
    """plain softmax attention in float64: q (pre-scaled), k, v [B][H][S][64] -> [B][S][H * 64]"""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    B, H, S, _ = q.shape
    s = np.einsum("bhqd,bhkd->bhqk", q, k)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bhkd->bhqd", p, v).transpose(0, 2, 1, 3).reshape(B, S, H * 64)


def attn_row_err(got, ref):
    """worst per-row error max_d |got - ref| / max_d |ref| over the rows (b, q, h) of [B][S][H * 64]: one bad query row does not
    hide behind the tensor's largest value; inf when the output holds a NaN or an infinity"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    g, r = got.reshape(-1, 64), ref.reshape(-1, 64)
    return float((np.abs(g - r).max(-1) / (np.abs(r).max(-1) + 1e-300)).max())


def attn_values(rng, shape):
    """V with a column-dependent scale, exact in bf16 and f16: ints in [-127, 127] times 2^(d % 7 - 3)"""
    assert shape[-1] == 64
    return rng.integers(-127, 128, shape) * _COL_SCALE


def attn_onehot_case(B, H, S, seed=0):
    """Keys are sign codes (+-3 per component, |k|^2 = 576) and query i of head (b, h) IS key pi[b, h, i], with pi(i) = (i * stride
    + off) % S, stride coprime to S and different per head: the selected score is 576 and, by ATTN_MARGIN (asserted on the CPU for
    every shape and seed in use), every other probability is exactly 0 in f32 -- the output row is V[pi(i)], bit for bit.
    -> q, k, v [B][H][S][64] float64, pi [B][H][S]"""
    rng = np.random.default_rng([seed, B, H, S])
    k = rng.choice([-3.0, 3.0], (B, H, S, 64))
    v = attn_values(rng, (B, H, S, 64))
    pi = np.zeros((B, H, S), np.int64)
    for b in range(B):
        for h in range(H):
            n = b * H + h
            stride = S // 3 + 7 * n + 1
            while math.gcd(stride, S) != 1:
                stride += 1
            pi[b, h] = (np.arange(S) * stride + 5 + 11 * n) % S
    q = np.take_along_axis(k, pi[..., None], axis=2)
    return q, k, v, pi


def attn_onehot_want(v, pi):
    """out[b][i][h * 64 ..] = v[b][h][pi[b][h][i]]"""
    B, H, S, _ = v.shape
    return np.take_along_axis(v, pi[..., None], axis=2).transpose(0, 2, 1, 3).reshape(B, S, H * 64)


def attn_onehot_margin(q, k, pi):
    """smallest gap between the selected score and any other score of the same query, in float64"""
    s = np.einsum("bhqd,bhkd->bhqk", np.asarray(q, np.float64), np.asarray(k, np.float64))
    sel = np.take_along_axis(s, pi[..., None], axis=3)
    assert np.all(sel == 576.0)
    if s.shape[-1] == 1:
        return float("inf")
    np.put_along_axis(s, pi[..., None], -np.inf, axis=3)
    return float((sel[..., 0] - s.max(-1)).min())


def attn_padkey_case(B, H, S, constant_v, seed=1):
    """All keys of a head are one sign code k0 and q = -k0: every score is -576, the probabilities are equal and the output is the
    column mean of V -- unless a zero-filled pad key (score 0) is admitted, which then takes all the mass.  constant_v: V is
    constant per column, so the mean is that constant exactly.  -> q, k, v, reference [B][S][H * 64]"""
    rng = np.random.default_rng([seed, B, H, S, int(constant_v)])
    k0 = rng.choice([-3.0, 3.0], (B, H, 1, 64))
    k = np.broadcast_to(k0, (B, H, S, 64)).copy()
    v = np.broadcast_to(attn_values(rng, (B, H, 1, 64)), (B, H, S, 64)).copy() if constant_v else attn_values(rng, (B, H, S, 64))
    ref = np.broadcast_to(v.mean(2)[:, None], (B, S, H, 64)).reshape(B, S, H * 64)
    return -k, k, v, ref


STAIR_KINDS = ("up5", "up8", "up8.5", "down5", "up5_jump40", "up5_rows_x2")


def attn_stair_levels(kind, S):
    """score level of every 64-key tile.  up5: below RESCALE_THR, so probabilities are taken against a stale max (up to e^5 .. e^8);
    up8: exactly the threshold (`>`: no move, then a move by 16); up8.5: moves every tile; down5: no move after the first tile;
    up5_jump40: +5 per tile and one +40 jump -- behind twelve tiles at S = 1500, behind six where there are fewer than fourteen;
    up5_rows_x2: up5 with every third query doubled, so lanes of one wave disagree about moving."""
    t = np.arange((S + 63) // 64, dtype=np.float64)
    if kind == "up5_jump40":
        return 5.0 * t + 40.0 * (t >= (12 if len(t) >= 14 else 6))
    return {"up5": 5.0, "up8": 8.0, "up8.5": 8.5, "down5": -5.0, "up5_rows_x2": 5.0}[kind] * t


def attn_stair_case(kind, B, H, S, seed=2):
    """Scores constant within a 64-key tile: q = u1 + u2 with u1 = +-1/8 on components 0..31 and u2 = +-1/8 on 32..63 (|q|^2 = 1),
    k[j] = a u1 + b u2 with (a + b) / 2 = level(j // 64).  a = b = level wherever the level is a bf16 number; 8.5 t is not one
    beyond 127.5, and there a = bf16(level), b = 2 level - a.  Every operand is exact in bf16 and f16 and every score exact in f32.
    -> q, k, v [B][H][S][64] float64"""
    rng = np.random.default_rng([seed, B, H, S, STAIR_KINDS.index(kind)])
    u = rng.choice([-0.125, 0.125], (B, H, 1, 64))
    u1, u2 = u.copy(), u.copy()
    u1[..., 32:] = 0.0
    u2[..., :32] = 0.0
    lev = attn_stair_levels(kind, S)[np.arange(S) // 64]
    a = round16("bf16", lev)
    b = 2.0 * lev - a
    k = a[:, None] * u1 + b[:, None] * u2
    q = np.broadcast_to(u, (B, H, S, 64)).copy()
    if kind == "up5_rows_x2":
        q[:, :, ::3] *= 2.0
    for dt in ("bf16", "f16"):
        assert np.array_equal(round16(dt, k), k) and np.array_equal(round16(dt, q), q), (kind, S, dt)
    assert np.array_equal(np.einsum("bhd,bhkd->bhk", q[:, :, 1], k), np.broadcast_to(lev, (B, H, S)))
    return q, k, attn_values(rng, (B, H, S, 64))


def attn_realistic_case(dt, B, H, S, seed=3):
    """Gaussian scores of standard deviation about 4 (q ~ 0.5 N(0, 1) on 63 components) plus an attention sink: component 63 of
    every query is 1, of key 0 it is 12 and of every other key 0.  V ~ N(0, 1) times the column scale.  Rounded to the engine's type.
    -> q, k, v [B][H][S][64] float64"""
    rng = np.random.default_rng([seed, B, H, S])
    q = 0.5 * rng.standard_normal((B, H, S, 64))
    k = rng.standard_normal((B, H, S, 64))
    v = rng.standard_normal((B, H, S, 64)) * _COL_SCALE
    q[..., 63] = 1.0
    k[..., 63] = 0.0
    k[:, :, 0, 63] = 12.0
    return tuple(round16(dt, t) for t in (q, k, v))


# Bounds of the comparisons that cannot be exact: per-row error (attn_row_err) against float64, 2-3 x the largest value measured on
# MI355X over the default kernels and, for the 16-bit engines, the 32-queries-per-wave kernel of the experiments build (CW_TEST_ERRLOG
# audit of tests/test_gpu_encoder_attention.py; the measured figures stand in that module's docstrings).  Key: (case, S).
ATTN_TOL = {
    ('padkey', 1): {"f32": 0, "bf16": 0, "f16": 0},   # f32 0.00e+00  bf16 0.00e+00 / 0.00e+00  f16 0.00e+00
    ('padkey', 63): {"f32": 3.7e-07, "bf16": 0.0055, "f16": 0.00077},   # f32 1.45e-07  bf16 2.18e-03  f16 3.05e-04
    ('padkey', 65): {"f32": 3.1e-07, "bf16": 0.0056, "f16": 0.00054},   # f32 1.23e-07  bf16 2.22e-03  f16 2.15e-04
    ('padkey', 200): {"f32": 5.2e-07, "bf16": 0.0052, "f16": 0.00061},   # f32 2.06e-07  bf16 2.08e-03  f16 2.42e-04
    ('padkey', 257): {"f32": 1.7e-06, "bf16": 0.005, "f16": 0.00051},   # f32 6.59e-07  bf16 1.96e-03  f16 2.01e-04
    ('padkey', 1499): {"f32": 1.8e-06, "f16": 0.00071},   # f32 6.83e-07  f16 2.82e-04
    ('padkey', 1500): {"f32": 1.9e-06, "f16": 0.00096},   # f32 7.23e-07  f16 3.81e-04
    ('up5', 1500): {"f32": 4.3e-07, "bf16": 0.0097, "f16": 0.0011},   # f32 1.70e-07  bf16 3.85e-03 / 3.85e-03  f16 4.31e-04
    ('up5', 700): {"f32": 7.2e-07, "bf16": 0.0077, "f16": 0.00091},   # f32 2.87e-07  bf16 3.05e-03  f16 3.63e-04
    ('up8', 1500): {"f32": 2e-07, "bf16": 0.009, "f16": 0.0011},   # f32 7.63e-08  bf16 3.58e-03  f16 4.22e-04
    ('up8', 700): {"f32": 5.6e-07, "bf16": 0.007, "f16": 0.00079},   # f32 2.23e-07  bf16 2.78e-03  f16 3.16e-04
    ('up8.5', 1500): {"f32": 3.2e-07, "bf16": 0.0066, "f16": 0.00061},   # f32 1.27e-07  bf16 2.63e-03  f16 2.43e-04
    ('up8.5', 700): {"f32": 2.9e-07, "bf16": 0.0034, "f16": 0.0006},   # f32 1.14e-07  bf16 1.33e-03  f16 2.36e-04
    ('down5', 1500): {"f32": 1.3e-06, "bf16": 0.0074, "f16": 0.00086},   # f32 4.82e-07  bf16 2.93e-03  f16 3.40e-04
    ('down5', 700): {"f32": 7.2e-07, "bf16": 0.0046, "f16": 0.00032},   # f32 2.88e-07  bf16 1.81e-03  f16 1.24e-04
    ('up5_jump40', 1500): {"f32": 3e-07, "bf16": 0.011, "f16": 0.0015},   # f32 1.20e-07  bf16 4.15e-03  f16 5.71e-04
    ('up5_jump40', 700): {"f32": 5.5e-07, "bf16": 0.0075, "f16": 0.0012},   # f32 2.18e-07  bf16 3.00e-03  f16 4.57e-04
    ('up5_rows_x2', 1500): {"f32": 6.5e-07, "bf16": 0.012, "f16": 0.00097},   # f32 2.58e-07  bf16 4.48e-03  f16 3.85e-04
    ('up5_rows_x2', 700): {"f32": 8.2e-07, "bf16": 0.0096, "f16": 0.00079},   # f32 3.27e-07  bf16 3.83e-03  f16 3.15e-04
    ('realistic', 1500): {"f32": 2.1e-05, "bf16": 0.024, "f16": 0.0027},   # f32 8.08e-06  bf16 9.38e-03 / 9.38e-03  f16 1.08e-03
    ('realistic', 257): {"f32": 1.1e-05, "bf16": 0.016, "f16": 0.0022},   # f32 4.18e-06  bf16 6.15e-03  f16 8.56e-04
}


def attn_tol(case, S, dt):
    if case == "padkey_const":      # f32 engine, V constant per column: S accumulations of fl(1 / S) c, one rounding each, and fl(1 / S)
        return (S + 2) * 2.0 ** -24
    assert (case, S) in ATTN_TOL, f"no bound recorded for {(case, S)}"
    return ATTN_TOL[(case, S)][dt]


def assert_attn_rows(case, S, dt, got, ref, what="", log=None):
    e = attn_row_err(got, ref)
    if log is not None:
        log(f"{case}-{S}-{dt}", e)
    assert e <= attn_tol(case, S, dt), (what, case, S, dt, f"per-row error {e:.3e}, bound {attn_tol(case, S, dt):.1e}")


def assert_within_one_ulp16(dt, got, want64, what=""):
    """16-bit output at most one unit in the last place from the (representable) float64 value"""
    assert np.isfinite(np.asarray(got)).all(), (what, "not finite")
    d = np.abs(ordinal16(dt, got) - ordinal16(dt, round16(dt, want64)))
    assert d.max() <= 1, (what, dt, f"{int((d > 1).sum())} elements more than one unit in the last place off")


ATTN_FAULTS = ("drop_last_key", "admit_pad_key", "mask_stride_8", "swap_v_halves", "swap_out_chunks", "clamp_q_s_minus_2",
               "skip_o_rescale", "max_frozen_f16_p")


def _round_p(dt, p):
    if dt == "f16":
        return p.astype(np.float16).astype(np.float64)        # overflows to inf like the conversion instruction
    return round16(dt, p)


def attn_q64_emulation(dt, q, k, v, fault=None):
    """numpy restatement of attn_encoder_q64_kernel's arithmetic, tile by tile: 64-key tiles over zero-padded K / V, the peeled tile's
    mask per lane group (local key c = kt * 16 + g * 4 + r exists iff kt * 16 + r < S - k0 - g * 4), the running max that moves
    only on a rise above RESCALE_THR, P rounded to the engine's type for the P V product, sums unrounded, one rounding of O / l.
    `fault` plants one of ATTN_FAULTS.  -> [B][S][H * 64] float64"""
    assert fault is None or fault in ATTN_FAULTS
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    B, H, S, _ = q.shape
    nt = (S + 63) // 64
    pad = np.zeros((B, H, nt * 64 - S, 64))
    kp, vp = np.concatenate([k, pad], 2), np.concatenate([v, pad], 2)
    c = np.arange(64)
    g = (c % 16) // 4
    out = np.zeros((B, S, H * 64))
    qi = np.minimum(np.arange(S), max(S - 2, 0)) if fault == "clamp_q_s_minus_2" else np.arange(S)
    pdt = "f16" if fault == "max_frozen_f16_p" else dt
    with np.errstate(all="ignore"):
        for b in range(B):
            for h in range(H):
                Q = q[b, h][qi]
                m, l, O = np.full(S, -np.inf), np.zeros(S), np.zeros((S, 64))
                for t in range(nt):
                    k0 = t * 64
                    s = (Q @ kp[b, h, k0:k0 + 64].T).astype(np.float32).astype(np.float64)
                    lim = S - k0 + {"drop_last_key": -1, "admit_pad_key": 1}.get(fault, 0)
                    stride = 8 if fault == "mask_stride_8" and S - k0 < 64 else 4
                    s = np.where(c - 4 * g + stride * g < lim, s, -np.inf)
                    mx = s.max(-1)
                    mv = np.full(S, t == 0) if fault == "max_frozen_f16_p" else mx > m + ATTN_RESCALE_THR
                    if mv.any():
                        mnew = np.where(mv, mx, m)
                        alpha = np.where(mnew == m, 1.0, np.exp(m - mnew))
                        l *= alpha
                        if fault != "skip_o_rescale":
                            O *= alpha[:, None]
                        m = mnew
                    p = np.exp(s - m[:, None]).astype(np.float32).astype(np.float64)
                    l += p.sum(-1)
                    vt = vp[b, h, k0:k0 + 64]
                    O += _round_p(pdt, p) @ (vt[c ^ 16] if fault == "swap_v_halves" else vt)
                o = round16(dt, (O * (1.0 / l)[:, None]).astype(np.float32))
                if fault == "swap_out_chunks":
                    o[:, 8:24] = np.concatenate([o[:, 16:24], o[:, 8:16]], 1)
                out[b, :, h * 64:(h + 1) * 64] = o
    return out
