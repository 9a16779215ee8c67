"""Host-side proof that the comparisons of tests/test_gpu_encoder_stages.py bite (no GPU): deliberately wrong "kernel outputs",
made in numpy from the GPU tests' own inputs, must fail the comparators of tests/encoder_refs.py on every shape the GPU tests
use, and the float32 restatement of the right formula must pass them.  Also establishes the 1 % cap of the 16-bit LayerNorm
check: the share of elements that the f32 arithmetic moves across a 16-bit rounding boundary."""
import numpy as np
import pytest

from tests import encoder_refs as R
from tests import test_gpu_encoder_stages as G


def _fails(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


# ---- conv gather ------------------------------------------------------------------------------------------------------------------
def _conv_mutant(inp, T_out, stride, row_off, row_valid, fault, tile=128):
    """conv_operand with one fault.  The input gets a guard row of the fill constant behind it (a window grown past the last item)."""
    inp = np.vstack([inp, np.full((1, inp.shape[1]), 3.0)])
    nb, C = len(row_off), inp.shape[1]
    x = np.zeros((nb * T_out, 3, C))
    for m in range(nb * T_out):
        b, t = divmod(m, T_out)
        if fault == "item_of_tile_row0":
            b = (m - m % tile) // T_out
        valid = row_valid[b] + {"valid+1": 1, "valid-1": -1}.get(fault, 0)
        for tap in range(3):
            t_in = t * stride + tap - (0 if fault == "no_minus_1" else 1)
            if 0 <= t_in < valid:
                x[m, 2 - tap if fault == "taps_reversed" else tap] = inp[min(row_off[b] + t_in, len(inp) - 1)]
    return x.reshape(nb * T_out, 3 * C)


CONV_SHAPES = [(name, wi) for name in ("conv1", "conv2") for wi in (0, 1)]


def _conv_inputs(name, wi):
    C_in, T_in, T_out, stride, N, windows = G.CONV_A if name == "conv1" else G.CONV_B
    rng = np.random.default_rng((11 if name == "conv1" else 23) + wi)
    inp, ro, rv = R.conv_case(rng, C_in, T_in, 3, *windows[wi])
    _, W, bias = R.int_operands(rng, len(ro) * T_out, N, 3 * C_in)
    return inp, T_out, stride, ro, rv, W, bias


@pytest.mark.parametrize("name,wi", CONV_SHAPES)
def test_conv_reference_passes_in_float32(name, wi):
    inp, T_out, stride, ro, rv, W, bias = _conv_inputs(name, wi)
    c = R.gemm64(R.conv_operand(inp, T_out, stride, ro, rv), W, bias)
    x32 = R.conv_operand(inp, T_out, stride, ro, rv).astype(np.float32)
    got = x32 @ W.astype(np.float32).T + bias.astype(np.float32)            # exact operands: any f32 summation order gives this
    R.assert_exact(got, c)
    assert np.abs(c).max() < R.SENTINEL / 8


@pytest.mark.parametrize("fault", ["valid+1", "valid-1", "taps_reversed", "no_minus_1", "item_of_tile_row0"])
@pytest.mark.parametrize("name,wi", CONV_SHAPES)
def test_conv_mutations_are_rejected(name, wi, fault):
    inp, T_out, stride, ro, rv, W, bias = _conv_inputs(name, wi)
    c = R.gemm64(R.conv_operand(inp, T_out, stride, ro, rv), W, bias)
    wrong = R.gemm64(_conv_mutant(inp, T_out, stride, ro, rv, fault), W, bias)
    _fails(R.assert_exact, wrong.astype(np.float32), c)                     # the EPI_STORE_F32 comparison
    for dt in G.DTS:                                                        # and the GELU / GELU + positions ones
        if stride == 1:
            assert R.rel_err_plain(R.round16(dt, R.gelu64(wrong)), R.gelu64(c)) > R.GELU_TOL[dt]
        else:
            assert R.rel_err_plain(R.gelu64(wrong).astype(np.float32), R.gelu64(c)) > R.GELU_POS_TOL[dt]


# ---- epilogue layouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,ldo", [(300, 200, 128, 200), (77, 51, 64, 51), (300, 256, 128, 320)])
def test_position_row_m_instead_of_m_mod_T_is_rejected(M, N, K, ldo):
    rng = np.random.default_rng(M + N + K + ldo)
    A, W, bias = R.int_operands(rng, M, N, K)
    c = R.gemm64(A, W, bias)
    T = 75
    pos_all = rng.integers(-32, 33, (M, ldo)) / 16.0                        # what lies behind pos[T] is other data
    ref = R.pos_epilogue(c, pos_all[:T], T)
    wrong = R.gelu64(c) + pos_all[:, :N]
    f32 = lambda t: t.astype(np.float32)
    for dt in G.DTS:
        assert R.rel_err_plain(f32(ref), ref) < R.GELU_POS_TOL[dt]
        assert R.rel_err_plain(f32(wrong), ref) > R.GELU_POS_TOL[dt]


def _heads_flat_T(c, T, H, S_pad, D):
    """head slot computed with T instead of S_pad: outs[which][((b H + h) T + s) 64 + dd]"""
    M, N = c.shape
    outs = []
    for w in range(N // D):
        o = np.full((M // T) * H * S_pad * 64, R.SENTINEL)
        for h in range(H):
            m = np.arange(M)
            idx = ((((m // T) * H + h) * T + m % T) * 64)[:, None] + np.arange(64)
            o[idx] = c[:, w * D + h * 64:w * D + (h + 1) * 64]
        outs.append(o.reshape(M // T, H, S_pad, 64))
    return outs


@pytest.mark.parametrize("M,T,H,D,K,S_pad", G.HEADS_SHAPES)
def test_head_split_mutations_are_rejected(M, T, H, D, K, S_pad):
    A, W, bias, want = G._heads_case(M, T, H, D, K, S_pad)
    c = R.gemm64(A, W, bias)
    for dt in G.DTS:
        got = [R.round16(dt, o).astype(np.float32) for o in want]           # the right kernel: one rounding of the exact value
        for w in range(3):
            R.assert_exact16(dt, got[w], want[w])
        swapped = [got[0], got[2], got[1]]                                   # `which` 1 and 2 swapped
        _fails(R.assert_exact16, dt, swapped[1], want[1])
        _fails(R.assert_exact16, dt, swapped[2], want[2])
        flat = [R.round16(dt, o).astype(np.float32) for o in _heads_flat_T(c, T, H, S_pad, D)]
        if (M // T) * H == 1:                                                # one (item, head): T and S_pad address the same slots
            R.assert_exact16(dt, flat[0], want[0])
        else:
            for w in range(3):
                _fails(R.assert_exact16, dt, flat[w], want[w])


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
def _ln_no_mean_in_variance(x, g, b):
    f = np.float32
    x = x.astype(f)
    d = f(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=f) / d
    rstd = f(1.0) / np.sqrt((x * x).sum(-1, keepdims=True, dtype=f) / d + f(1e-5))
    return (x - mean) * rstd * g + b


# Elements of the float32 restatement that land on the other side of a 16-bit rounding boundary than float64 (rows = 8; d = 4, 128,
# 384, 1280, 2048, 2052):   normal rows  bf16 0 0 0 0 2 1, f16 0 0 1 3 3 5;   offset rows  bf16 0 0 0 0 3 1, f16 0 0 1 7 7 6;
# constant rows 0 throughout -- 0.07 % at most (7 of 10240).  The cap of the GPU check is 1 %; a case above a quarter of it here
# means another seed (G.ln_seed: the first choice had 7 of 1920 on the offset rows of d = 384, rows = 5, in f16).
@pytest.mark.parametrize("d", G.LN_D)
def test_layernorm_restatement_passes_and_stays_under_a_quarter_of_the_cap(d):
    for kind in G.LN_KINDS:
        x, g, b = R.ln_inputs(kind, 8, d, G.ln_seed(kind, d))
        ref = R.layer_norm64(x, g, b)
        y = R.layer_norm_f32(x, g, b)
        assert R.rel_err_plain(y, ref) < R.LN_F32_TOL
        for rows in G.LN_ROWS:
            for dt in ("bf16", "f16"):
                got = R.round16(dt, y[:rows].astype(np.float64)).astype(np.float32)
                one, more = R.ln16_ulp_counts(dt, got, ref[:rows])
                print(f"d={d} {kind} rows={rows} {dt}: {one} of {got.size} elements across a rounding boundary")
                assert more == 0 and one <= R.LN_ULP_CAP / 4 * got.size, (kind, rows, dt, one, got.size)
                R.assert_ln16(dt, got, ref[:rows])
        if kind == "constant":
            assert np.array_equal(y, np.broadcast_to(b, y.shape))


@pytest.mark.parametrize("d", G.LN_D)
def test_variance_without_the_mean_is_rejected(d):
    """On the offset rows by every comparator; on the N(0, 1) rows, whose mean is nearly 0, by the f32 one."""
    for rows in G.LN_ROWS:
        x, g, b = R.ln_inputs("offset", 8, d, G.ln_seed("offset", d))
        ref = R.layer_norm64(x[:rows], g, b)
        wrong = _ln_no_mean_in_variance(x[:rows], g, b)
        assert R.rel_err_plain(wrong, ref) > R.LN_F32_TOL
        for dt in ("bf16", "f16"):
            _fails(R.assert_ln16, dt, R.round16(dt, wrong.astype(np.float64)).astype(np.float32), ref)
        x, g, b = R.ln_inputs("normal", 8, d, G.ln_seed("normal", d))
        assert R.rel_err_plain(_ln_no_mean_in_variance(x[:rows], g, b), R.layer_norm64(x[:rows], g, b)) > R.LN_F32_TOL


# ---- e4m3 rows ------------------------------------------------------------------------------------------------------------------------
def _quantise(y, div):
    y = np.asarray(y, np.float32)
    s = (np.abs(y).max(-1) / np.float32(div)).astype(np.float32)
    inv = (np.float32(1.0) / s).astype(np.float32)
    return R.e4m3_encode(R.Hh.e4m3_round((y * inv[:, None]).astype(np.float32))), s


@pytest.mark.parametrize("rows,d", [(5, 128), (8, 1280), (3, 2048)])
def test_fp8_layernorm_comparator(rows, d):
    for kind in ("normal", "offset"):
        x, g, b = R.ln_inputs(kind, rows, d, G.ln_seed(kind, d))
        ref = R.layer_norm64(x, g, b)
        tol = R.LN_F32_TOL * np.abs(ref).max()
        y = R.layer_norm_f32(x, g, b)
        R.assert_fp8_rows(*_quantise(y, 448.0), ref, tol, tol)
        _fails(R.assert_fp8_rows, *_quantise(y, 240.0), ref, tol, tol)                  # the e4m3fnuz maximum
        codes, s = _quantise(y, 448.0)
        codes[rows - 1, d - 1] ^= 1                                                     # one byte, one step off
        _fails(R.assert_fp8_rows, codes, s, ref, tol, tol)
        _fails(R.assert_fp8_rows, *_quantise(_ln_no_mean_in_variance(x, g, b), 448.0), ref, tol, tol) if kind == "offset" else None


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("rows,K", [(5, 8), (8, 128), (3, 1280)])
def test_quant_rows_reference_rejects_the_other_maximum(dt, rows, K):
    rng = np.random.default_rng(rows * 31 + K)
    x = (rng.standard_normal((rows, K)) * np.logspace(-2, 2, rows)[:, None]).astype(np.float32)
    want, want_s = R.quant_rows_ref(dt, x)
    x16 = R.round16(dt, x).astype(np.float32)
    codes, s = _quantise(x16, 448.0)
    assert np.array_equal(s, want_s)
    R.assert_exact(R.e4m3_table()[codes], want)
    codes, s = _quantise(x16, 240.0)
    assert not np.array_equal(s, want_s)
    _fails(R.assert_exact, R.e4m3_table()[codes], want)


def test_number_format_helpers():
    t = R.e4m3_table()
    assert t[0x7E] == 448.0 and t[0x08] == 2.0 ** -6 and t[0x01] == 2.0 ** -9 and np.isnan(t[0x7F]) and t[0xB8] == -1.0
    fin = t[~np.isnan(t)]
    assert np.array_equal(R.Hh.e4m3_round(fin), fin) and np.array_equal(t[R.e4m3_encode(fin[fin != 0])], fin[fin != 0])
    x = np.asarray([1.0, 1.00390625, 1.01171875, 300.5, -300.5, 65504.0, 2.0 ** -20, R.SENTINEL])
    assert R.round16("bf16", x).tolist() == [1.0, 1.0, 1.015625, 300.0, -300.0, 65536.0, 2.0 ** -20, R.SENTINEL]      # ties to even
    assert np.array_equal(R.round16("f16", x), x.astype(np.float16).astype(np.float64))
    for dt in ("bf16", "f16"):
        v = R.round16(dt, np.linspace(-3, 3, 4001))
        u = np.unique(v)
        assert np.array_equal(np.diff(R.ordinal16(dt, u)) >= 1, np.ones(len(u) - 1, bool))
        assert R.ordinal16(dt, np.float32(1.0)) + 1 == R.ordinal16(dt, np.float32(1.0 + (2.0 ** -7 if dt == "bf16" else 2.0 ** -10)))
