"""GPU parity tests of encoder self-attention, one launch at a time (cw_test_attention), against plain numpy float64
(tests/encoder_refs.py): which key, V row and output column every query reaches (bit for bit), the key-validity mask of the
peeled last tile, the deferred rescale of the running max, and a realistic score distribution judged row by row.  The output
buffer starts as a sentinel, the hook keeps guard rows behind it, and K / V pad rows are zero as in the engine.

Which kernel body a case reaches (cw_launch_attn_encoder in csrc/attention.hip): f32 engine -> attn_encoder_f32_kernel; 16-bit
engines -> attn_encoder_q64_kernel<4>, full tiles a3_tile<false> for S >= 64 and the peeled masked tile a3_tile<true> for
S % 64 != 0; CW_ATTN_V1=1 on the experiments build (child process) -> attn_encoder_bf16_kernel, 32 queries per wave.
tests/test_encoder_attention_refs.py shows on the CPU that these comparisons reject a lost or extra key, a wrong mask stride, a
misrouted V row or output chunk, a wrong query clamp and a wrong rescale."""
import os

import numpy as np
import pytest

from crisperwhisper_amd.engine import Engine, EngineError
from tests import encoder_refs as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DTS = ("f32", "bf16", "f16")
# one-hot sweeps at B = H = 1: every S of the first tile; the tile and q-block seams; every remainder S % 64 behind four full tiles
# and a full 256-query block, the last q-block partial; the sizes around the model's 1500 frames
ONEHOT_SWEEPS = {"1-64": tuple(range(1, 65)), "seams": (65, 127, 128, 129), "257-320": tuple(range(257, 321)),
                 "large": (511, 512, 1499, 1500)}
ONEHOT_BATCHED = (1, 63, 65, 257, 320, 1500)      # B = 2, H = 3
ONEHOT_POISONED = (1, 63, 65, 300, 1499)          # (B, H) = (2, 3) below 100, (1, 1) above
PAD_S = (1, 63, 65, 200, 257, 1499, 1500)
STAIR_S = (1500, 700)
REAL_S = (1500, 257)


@pytest.fixture(scope="module")
def engines():
    g, v, W, spec = Hh.tiny_setup()
    out = {}
    for dt in DTS:
        out[dt] = Engine(spec, dtype=dt, max_batch=4)
    yield out
    for e in out.values():
        e.close()


def _audit(key, e):
    print(f"measured {key}: {e:.3e}")
    log = os.environ.get("CW_TEST_ERRLOG")                       # tolerance audit: CW_TEST_ERRLOG=<file> records every measured error
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{key}\t{e:.3e}\n")


def _run(eng, q, k, v):
    B, H, S, _ = q.shape
    return eng.test_attention(q, k, v, out0=np.full((B, S, H * 64), R.SENTINEL, np.float32))


# ---- a: one-hot routing -------------------------------------------------------------------------------------------------------------
def _check_onehot(eng, dt, B, H, S):
    q, k, v, pi = R.attn_onehot_case(B, H, S)
    got = _run(eng, q, k, v)
    R.assert_exact(got, R.attn_onehot_want(v, pi), (dt, "one-hot", B, H, S))      # no sentinel left: every row < S was written
    return got


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("sweep", list(ONEHOT_SWEEPS))
def test_onehot_routing_sweep(engines, dt, sweep):
    """Query i is key pi(i) (+-3 sign codes, selected score 576, every other at least 120 lower): out[i] == V[pi(i)] exactly, V with
    a column scale.  A dropped key, a V row or an output column in the wrong place, a query row from elsewhere all change bits."""
    for S in ONEHOT_SWEEPS[sweep]:
        _check_onehot(engines[dt], dt, 1, 1, S)


@pytest.mark.parametrize("dt", DTS)
def test_onehot_routing_batched_heads(engines, dt):
    """B = 2, H = 3: head offsets with S_pad != S, the XCD-aware block order, rows of the next batch item right behind row S-1."""
    for S in ONEHOT_BATCHED:
        _check_onehot(engines[dt], dt, 2, 3, S)


@pytest.mark.parametrize("dt", DTS)
def test_onehot_with_nan_query_padding(engines, dt):
    """Q rows S .. S_pad-1 hold NaN: the kernels clamp query loads to row S-1, so nothing changes."""
    _check_nan_query_padding(engines[dt], dt)


def _check_nan_query_padding(eng, dt):
    for S in ONEHOT_POISONED:
        B, H = (2, 3) if S < 100 else (1, 1)
        plain = _check_onehot(eng, dt, B, H, S)
        assert eng.lib.cw_test_set_option(b"attn_poison_qpad", 1) == 0
        try:
            poisoned = _check_onehot(eng, dt, B, H, S)
        finally:
            eng.lib.cw_test_set_option(b"attn_poison_qpad", 0)
        assert np.array_equal(plain, poisoned), (dt, S)


# ---- b: pad keys ----------------------------------------------------------------------------------------------------------------------
def _check_padkeys(eng, dt, S):
    B, H = 1, 2
    if not (dt == "bf16" and S >= 1000):
        q, k, v, ref = R.attn_padkey_case(B, H, S, constant_v=False)
        R.assert_attn_rows("padkey", S, dt, _run(eng, q, k, v), ref, "mean of V", _audit)
    q, k, v, ref = R.attn_padkey_case(B, H, S, constant_v=True)
    got = _run(eng, q, k, v)
    if dt == "f32":
        R.assert_attn_rows("padkey_const", S, dt, got, ref, "constant V", _audit)
    else:
        R.assert_within_one_ulp16(dt, got, ref, ("constant V", S))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", PAD_S)
def test_pad_keys_take_no_mass(engines, dt, S):
    """All scores -576 (one key vector, q = -k0): the output is the column mean of V, and one admitted zero pad key (score 0) would
    take all of it.  Random V: per-row error against the float64 mean, measured f32 1.2e-7 .. 7.2e-7, f16 2.0e-4 .. 3.8e-4, bf16
    2.0e-3 .. 2.2e-3 (S = 63 .. 257; 0 at S = 1) -- the 16-bit figures are the rounding of the stored mean, up to 2^-9 of an
    element in bf16.  That is six times the 0.5 / S = 3.3e-4 a bf16 bound has to stay under at S >= 1000, so bf16 at S = 1499 and
    1500 is judged on V constant per column instead: sum and mean are exact and the stored output lies within one unit in the last
    place of the constant.  Every engine and size runs that form too; the f32 engine's bound there is the worst case of its S
    roundings, (S + 2) 2^-24.  Bounds of the random form: R.ATTN_TOL, 2.5 x the measured value."""
    _check_padkeys(engines[dt], dt, S)


# ---- c: stale-max staircases ------------------------------------------------------------------------------------------------------------
def _check_stair(eng, dt, kind, S):
    q, k, v = R.attn_stair_case(kind, 1, 2, S)
    R.assert_attn_rows(kind, S, dt, _run(eng, q, k, v), R.attention64(q, k, v), "staircase", _audit)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", STAIR_S)
@pytest.mark.parametrize("kind", R.STAIR_KINDS)
def test_stale_max_staircase(engines, dt, kind, S):
    """Scores constant inside a 64-key tile and stepping between tiles (R.attn_stair_levels): probabilities against a stale max up
    to e^8 (the f16 P fragments), the threshold itself, a move on every tile, no move at all, a stale stretch followed by a +40
    move, and lanes of one wave that disagree about moving.  Per-row error against float64, measured over the twelve cases: f32
    7.6e-8 .. 4.8e-7, bf16 1.3e-3 .. 4.5e-3, f16 1.2e-4 .. 5.7e-4 (largest: up5_rows_x2 / up5_jump40 at S = 1500); each case's own
    figure and bound (2.5 x): R.ATTN_TOL."""
    _check_stair(engines[dt], dt, kind, S)


# ---- d: realistic scores ----------------------------------------------------------------------------------------------------------------
def _check_realistic(eng, dt, S):
    q, k, v = R.attn_realistic_case(dt, 2, 3, S)
    R.assert_attn_rows("realistic", S, dt, _run(eng, q, k, v), R.attention64(q, k, v), "realistic", _audit)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", REAL_S)
def test_realistic_scores_per_row(engines, dt, S):
    """Score standard deviation about 4, an attention sink (+12 on key 0 for every query), column-scaled V, B = 2, H = 3: every
    query row on its own against float64.  Measured S = 1500 / 257: f32 8.1e-6 / 4.2e-6, bf16 9.4e-3 / 6.2e-3, f16 1.1e-3 /
    8.6e-4; bounds 2.5 x (R.ATTN_TOL)."""
    _check_realistic(engines[dt], dt, S)


# ---- the 32-queries-per-wave kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["onehot", "padkeys", "staircase", "realistic"])
def test_v1_kernel(request, engines, what):
    """attn_encoder_bf16_kernel (experiments build, CW_ATTN_V1=1, read once per process: child process): every 16-bit case above."""
    if not (Hh.has_experiments() and os.environ.get("CW_ATTN_V1")):
        return Hh.run_in_child(request, dict(Hh.experiments_env(), CW_ATTN_V1="1"), lambda p: True)
    for dt in ("bf16", "f16"):
        eng = engines[dt]
        if what == "onehot":
            for S in sum(ONEHOT_SWEEPS.values(), ()):
                _check_onehot(eng, dt, 1, 1, S)
            for S in ONEHOT_BATCHED:
                _check_onehot(eng, dt, 2, 3, S)
            _check_nan_query_padding(eng, dt)
        elif what == "padkeys":
            for S in PAD_S:
                _check_padkeys(eng, dt, S)
        elif what == "staircase":
            for kind in R.STAIR_KINDS:
                for S in STAIR_S:
                    _check_stair(eng, dt, kind, S)
        else:
            for S in REAL_S:
                _check_realistic(eng, dt, S)


# ---- the hook ------------------------------------------------------------------------------------------------------------------------------
def test_hook_refuses_empty_shapes(engines):
    """B, H or S < 1: CW_ERR_INVALID before anything is allocated or launched, and the context stays usable."""
    eng = engines["bf16"]
    for shape in [(0, 1, 4, 64), (1, 0, 4, 64), (1, 1, 0, 64)]:
        z = np.zeros(shape, np.float32)
        with pytest.raises(EngineError, match=r"\(-22\)"):
            eng.test_attention(z, z, z)
        _check_onehot(eng, "bf16", 1, 1, 5)


def test_output_is_in_out_and_default_is_zeros(engines):
    """Existing callers pass no out0; with one, the buffer travels to the device and back (shape checked on the host)."""
    eng = engines["f16"]
    q, k, v, pi = R.attn_onehot_case(1, 2, 9)
    assert np.array_equal(eng.test_attention(q, k, v), R.attn_onehot_want(v, pi))
    with pytest.raises(AssertionError):
        eng.test_attention(q, k, v, out0=np.zeros((1, 8, 128), np.float32))
