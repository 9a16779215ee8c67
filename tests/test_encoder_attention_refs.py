"""Host-side proof that the comparisons of tests/test_gpu_encoder_attention.py bite (no GPU).  A numpy restatement of the
64-queries-per-wave kernel's arithmetic (R.attn_q64_emulation: 64-key tiles, the per-lane-group mask of the peeled tile, the
deferred rescale, 16-bit P, one rounding of the output) passes every comparator on the GPU tests' own inputs; with one fault
planted -- a lost key, an admitted pad key, the wrong mask stride, V rows or output chunks swapped, the wrong query clamp, a
skipped rescale, a frozen running max -- it fails the comparators named in CAUGHT_BY.  Also holds what the one-hot equality
rests on: on every shape and seed the GPU tests use, every other score lies at least 120 below the selected one."""
import functools

import numpy as np
import pytest

from tests import encoder_refs as R
from tests import test_gpu_encoder_attention as G

ONEHOT_SHAPES = sorted({(1, 1, S) for S in sum(G.ONEHOT_SWEEPS.values(), ())} | {(2, 3, S) for S in G.ONEHOT_BATCHED}
                       | {((2, 3) if S < 100 else (1, 1)) + (S,) for S in G.ONEHOT_POISONED} | {(1, 1, 5), (1, 2, 9)})


# ---- what the exact comparison rests on ------------------------------------------------------------------------------------------------
def test_onehot_margin_on_every_shape_in_use():
    """selected score 576, every other at least ATTN_MARGIN lower: e^-120 and below is 0 in f32 (smallest subnormal e^-103.3), so the
    softmax is one-hot to the bit; V is exact in both 16-bit types, no V row repeats inside a head and none holds the sentinel"""
    worst = np.inf
    for B, H, S in ONEHOT_SHAPES:
        q, k, v, pi = R.attn_onehot_case(B, H, S)
        for b in range(B):
            for h in range(H):
                assert sorted(pi[b, h]) == list(range(S)), (B, H, S, "pi is no permutation")
                assert len(np.unique(v[b, h], axis=0)) == S, (B, H, S, "two equal V rows: a misrouted key would not show")
        m = R.attn_onehot_margin(q, k, pi)
        assert m >= R.ATTN_MARGIN, (B, H, S, m)
        worst = min(worst, m)
        for dt in ("bf16", "f16"):
            assert np.array_equal(R.round16(dt, v), v) and np.array_equal(R.round16(dt, k), k)
        assert np.abs(v).max() < R.SENTINEL / 8
    print(f"smallest margin over {len(ONEHOT_SHAPES)} shapes: {worst}")
    assert np.exp(np.float32(-R.ATTN_MARGIN)) == 0.0 and 2.0 ** np.float32(-R.ATTN_MARGIN * 1.4426950408889634) < 2.0 ** -149


def test_builders_give_what_the_cases_claim():
    for S in G.PAD_S:
        for const in (False, True):
            q, k, v, ref = R.attn_padkey_case(1, 2, S, const)
            s = np.einsum("bhqd,bhkd->bhqk", q, k)
            assert np.all(s == -576.0)                                         # common score <= -500: a pad key (score 0) takes all
            assert R.attn_row_err(R.attention64(q, k, v), ref) < 1e-12        # float64 round-off of the plain reference
            if const:
                assert np.all(v == v[:, :, :1])
    lev = R.attn_stair_levels("up5_jump40", 1500)
    assert lev[11] == 55.0 and lev[12] == 100.0 and lev[23] == 155.0
    assert R.attn_stair_levels("up5_jump40", 700).tolist() == [0, 5, 10, 15, 20, 25, 70, 75, 80, 85, 90]
    assert R.attn_stair_levels("up8.5", 1500)[23] == 195.5                     # no bf16 number: split over the two half vectors
    for kind in R.STAIR_KINDS:
        for S in G.STAIR_S:
            R.attn_stair_case(kind, 1, 2, S)                                   # asserts exact operands and exact scores itself
    for dt in G.DTS:
        q, k, v = R.attn_realistic_case(dt, 2, 3, 257)
        s = np.einsum("bhqd,bhkd->bhqk", q, k)
        assert 3.5 < s[..., 1:].std() < 4.5
        assert abs((s[..., 0].mean() - s[..., 1:].mean()) - 12.0) < 0.5


def test_row_error_sees_one_bad_row():
    ref = np.ones((1, 4, 128)); ref[0, 0] = 1000.0
    got = ref.copy(); got[0, 3, 70] = 1.5
    assert R.attn_row_err(got, ref) == 0.5 and R.rel_err_plain(got, ref) < 1e-3
    got[0, 2, 0] = np.nan
    assert R.attn_row_err(got, ref) == np.inf


# ---- the comparators of the GPU tests, as callables on an attention implementation --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _onehot(B, H, S):
    q, k, v, pi = R.attn_onehot_case(B, H, S)
    return q, k, v, R.attn_onehot_want(v, pi)


@functools.lru_cache(maxsize=None)
def _padkey(S, const):
    return R.attn_padkey_case(1, 2, S, const)


@functools.lru_cache(maxsize=None)
def _stair(kind, S):
    q, k, v = R.attn_stair_case(kind, 1, 2, S)
    return q, k, v, R.attention64(q, k, v)


@functools.lru_cache(maxsize=None)
def _real(dt, S):
    q, k, v = R.attn_realistic_case(dt, 2, 3, S)
    return q, k, v, R.attention64(q, k, v)


def _cmp_onehot(B, H, S):
    def check(dt, attn):
        q, k, v, want = _onehot(B, H, S)
        R.assert_exact(attn(dt, q, k, v), want)
    return check


def _cmp_padkey(S):
    def check(dt, attn):                                                       # G._check_padkeys
        if not (dt == "bf16" and S >= 1000):
            q, k, v, ref = _padkey(S, False)
            R.assert_attn_rows("padkey", S, dt, attn(dt, q, k, v), ref)
        q, k, v, ref = _padkey(S, True)
        if dt == "f32":
            R.assert_attn_rows("padkey_const", S, dt, attn(dt, q, k, v), ref)
        else:
            R.assert_within_one_ulp16(dt, attn(dt, q, k, v), ref)
    return check


def _cmp_stair(kind, S):
    def check(dt, attn):
        q, k, v, ref = _stair(kind, S)
        R.assert_attn_rows(kind, S, dt, attn(dt, q, k, v), ref)
    return check


def _cmp_real(S):
    def check(dt, attn):
        q, k, v, ref = _real(dt, S)
        R.assert_attn_rows("realistic", S, dt, attn(dt, q, k, v), ref)
    return check


COMPARATORS = {}
for _S in (1, 2, 17, 63, 64, 65, 300, 1500):
    COMPARATORS[f"onehot-{_S}"] = _cmp_onehot(1, 1, _S)
COMPARATORS["onehot-2x3-65"] = _cmp_onehot(2, 3, 65)
for _S in G.PAD_S:
    COMPARATORS[f"padkey-{_S}"] = _cmp_padkey(_S)
for _kind in R.STAIR_KINDS:
    for _S in G.STAIR_S:
        COMPARATORS[f"{_kind}-{_S}"] = _cmp_stair(_kind, _S)
for _S in G.REAL_S:
    COMPARATORS[f"realistic-{_S}"] = _cmp_real(_S)
QUICK = [n for n in COMPARATORS if not n.endswith("-1500") or n in ("onehot-1500", "padkey-1500", "up5_jump40-1500")]

# The comparators every 16-bit engine must fail with the fault planted (others may fail too):
#   a lost last key / V halves / output chunks: every one-hot size -- at S = 1 the lost key leaves no key at all (NaN);
#   an admitted pad key has score 0 against 576 in the one-hot cases (invisible) and against -576 in the pad-key cases (all the mass);
#   the g * 8 mask stride drops keys only where the remainder is at least 5: S = 1, 2 (and 64: no masked tile) pass it;
#   the query clamp needs a second row; a skipped rescale of O needs a second tile.
UP = [f"{k}-700" for k in R.STAIR_KINDS if k != "down5"]
CAUGHT_BY = {
    "drop_last_key": [f"onehot-{S}" for S in (1, 2, 17, 63, 64, 65, 300, 1500)],
    "admit_pad_key": [f"padkey-{S}" for S in G.PAD_S],
    "mask_stride_8": [f"onehot-{S}" for S in (17, 63, 300, 1500)],
    "swap_v_halves": [f"onehot-{S}" for S in (1, 2, 17, 63, 64, 65, 300, 1500)],
    "swap_out_chunks": [f"onehot-{S}" for S in (1, 2, 17, 63, 64, 65, 300, 1500)],
    "clamp_q_s_minus_2": [f"onehot-{S}" for S in (2, 17, 63, 64, 65, 300, 1500)],
    "skip_o_rescale": [f"onehot-{S}" for S in (65, 300, 1500)] + UP,
    "max_frozen_f16_p": UP + ["up5_jump40-1500"],
}


def _failing(dt, attn, names):
    bad = []
    for n in names:
        try:
            COMPARATORS[n](dt, attn)
        except AssertionError:
            bad.append(n)
    return bad


@pytest.mark.parametrize("dt", G.DTS)
def test_emulation_passes_every_comparator(dt):
    assert _failing(dt, R.attn_q64_emulation, list(COMPARATORS)) == []


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_emulation_is_exact_on_the_small_onehot_sweeps(dt):
    for sweep in ("1-64", "seams", "257-320"):
        for S in G.ONEHOT_SWEEPS[sweep]:
            _cmp_onehot(1, 1, S)(dt, R.attn_q64_emulation)


@pytest.mark.parametrize("fault", R.ATTN_FAULTS)
def test_planted_fault_is_rejected(fault):
    assert sorted(CAUGHT_BY) == sorted(R.ATTN_FAULTS)
    for dt in ("bf16", "f16"):
        bad = _failing(dt, lambda d, q, k, v: R.attn_q64_emulation(d, q, k, v, fault=fault), QUICK)
        print(f"{fault} {dt}: rejected by {bad}")
        missing = [n for n in CAUGHT_BY[fault] if n not in bad]
        assert bad and not missing, (fault, dt, "not rejected by", missing)


def test_remainders_where_the_mask_stride_shows():
    """g * 8 in place of g * 4 loses a key for every remainder S % 64 >= 5 -- each of those is in the sweeps, in the first tile
    (S = 5 .. 63) and behind four full ones (S = 261 .. 319)"""
    for S in tuple(range(1, 64)) + tuple(range(257, 320)):
        q, k, v, want = _onehot(1, 1, S)
        same = np.array_equal(R.attn_q64_emulation("bf16", q, k, v, fault="mask_stride_8"), want)
        assert same == (S % 64 < 5), S
