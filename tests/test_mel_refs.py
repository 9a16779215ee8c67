"""The float64 log-mel reference of tests/mel_refs.py held to what it must agree with before the GPU tests lean on it (no GPU):
the oracle and the transformers golden inside the existing 1e-4, its own FFT against a direct matrix DFT to a tenth of the GPU bar
on every case, the closed form of the impulse frames, and the CPU gap the GPU bar is derived from."""
import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from oracle import mel as OM
from tests import helpers as Hh
from tests import mel_refs as R

MELS = (128, 80)


def _hf(feats_tm):
    return np.ascontiguousarray(feats_tm.T)


@pytest.mark.parametrize("n_mels", MELS)
def test_reference_agrees_with_the_oracle(n_mels):
    """every case against oracle.mel.log_mel (f32 after the power spectrum): inside the suite's 1e-4; measured <= 1.2e-5"""
    worst = 0.0
    for name in R.CASE_NAMES:
        xp, _ = OM.pad_or_trim(R.clip(name))
        want = OM.log_mel(xp[None], n_mels)[0]
        worst = max(worst, float(np.abs(_hf(R.case_reference(name, n_mels)[2]) - want).max()))
    assert worst < 1e-4, worst


@pytest.mark.parametrize("kind,n", [("noise", 480000), ("mixed", 320000), ("chirp", 480000), ("noise_short", 12345)])
def test_reference_agrees_with_the_transformers_golden(kind, n):
    g = Hh.gold_npz("mel_golden.npz")
    x = syn.synth_audio(1, n, kind.split("_")[0])
    feats = _hf(R.reference(x, 128)[2])
    assert R.n_frames(len(x)) == int(g[f"{kind}_nframes"])
    assert np.abs(feats[:, ::5] - g[f"{kind}_feats_sub"]).max() < 1e-4


@pytest.mark.parametrize("n_mels", MELS)
def test_fft_and_direct_dft_agree_on_every_case(n_mels):
    """The condition under which the reference alone stays inside the bar: its FFT and a direct float64 matrix DFT of the same
    frames give the same raw log spectrum to a tenth of the GPU tolerance (measured: 3.1e-11, the between-bins sine)."""
    for name in R.CASE_NAMES:
        raw = R.case_reference(name, n_mels)[0]
        d = float(np.abs(R.raw_of(R.power_dft(R.frames(R.clip(name))), n_mels) - raw).max())
        assert d < R.TOL / 10.0, (name, d)


@pytest.mark.parametrize("n_mels", MELS)
@pytest.mark.parametrize("at", R.IMPULSES)
def test_impulse_frames_have_the_closed_form(n_mels, at):
    raw, cmax, _ = R.case_reference(f"impulse_{at}", n_mels)
    want = R.impulse_closed_form(at, n_mels)
    assert np.abs(raw - want).max() < 1e-12
    seen = np.flatnonzero((want > -10.0).any(axis=1))
    assert list(seen) == [t for t in range(R.N_FRAMES) if 0 <= at + 200 - 160 * t < 400]
    if at == 479999:          # the last frame alone sees it, far down the window: a negative maximum, nothing at the floor
        assert list(seen) == [2999] and -3.7 < cmax < -3.2 and raw.min() > cmax - 8.0


@pytest.mark.parametrize("n_mels", MELS)
def test_the_bar_is_four_times_the_f32_emulation_gap(n_mels):
    """TOL comes from here: the largest gap between the float64 reference and its emulation with mel.hip's three f32 roundings,
    over every case; the same emulation rounded to the 16-bit types passes the feats_tm rule of the GPU tests."""
    gap = 0.0
    for name in R.CASE_NAMES:
        raw, _, feats = R.case_reference(name, n_mels)
        em = R.emulate_f32(None, n_mels, P=R._power(name))
        gap = max(gap, float(np.abs(raw - em.astype(np.float64)).max()))
        f32 = np.float32
        em_feats = (np.maximum(em, em.max() - f32(8.0)) + f32(4.0)) / f32(4.0)
        assert float(np.abs(em_feats - feats).max()) < R.TOL_FEATS, name
        for dt in ("bf16", "f16"):
            assert R.tm16_violations(dt, R.round16(dt, em_feats), feats) == 0, (name, dt)
    assert 2.0 ** -21 <= gap and 4.0 * gap <= R.TOL * 1.001, gap
    assert R.TOL >= 4.0 * 2.0 ** -20


def test_case_table_has_the_signs_and_lengths_the_gpu_tests_count_on():
    assert R.case_reference("silence", 128)[1] == -10.0 and np.all(R.case_reference("silence", 128)[2] == -1.5)
    for n_mels in MELS:
        assert -7.2 < R.case_reference("quiet_noise", n_mels)[1] < -6.4
        assert R.case_reference("loud_noise", n_mels)[1] > 10.0
    for n in R.LADDER:
        x = R.clip(f"len_{n}")
        assert len(x) == n and (n == 0 or x[-1] == 1.0)
    assert [R.n_frames(n) for n in (0, 1, 160, 161, 479840, 479841, 480000)] == [0, 1, 1, 2, 2999, 3000, 3000]


def test_round16_matches_numpy_and_the_ordered_map_is_monotonic():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 3.0, np.float32([0.0, -0.0, 1.0, -1.5, 2.0 ** -20, -2.0 ** -20])])
    for dt in ("bf16", "f16"):
        r = R.round16(dt, a)
        assert np.array_equal(R.round16(dt, r), r)
        order = np.argsort(r, kind="stable")
        assert np.all(np.diff(R.ordered16(dt, r)[order]) >= 0)
    b = np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])                      # ties: to even
    assert np.array_equal(R.round16("bf16", b), np.float32([1.0, 1.0 + 2.0 ** -6]))
