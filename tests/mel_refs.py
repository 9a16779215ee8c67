"""Float64 reference of the log-mel front end (csrc/mel.hip), built from the definition, in the three stages the kernels produce,
and the case table the CPU tests (tests/test_mel_refs.py) and the GPU tests (tests/test_gpu_mel.py) share.

    raw    [3000][n_mels]  log10(max(P F, 1e-10)); P [3000][201] the float64 power spectrum of the reflect-padded frames (hop 160,
                           400 samples) under the periodic Hann window rounded to f32 (torch.hann_window is f32; the engine rounds
                           its table the same way), F [201][n_mels] the slaney bank of oracle/mel.py rounded to f32, used in float64
    cmax                   the clip maximum of raw
    feats  [3000][n_mels]  (max(raw, cmax - 8) + 4) / 4, time-major

`emulate_f32` repeats the computation with the three f32 roundings mel.hip documents (power -> f32, mel sum -> f32, log10 evaluated
in f32).  The GPU tolerance is derived from the gap between the two on the CPU, never from the kernels: see TOL below.

Tolerance.  Largest |raw - emulate_f32 raw| over every case of the table, measured on the CPU (test_mel_refs.py asserts that four
times the gap it measures stays inside the bar): 1.27e-6 at 128 mels and at 80 mels (loud_noise; 9.5e-7 on every value at the clamp,
where numpy's f32 log10 of 1e-10f is one unit in the last place away from -10) -- the rounding of the f32 log10 result itself at
magnitude 8 .. 16; the f32 roundings of the power and of the mel sum add 3e-8 each.  Four times that gap is 5.08e-6, above the floor
the bar may never go below (4 ulp of f32 at magnitude 10 = 4 * 2^-20 = 3.8e-6: the device log10f is another implementation than
numpy's).  TOL = 5.08e-6 on raw and on the clip maximum, TOL / 4 = 1.27e-6 on the features."""
from __future__ import annotations

import functools

import numpy as np

from oracle import mel as OM

N_FFT, HOP, N_SAMPLES, N_FRAMES, N_BINS = 400, 160, 480000, 3000, 201

CPU_GAP = 1.27e-6                               # measured: see the module docstring
TOL = max(4.0 * CPU_GAP, 4.0 * 2.0 ** -20)      # 5.08e-6
TOL_FEATS = TOL / 4.0


def window() -> np.ndarray:
    return OM.hann_periodic().astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def bank(n_mels: int) -> np.ndarray:
    """[201][n_mels]: the slaney bank rounded to f32, as float64"""
    return OM.mel_filter_bank(n_mels).astype(np.float32).astype(np.float64)


def frames(x) -> np.ndarray:
    """[3000][400] float64: the clip zero-padded to 30 s, reflect-padded by 200 (center=True), cut at hop 160, windowed"""
    x = np.asarray(x, np.float32)
    assert x.ndim == 1 and len(x) <= N_SAMPLES
    pad = np.zeros(N_SAMPLES, np.float64)
    pad[:len(x)] = x
    xp = np.concatenate([pad[N_FFT // 2:0:-1], pad, pad[-2:-N_FFT // 2 - 2:-1]])
    idx = np.arange(N_FFT)[None, :] + HOP * np.arange(N_FRAMES)[:, None]
    return xp[idx] * window()[None, :]


def power_fft(fr) -> np.ndarray:
    s = np.fft.rfft(fr, axis=1)
    return s.real ** 2 + s.imag ** 2


@functools.lru_cache(maxsize=None)
def _dft_basis():
    ph = (np.arange(N_FFT)[:, None] * np.arange(N_BINS)[None, :]) % N_FFT          # exact phase reduction
    ang = 2.0 * np.pi * ph / N_FFT
    return np.cos(ang), np.sin(ang)


def power_dft(fr) -> np.ndarray:
    """the same power spectrum as a direct float64 matrix DFT (no FFT)"""
    c, s = _dft_basis()
    re, im = fr @ c, fr @ s
    return re ** 2 + im ** 2


def raw_of(P, n_mels: int) -> np.ndarray:
    return np.log10(np.maximum(P @ bank(n_mels), 1e-10))


def stages(raw):
    """(raw, cmax, feats) of a raw log spectrum, float64"""
    cmax = float(raw.max())
    return raw, cmax, (np.maximum(raw, cmax - 8.0) + 4.0) / 4.0


def reference(x, n_mels: int, P=None):
    return stages(raw_of(power_fft(frames(x)) if P is None else P, n_mels))


def emulate_f32(x, n_mels: int, P=None) -> np.ndarray:
    """raw with the three f32 roundings of mel.hip: the power spectrum (f64 DFT) is rounded to f32, the mel sum (f64 accumulation of
    f32 x f32 products) is rounded to f32, log10 of max(., 1e-10f) is evaluated in f32"""
    P = power_fft(frames(x)) if P is None else P
    mel = (P.astype(np.float32).astype(np.float64) @ bank(n_mels)).astype(np.float32)
    return np.log10(np.maximum(mel, np.float32(1e-10))).astype(np.float32)


def n_frames(n: int) -> int:
    return (n + HOP - 1) // HOP


# ---- 16-bit rounding by the engine's rule (csrc/common.h: round to nearest even) ---------------------------------------------
def round16(dt: str, a) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    if dt == "bf16":
        u = a.view(np.uint32)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    if dt == "f16":
        return a.astype(np.float16).astype(np.float32)
    return a


def ordered16(dt: str, a) -> np.ndarray:
    """values of the 16-bit type `dt` (held in f32) -> integers in which neighbouring representable values differ by one"""
    a = np.ascontiguousarray(a, np.float32)
    bits = (a.view(np.uint32) >> 16).astype(np.int64) if dt == "bf16" else a.astype(np.float16).view(np.uint16).astype(np.int64)
    return np.where(bits & 0x8000, -(bits & 0x7FFF), bits)


def tm16_violations(dt: str, got_tm, ref_feats) -> int:
    """Elements of a 16-bit feats_tm that are neither within one unit in the last place of the reference rounded to the type nor
    between the roundings of ref - TOL_FEATS and ref + TOL_FEATS.  The second clause matters only next to zero (raw next to -4),
    where the spacing of the 16-bit type falls below the f32 tolerance the features themselves are held to: there a kernel that is
    right to that tolerance can land several tiny units away, and the rounding of the tolerance interval's two ends is the sharpest
    statement that holds.  Everywhere else the interval's ends round to the reference's own value or its neighbour, so the clause
    adds nothing to the one-unit bound."""
    ref = np.asarray(ref_feats, np.float64)
    o = ordered16(dt, got_tm)
    near = np.abs(o - ordered16(dt, round16(dt, ref.astype(np.float32)))) <= 1
    lo = ordered16(dt, round16(dt, (ref - TOL_FEATS).astype(np.float32)))
    hi = ordered16(dt, round16(dt, (ref + TOL_FEATS).astype(np.float32)))
    return int(np.count_nonzero(~(near | ((o >= lo) & (o <= hi)))))


# ---- the case table ----------------------------------------------------------------------------------------------------------
LADDER = (0, 1, 159, 160, 161, 199, 200, 201, 399, 400, 401, 5119, 5120, 5121, 479839, 479840, 479999, 480000)
IMPULSES = (0, 5119, 479999)


def _noise(seed, n, sigma):
    return (np.random.default_rng(seed).standard_normal(n) * sigma).astype(np.float32)


def _impulse(at):
    x = np.zeros(at + 1, np.float32)
    x[at] = 1.0
    return x


def _ladder(n):
    x = _noise(1000 + n, n, 0.1)
    if n:
        x[-1] = 1.0                     # an off-by-one in the length shows
    return x


def _sine(hz):
    return np.sin(2.0 * np.pi * hz * np.arange(N_SAMPLES) / 16000.0).astype(np.float32)


CASES = {
    "silence": lambda: np.zeros(1000, np.float32),
    **{f"impulse_{at}": functools.partial(_impulse, at) for at in IMPULSES},
    "dc": lambda: np.ones(N_SAMPLES, np.float32),
    "sine_bin100": lambda: _sine(4000.0),
    "alternating_bin200": lambda: (1.0 - 2.0 * (np.arange(N_SAMPLES) % 2)).astype(np.float32),
    "sine_1234p5hz": lambda: _sine(1234.5),
    "quiet_noise": lambda: _noise(7, 201, 1e-4),
    "loud_noise": lambda: _noise(8, 479999, 20000.0),
    **{f"len_{n}": functools.partial(_ladder, n) for n in LADDER},
}
CASE_NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def clip(name: str) -> np.ndarray:
    x = CASES[name]()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _power(name: str) -> np.ndarray:
    P = power_fft(frames(clip(name)))
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def case_reference(name: str, n_mels: int):
    """(raw, cmax, feats) of a case, computed once per process and read-only"""
    raw, cmax, feats = reference(None, n_mels, P=_power(name))
    raw.setflags(write=False)
    feats.setflags(write=False)
    return raw, cmax, feats


def impulse_closed_form(at: int, n_mels: int) -> np.ndarray:
    """raw of a unit impulse at sample `at`: the frame that holds it at window position n has the flat power w[n]^2, so its mel sum
    is w[n]^2 * sum_k F[k][m]; every other frame is at the clamp"""
    raw = np.full((N_FRAMES, n_mels), -10.0)
    w, colsum = window(), bank(n_mels).sum(axis=0)
    for t in range(N_FRAMES):
        n = at + N_FFT // 2 - HOP * t
        if 0 <= n < N_FFT:
            raw[t] = np.log10(np.maximum(w[n] ** 2 * colsum, 1e-10))
    return raw
