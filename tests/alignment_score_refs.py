"""Float64 definition of the alignment scores (cw_set_alignment_scores; align_path_score_kernel in csrc/align.hip) and the
error bounds the GPU tests hold the kernel to.  Plain numpy, no engine.

For one sequence with n frames (the columns that reached the DTW), rows w[h][i][0 .. n-1] of the Ha alignment heads, the DTW's
first frames fc[0 .. N-1] (fc[N] := n) and a collar of c >= 0 frames, token i has
    lo = fc[i], hi = max(lo + 1, fc[i+1]), window = [max(0, lo - c), min(n, hi + c))
    T_h = sum_j w[h][i][j],  p_h[j] = w[h][i][j] / T_h,  pbar[j] = mean_h p_h[j]
    mass   = sum of pbar[j] over the window
    spread = 0.02 * sqrt(sum_j pbar[j] (j - mu)^2) seconds,  mu = sum_j pbar[j] j
both NaN when n == 0, when any T_h == 0 or when fc[i] < 0.  Frames at or beyond n never enter a sum."""
import numpy as np

FRAME_S = 0.02
U = 2.0 ** -24                  # unit round-off of float32


def timestamp_ncols(num_frames, S=1500):
    """The frames that reach the DTW, as the engine's timestamp_ncols computes them: python's ``[..., : nf // 2]`` applied twice
    when every item has the same num_frames, once otherwise."""
    nf = [int(x) for x in num_frames]
    uniform = all(x == nf[0] for x in nf)
    out = []
    for x in nf:
        n1 = len(range(S)[: x // 2])
        out.append(len(range(n1)[: x // 2]) if uniform else n1)
    return out


def token_variance(w, n, fc, collar):
    """(mass [N], variance in frames^2 [N]) in float64.  w [Ha][N][>= n]; fc [N]."""
    w = np.asarray(w, np.float64)
    Ha, N = w.shape[0], w.shape[1]
    fc = [int(x) for x in fc]
    mass, var = np.full(N, np.nan), np.full(N, np.nan)
    if n <= 0:
        return mass, var
    j = np.arange(n, dtype=np.float64)
    for i in range(N):
        lo = fc[i]
        if lo < 0:
            continue
        hi = max(lo + 1, fc[i + 1] if i + 1 < N else n)
        a, b = max(0, lo - collar), min(n, hi + collar)
        rows = w[:, i, :n]
        T = rows.sum(axis=1)
        if np.any(T == 0):
            continue
        pbar = (rows / T[:, None]).mean(axis=0)
        mass[i] = pbar[a:b].sum() if b > a else 0.0
        mu = float((pbar * j).sum())
        var[i] = float((pbar * (j - mu) ** 2).sum())
    return mass, var


def token_scores(w, n, fc, collar):
    """(mass [N], spread in seconds [N]) in float64."""
    mass, var = token_variance(w, n, fc, collar)
    return mass, FRAME_S * np.sqrt(var)


def word_scores(groups, mass, spread):
    """Per word (mass, spread): the float64 mean over the word's token group (indices into the concatenation of all windows'
    tokens); NaN if any member is NaN.  A token in no group counts in no word."""
    mass, spread = np.asarray(mass, np.float64), np.asarray(spread, np.float64)
    out = []
    for g in groups:
        g = np.asarray(g, np.int64).reshape(-1)
        out.append((float(np.mean(mass[g])), float(np.mean(spread[g]))) if g.size else (float("nan"), float("nan")))
    return out


def mass_tolerance(n):
    """|mass_kernel - mass_float64| <= 2 n u: the worst case of a ratio of two float32 sums of n non-negative terms (each sum
    carries a relative error below n u, the ratio is at most 1)."""
    return 2.0 * n * U


U64 = 2.0 ** -53                # ... and of float64, in which this reference itself computes


def spread_interval(var, n):
    """[lo, hi] seconds for the kernel's spread given the float64 variance ``var`` (frames^2) over n frames: the mass bound
    applied to the variance, var (1 -+ 2 n u), carried through the square root, and one rounding to float32 (derivation:
    tests/test_gpu_alignment_scores.py).  The only slack besides is this reference's own: its centre mu is a float64 sum of n
    terms below n, off by at most d = n^2 u64, which moves its variance by at most d^2 (about 1e-21 frames^2 at n = 1500)."""
    e = 2.0 * n * U
    d = float(n) * n * U64
    lo = FRAME_S * np.sqrt(np.maximum(var * (1.0 - e) - d * d, 0.0)) * (1.0 - 2 * U)
    hi = FRAME_S * np.sqrt(var * (1.0 + e) + d * d) * (1.0 + 2 * U)
    return lo, hi


def check_against(mass_got, spread_got, w, n, fc, collar, where=""):
    """Asserts one sequence's kernel output [N] against the definition: NaN positions exactly, the values within the bounds."""
    mass_got, spread_got = np.asarray(mass_got), np.asarray(spread_got)
    mass, var = token_variance(w, n, fc, collar)
    assert np.array_equal(np.isnan(mass_got), np.isnan(mass)), (where, "mass NaN positions", mass_got, mass)
    assert np.array_equal(np.isnan(spread_got), np.isnan(var)), (where, "spread NaN positions", spread_got, var)
    ok = ~np.isnan(mass)
    if not ok.any():
        return 0.0
    err = np.abs(mass_got[ok].astype(np.float64) - mass[ok])
    assert np.all(err <= mass_tolerance(n)), (where, "mass", float(err.max()), mass_tolerance(n))
    lo, hi = spread_interval(var[ok], n)
    s = spread_got[ok].astype(np.float64)
    assert np.all((s >= lo) & (s <= hi)), (where, "spread", s, lo, hi)
    return float(err.max())
