"""Float64 reference and comparator for the per-token log-probabilities of the sampler kernels (cw_set_token_logprobs;
sample_partial_kernel / sample_kernel in csrc/elementwise.hip), and a float32 numpy model of the kernels' reduction in which
faults can be planted (tests/test_token_logprob_refs.py proves the comparator rejects them).

Definition.  logprob = x[tok] - logsumexp(x[0 .. V-1]) on the raw f32 logits x of the step that wrote `tok`; the pad columns
V .. ldv-1 never count, masked tokens do.

What the kernels do with a row (ldv columns, 16 slices of per4 = ceil(ldv / 4 / 16) float4 groups, 256 threads per slice):
a thread walks n_it = ceil(per4 / 256) groups keeping a running maximum m and s = sum exp(x - m): per group one rescale
s *= expf(m_old - m_new) and up to four additions of expf(x - m); the block then takes the slice maximum, every thread rescales
its s once (expf, one multiplication), a 6-step wave scan and a 4-term sum over the waves add them; sample_kernel rescales the
16 slice sums to the row maximum (expf, one multiplication each), adds them in sequence, and stores
x[tok] - (M + logf(S)).

Bound (first order, u = 2^-24, every term a worst-case sum, nothing fitted to what the kernel returns).
  relative error of S, which is the absolute error of log S:
      u * [ 4 n_it          additions in the thread
          + n_it (1 + 2 E)   its rescales: one multiplication, one expf
          + 2 E              the expf of the term itself
          + (1 + 2 E)        rescale to the slice maximum
          + 6 + 4            wave scan, sum over the four waves
          + (1 + 2 E)        rescale to the row maximum
          + 16 ]             sum over the 16 slice records
    + u * sum_v p_v (max - x_v)     the exponents' arguments: every difference of two f32 numbers is rounded once (relative u of
                                    its size, which the exponential turns into a relative error of that size); along the chain
                                    element -> thread maximum -> slice maximum -> row maximum the sizes add up to max - x_v, and
                                    an element weighs p_v = softmax(x)_v in S
  + 2 L u |log S|                   logf
  + u (|x_tok| + 2 |lse|)           M + logf(S) and the final subtraction
E and L are the errors of expf / logf in ulp (1 ulp = 2 u relative).  The device library implements the accuracy of the OpenCL
full profile, which allows exp and log 3 ulp each: E = L = 3.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
EXPF_ULP = 3
LOGF_ULP = 3
NS = 16            # slices per row (SAMPLE_NS)
THREADS = 256


def reference(x, tok, V):
    """(logprob, lse) in float64 for one row; x may carry pad columns behind V.  An all -inf row has no value: (nan, -inf)."""
    x64 = np.asarray(x[:V], np.float64)
    m = x64.max()
    if not np.isfinite(m):
        return float("nan"), float(m)
    lse = m + np.log(np.exp(x64 - m).sum())
    return float(x64[tok] - lse), float(lse)


def n_iter(V):
    ldv = (V + 3) & ~3
    per4 = ((ldv >> 2) + NS - 1) // NS
    return (per4 + THREADS - 1) // THREADS


def bound(x, tok, V):
    x64 = np.asarray(x[:V], np.float64)
    m = x64.max()
    fin = np.isfinite(x64)
    p = np.zeros_like(x64); p[fin] = np.exp(x64[fin] - m)
    S = p.sum()
    lse = m + np.log(S)
    n = n_iter(V)
    E = EXPF_ULP
    ops = 4 * n + n * (1 + 2 * E) + 2 * E + (1 + 2 * E) + 6 + 4 + (1 + 2 * E) + NS
    arg = float((p[fin] * (m - x64[fin])).sum() / S)
    xt = abs(float(x64[tok])) if np.isfinite(x64[tok]) else 0.0
    return U * (ops + arg) + 2 * LOGF_ULP * U * abs(np.log(S)) + U * (xt + 2 * abs(lse))


def compare(got, x, tok, V):
    """-> (ok, |got - ref|, bound) for one row.  Where the definition gives -inf (a -inf logit at tok) or nothing (an all -inf
    row) the kernel's f32 arithmetic must give the same: -inf, respectively NaN."""
    ref, lse = reference(x, tok, V)
    got = float(got)
    if np.isnan(ref):
        return bool(np.isnan(got)), 0.0, 0.0
    if np.isinf(ref):
        return got == ref, 0.0, 0.0
    b = bound(x, tok, V)
    if not np.isfinite(got):
        return False, float("inf"), b
    return abs(got - ref) <= b, abs(got - ref), b


def check_rows(got, logits, toks, V, what=""):
    """Asserts compare() for every row; prints the worst |error| / bound ratio before it asserts."""
    worst, bad = 0.0, []
    for b in range(len(toks)):
        ok, err, bd = compare(got[b], logits[b], int(toks[b]), V)
        if bd > 0:
            worst = max(worst, err / bd)
        if not ok:
            bad.append((b, int(toks[b]), float(got[b]), reference(logits[b], int(toks[b]), V)[0], err, bd))
    print(f"{what}: {len(toks)} rows, worst |err| / bound = {worst:.3f}")
    assert not bad, (what, bad[:3])


# ---- float32 model of the kernels' reduction, with faults to plant ---------------------------------------------------------
def kernel_model(x, tok, V, dead=None, fault=None):
    """x: f32 row of ldv columns (pad columns behind V hold whatever the logits GEMV left there).  dead: bool [V] of the tokens
    the processors mask (they count all the same).  fault: None, "pad" (pad columns summed), "masked" (masked tokens left out:
    the processed denominator of lp_sum), "norescale" (slice records merged without rescaling to the row maximum)."""
    f32 = np.float32
    x = np.asarray(x, f32)
    ldv = len(x)
    assert ldv % 4 == 0 and ldv >= V
    per4 = ((ldv >> 2) + NS - 1) // NS
    ms, ss = [], []
    for sl in range(NS):
        lo, hi = sl * per4 * 4, min(ldv, (sl + 1) * per4 * 4)
        idx = np.arange(lo, hi)
        keep = idx < (ldv if fault == "pad" else V)
        if fault == "masked" and dead is not None:
            keep &= ~np.concatenate([dead, np.ones(ldv - V, bool)])[idx]
        xs = x[idx[keep]]
        xs = xs[np.isfinite(xs) | (xs > 0)]
        if len(xs) == 0 or not np.isfinite(xs.max()):
            ms.append(f32(-np.inf)); ss.append(f32(0))
            continue
        m = xs.max()
        ms.append(f32(m)); ss.append(np.exp(xs - m, dtype=f32).sum(dtype=f32))
    ms, ss = np.asarray(ms, f32), np.asarray(ss, f32)
    M = ms.max()
    if not np.isfinite(M):
        return f32(np.nan)
    live = np.isfinite(ms)
    if fault == "norescale":
        S = ss[live].sum(dtype=f32)
    else:
        S = (ss[live] * np.exp(ms[live] - M, dtype=f32)).sum(dtype=f32)
    return f32(x[tok] - f32(M + np.log(S, dtype=f32)))


def crafted_rows(V, seed=0):
    """Rows (name, x [ldv] f32 with junk in the pad columns, dead [V], tok, argmax) on which every planted fault is far outside the
    bound: logits spread over +-60, a dominant last id next to the pad columns, a row whose processors mask everything but one
    token, a forced token far from the arg-max."""
    rng = np.random.default_rng(seed)
    ldv = (V + 3) & ~3
    assert ldv > V, "the pad-column fault needs a vocabulary that is no multiple of 4"
    out = []

    def row(name, body, dead, tok):
        x = np.empty(ldv, np.float32)
        x[:V] = body
        x[V:] = 75.0                                   # what must never count
        out.append((name, x, dead, int(tok), int(np.argmax(body))))

    none = np.zeros(V, bool)
    body = rng.uniform(-60, 60, V).astype(np.float32)
    row("spread", body, rng.random(V) < 0.3, int(rng.integers(0, V)))
    body = (rng.standard_normal(V) * 2).astype(np.float32); body[V - 1] = 30.0
    dead = none.copy(); dead[V - 1] = True
    row("dominant_last_id_masked", body, dead, V - 1)
    body = (rng.standard_normal(V) * 3).astype(np.float32)
    dead = np.ones(V, bool); dead[V // 2] = False
    row("all_but_one_masked", body, dead, V // 2)
    body = (rng.standard_normal(V) * 3).astype(np.float32); body[5] = 25.0
    dead = rng.random(V) < 0.5; dead[5] = True
    row("forced_far_from_argmax", body, dead, V - 7)
    body = rng.uniform(-60, 60, V).astype(np.float32); body[::NS] += 20
    row("spread_every_slice_has_mass", body, rng.random(V) < 0.5, 3)
    return out
