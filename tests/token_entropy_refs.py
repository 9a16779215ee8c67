"""Float64 reference and comparator for the token entropy of the sampler kernels and of the scoring head (cw_set_token_entropy /
cw_set_score_entropy; csrc/elementwise.hip, csrc/score.hip), and a float32 numpy model of the kernels' reduction in which faults
can be planted (tests/test_token_entropy_refs.py proves the comparator rejects them).

Definition.  For raw f32 logits x[0 .. V-1] (pad columns behind V never count), F = {v < V : x[v] > -inf}, m = max_F x,
    S = sum_F exp(x - m),   Zc = sum_F exp(x - m) (x - m) <= 0,   H = log S - Zc / S      (nats, 0 <= H <= log |F|);
H is NaN when F is empty or any x[v], v < V, is NaN or +inf.  Partials (m_i, S_i, Zc_i) merge as
    M = max m_i,   S = sum S_i e^(m_i - M),   Zc = sum (Zc_i + S_i (m_i - M)) e^(m_i - M).

What the sampler kernels do with a row is what tests/token_logprob_refs.py describes for S (16 slices, 256 threads, n_it groups of
four per thread, block merge, 16-slice merge), with Zc kept beside S: per element one more product e * d, per move of a centre
(in the thread: n_it times; to the slice maximum; to the row maximum) one product S_i * delta, one addition and the product with
the expf the S rescale already pays; the additions of the partial sums are those of S.

Bound (first order, u = 2^-24, every term a worst-case sum, nothing fitted to what the kernel returns).  All terms of Zc have one
sign, so a relative error of a partial sum is a relative error of |Zc| at most.
  eS, the relative error of S = the absolute error of log S: the bound of token_logprob_refs.py,
      u * [ops + sum_v p_v (m - x_v)],  ops = 4 n + n (1 + 2 E) + 2 E + (1 + 2 E) + 6 + 4 + (1 + 2 E) + merge_adds
  eZ, the absolute error of Zc in units of S (i.e. of Zc / S before the division's own rounding):
      u * [(ops + 1 + 2 (n + 2) + 1) * |Zc| / S      the chain of S, the product e * d, two more operations per move of a centre,
                                                     and the rounded differences as the factor d (their sizes add up to m - x_v)
          + sum_v p_v (m - x_v)^2 ]                  the rounded differences as the exponents' arguments, weighted by |d|
  H = log S - Zc / S:   eS + 2 L u |log S|  +  eZ + (eS + u) |Zc| / S  +  u (|log S| + |Zc| / S)
E and L are the errors of expf / logf in ulp (1 ulp = 2 u relative): E = L = 3, as in token_logprob_refs.py.  The scoring head
walks its columns in another order (per lane, 16-lane merge, split merge): `head_depth` gives its n and merge_adds.

first_order(x, V, delta): what an error of at most delta in every logit can move H by, dH/dx_v = -p_v (log p_v + H):
    delta * sum_v p_v |log p_v + H|  +  delta^2 * (1 + sum_v p_v (log p_v + H)^2)
(the second term bounds the curvature: the Hessian's entries are products of p's with (log p + H) and 1, for delta << 1)."""
from __future__ import annotations

import numpy as np

from tests.token_logprob_refs import EXPF_ULP, LOGF_ULP, NS, THREADS, U, n_iter


def _finite_set(x, V):
    x64 = np.asarray(x[:V], np.float64)
    bad = bool(np.isnan(x64).any() or np.isposinf(x64).any())
    return x64, bad, np.isfinite(x64)


def reference(x, V):
    """H in float64 for one row; x may carry pad columns behind V."""
    x64, bad, fin = _finite_set(x, V)
    if bad or not fin.any():
        return float("nan")
    d = x64[fin] - x64[fin].max()
    e = np.exp(d)
    S = e.sum()
    return float(np.log(S) - (e * d).sum() / S)


def merge(parts):
    """The merge rule on (m, S, Zc) triples, evaluated as written (float64 in, float64 out)."""
    live = [(m, S, Z) for m, S, Z in parts if m > -np.inf]
    if not live:
        return -np.inf, 0.0, 0.0
    M = max(m for m, _, _ in live)
    S = sum(s * np.exp(m - M) for m, s, _ in live)
    Z = sum((z + s * (m - M)) * np.exp(m - M) for m, s, z in live)
    return M, S, Z


def direct(x):
    """(m, S, Zc) of a float64 vector, -inf entries ignored."""
    x = np.asarray(x, np.float64)
    x = x[x > -np.inf]
    if not len(x):
        return -np.inf, 0.0, 0.0
    m = x.max()
    d = x - m
    e = np.exp(d)
    return float(m), float(e.sum()), float((e * d).sum())


def sampler_depth(V):
    return n_iter(V), NS


def head_depth(V, n_split):
    """The scoring head: a lane meets ceil(tiles of its split / 4) groups of four columns; 4 merge steps over the 16 lanes of a row
    count as 4 more moves of a centre with one addition each; then n_split partials are added."""
    tiles = (V + 15) // 16
    per = (tiles + n_split - 1) // n_split
    return (per + 3) // 4 + 4, n_split + 4


def bound(x, V, depth=None):
    x64, bad, fin = _finite_set(x, V)
    assert not bad and fin.any()
    n, merge_adds = depth if depth is not None else sampler_depth(V)
    m = x64[fin].max()
    d = x64[fin] - m
    p = np.exp(d)
    S = p.sum()
    Z = abs(float((p * d).sum()))
    E = EXPF_ULP
    ops = 4 * n + n * (1 + 2 * E) + 2 * E + (1 + 2 * E) + 6 + 4 + (1 + 2 * E) + merge_adds
    eS = U * (ops + float((p * -d).sum() / S))
    eZ = U * ((ops + 1 + 2 * (n + 2) + 1) * Z / S + float((p * d * d).sum() / S))
    lS = abs(float(np.log(S)))
    return eS + 2 * LOGF_ULP * U * lS + eZ + (eS + U) * Z / S + U * (lS + Z / S)


def first_order(x, V, delta):
    x64, bad, fin = _finite_set(x, V)
    assert not bad and fin.any()
    d = x64[fin] - x64[fin].max()
    lp = d - np.log(np.exp(d).sum())
    p = np.exp(lp)
    H = -(p * lp).sum()
    return float(delta * (p * np.abs(lp + H)).sum() + delta * delta * (1.0 + (p * (lp + H) ** 2).sum()))


def compare(got, x, V, depth=None, extra=0.0):
    """-> (ok, |got - ref|, bound) for one row.  Where the definition gives NaN the kernel must give NaN."""
    ref = reference(x, V)
    got = float(got)
    if np.isnan(ref):
        return bool(np.isnan(got)), 0.0, 0.0
    b = bound(x, V, depth) + extra
    if not np.isfinite(got):
        return False, float("inf"), b
    return abs(got - ref) <= b, abs(got - ref), b


def check_rows(got, logits, V, what="", depth=None, extra=None):
    """Asserts compare() for every row and 0 <= H <= log |F| (up to the bound); prints the worst |error| / bound ratio first."""
    worst, bad = 0.0, []
    for b in range(len(got)):
        ex = 0.0 if extra is None else float(extra[b])
        ok, err, bd = compare(got[b], logits[b], V, depth, ex)
        if bd > 0:
            worst = max(worst, err / bd)
            nF = int(np.isfinite(np.asarray(logits[b][:V], np.float64)).sum())
            ok = ok and 0.0 <= float(got[b]) <= np.log(nF) + bd
        if not ok:
            bad.append((b, float(got[b]), reference(logits[b], V), err, bd))
    print(f"{what}: {len(got)} rows, worst |err| / bound = {worst:.3f}")
    assert not bad, (what, bad[:3])


# ---- float32 model of the sampler kernels' reduction, with faults to plant -------------------------------------------------
def kernel_model(x, V, fault=None):
    """x: f32 row of ldv columns (pad columns behind V hold whatever the logits GEMV left there).  fault: None, "pad" (pad columns
    counted), "noshift" (the S_i (m_i - M) term dropped when the slices move to the row maximum)."""
    f32 = np.float32
    x = np.asarray(x, f32)
    ldv = len(x)
    assert ldv % 4 == 0 and ldv >= V
    lim = ldv if fault == "pad" else V
    if np.isnan(x[:lim]).any() or np.isposinf(x[:lim]).any():
        return f32(np.nan)
    per4 = ((ldv >> 2) + NS - 1) // NS
    parts = []
    for sl in range(NS):
        lo, hi = sl * per4 * 4, min(ldv, (sl + 1) * per4 * 4)
        # a thread: groups lo/4 + tid, + 256, ...; its online triple
        thr = []
        for tid in range(min(THREADS, max(0, (hi - lo + 3) // 4))):
            m, s, z = f32(-np.inf), f32(0), f32(0)
            for g in range(lo // 4 + tid, hi // 4, THREADS):
                xs = [x[v] for v in range(4 * g, 4 * g + 4) if v < lim]
                gm = max(xs, default=f32(-np.inf))
                if gm > m:
                    if m > -np.inf:
                        d = f32(m - gm); e = np.exp(d, dtype=f32)
                        z = f32(f32(z + f32(s * d)) * e); s = f32(s * e)
                    m = gm
                if m > -np.inf:
                    for v in xs:
                        d = f32(v - m); e = np.exp(d, dtype=f32)
                        s = f32(s + e)
                        if d > -np.inf:
                            z = f32(z + f32(e * d))
            thr.append((m, s, z))
        ms = max((t[0] for t in thr), default=f32(-np.inf))
        S, Z = f32(0), f32(0)
        for m, s, z in thr:
            if m > -np.inf:
                d = f32(m - ms); e = np.exp(d, dtype=f32)
                S = f32(S + f32(s * e)); Z = f32(Z + f32(f32(z + f32(s * d)) * e))
        parts.append((ms, S, Z))
    M = max(p[0] for p in parts)
    if not np.isfinite(M):
        return f32(np.nan)
    S, Z = f32(0), f32(0)
    for m, s, z in parts:
        if m > -np.inf:
            d = f32(m - M); e = np.exp(d, dtype=f32)
            S = f32(S + f32(s * e))
            shift = f32(0) if fault == "noshift" else f32(s * d)
            Z = f32(Z + f32(f32(z + shift) * e))
    H = f32(np.log(S, dtype=f32) - f32(Z / S))
    return f32(0) if H < 0 else H


def crafted_rows(V, seed=0):
    """Rows (name, x [ldv] f32 with +75 in the pad columns) on which every planted fault is far outside the bound: logits spread
    over +-60, a dominant last id next to the pad columns, mass in every slice at different heights."""
    rng = np.random.default_rng(seed)
    ldv = (V + 3) & ~3
    assert ldv > V, "the pad-column fault needs a vocabulary that is no multiple of 4"
    out = []

    def row(name, body):
        x = np.empty(ldv, np.float32)
        x[:V] = body
        x[V:] = 75.0                                   # what must never count
        out.append((name, x))

    row("spread", rng.uniform(-60, 60, V).astype(np.float32))
    body = (rng.standard_normal(V) * 2).astype(np.float32); body[V - 1] = 30.0
    row("dominant_last_id", body)
    body = rng.uniform(-3, 3, V).astype(np.float32)
    per = (ldv // 4 + NS - 1) // NS * 4
    for sl in range(NS):
        body[sl * per:(sl + 1) * per] += 4.0 * (sl % 5)            # every slice has mass, the slice maxima differ by up to 16
    row("slices_at_different_heights", body)
    body = (rng.standard_normal(V) * 3).astype(np.float32); body[rng.random(V) < 0.4] = -np.inf
    row("many_minus_inf", body)
    return out
