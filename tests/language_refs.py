"""Float64 reference and comparator for the language-identification kernel (cw_detect_language / cw_test_language_probs;
language_probs_kernel in csrc/langid.hip), and a float32 numpy model of the kernel in which faults can be planted
(tests/test_language_refs.py proves the comparator rejects them).

Definition, for one row x of f32 logits (V valid columns, pad columns behind them) and a table of n_lang candidate token ids:
  l_k   = x[ids[k]], a NaN counting as -inf (never a candidate)
  best  = the id with the largest l_k, the lowest id on an exact tie; no l_k above -inf: the lowest id of the table
  prob  = softmax over the candidates ONLY, in table order (Whisper's detect_language masks every other column): a candidate
          at -inf has exactly 0; no l_k above -inf: all NaN
  ns    = softmax(x[0 .. V-1])[ns_tok] over the whole vocabulary; the pad columns never count

What the kernel does with a row (one block of 256 threads, four waves of 64):
  language part   thread k holds l_k; the maximum m is exact (comparisons only).  e_k = expf(l_k - m): one subtraction, one expf.
                  S = sum of the e_k: a 6-step butterfly inside each wave, then (w0 + w1) + (w2 + w3).  prob_k = e_k / S.
  no-speech part  thread t walks the groups t, t + 256, ... of four columns (n_it = ceil(ldv / 4 / 256) of them), keeping a
                  running maximum m_t and s_t = sum expf(x - m_t): per group one rescale s *= expf(m_old - m_new), three
                  additions inside the group and one onto s.  The block maximum M is exact; every thread rescales once,
                  s_t * expf(m_t - M); the same butterfly and 4-term sum give Z.  ns = expf(x[ns_tok] - M) / Z.

Bounds (first order, u = 2^-24, every term a worst-case sum, nothing fitted to what the kernel returns).  E is the error of expf
in ulp (1 ulp = 2 u relative); the device library implements the accuracy of the OpenCL full profile, which allows exp 3 ulp.
  relative error of prob_k:
      u * [ |l_k - m| + 2 E                      e_k: the rounded difference (relative u of its size, which the exponential
                                                 turns into a relative error of that size), the expf
          + sum_j p_j (|l_j - m| + 2 E)          the same for every term of S, weighted by its share p_j of S
          + 6 + 2                                butterfly, sum over the waves
          + 1 ]                                  the division
  relative error of ns:
      u * [ n_it (4 + 1 + 2 E)                   per group: four additions, the rescale (one multiplication, one expf)
          + 2 E                                  the expf of the term itself
          + (1 + 2 E)                            rescale to the row maximum
          + 6 + 2                                butterfly, sum over the waves
          + sum_v p_v (M - x_v) ]                the exponents' arguments: along element -> thread maximum -> row maximum the
                                                 rounded differences add up to M - x_v; an element weighs p_v = softmax(x)_v in Z
    + u * [ |x_tok - M| + 2 E + 1 ]              numerator and division
  absolute, both: 2 * 2^-126                     a result below the smallest normal f32 may be flushed to zero or rounded to a
                                                 subnormal, by expf and by the division (S >= 1 and Z >= 1: the largest term is 1)
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
EXPF_ULP = 3
TINY = 2.0 * 2.0 ** -126
THREADS = 256
LANG_IDS_MAX = 128

FAULTS = ("pad", "vocab_softmax", "tie_high", "sorted_order", "nan_wins")


def n_iter(V):
    ldv = (V + 3) & ~3
    return ((ldv >> 2) + THREADS - 1) // THREADS


def _cand(x, ids):
    l = np.asarray(x, np.float64)[np.asarray(ids, np.int64)]
    return np.where(np.isnan(l), -np.inf, l)


def reference(x, ids, V, ns_tok):
    """(best, prob [n_lang] float64 in table order, ns float64 or NaN when ns_tok < 0) for one row."""
    ids = np.asarray(ids, np.int64)
    l = _cand(x, ids)
    m = l.max()
    if m == -np.inf:
        best, prob = int(ids.min()), np.full(len(ids), np.nan)
    else:
        best = int(ids[l == m].min())
        with np.errstate(invalid="ignore"):
            e = np.exp(l - m)                      # (+inf - +inf: NaN, as the kernel's f32 arithmetic gives)
        prob = e / e.sum()
    ns = float("nan")
    if ns_tok >= 0:
        x64 = np.asarray(x[:V], np.float64)
        M = x64.max()
        with np.errstate(invalid="ignore"):
            ns = float(np.exp(x64[ns_tok] - M) / np.exp(x64 - M).sum())
    return best, prob, ns


def prob_bound(x, ids):
    """Absolute bound per candidate (zeros where the definition gives an exact value)."""
    l = _cand(x, ids)
    m = l.max()
    fin = np.isfinite(l)
    p = np.zeros(len(l)); p[fin] = np.exp(l[fin] - m); p /= p.sum()
    E = EXPF_ULP
    common = float((p[fin] * ((m - l[fin]) + 2 * E)).sum()) + 6 + 2 + 1
    out = np.zeros(len(l))
    out[fin] = p[fin] * U * ((m - l[fin]) + 2 * E + common) + TINY
    return out


def sum_bound(n):
    """Bound on |sum_k prob_k - 1| for n candidates when the logits are not at hand: with d_k = m - l_k and p_k = exp(-d_k) / S,
    S >= 1, every p_k d_k is at most 1 / e, so sum_k p_k (d_k + 2 E + sum_j p_j (d_j + 2 E) + 9) <= 2 n / e + 4 E + 9."""
    return U * (2.0 * n / np.e + 4 * EXPF_ULP + 9) + n * TINY


def ns_bound(x, V, ns_tok):
    x64 = np.asarray(x[:V], np.float64)
    M = x64.max()
    fin = np.isfinite(x64)
    p = np.zeros(V); p[fin] = np.exp(x64[fin] - M)
    Z = p.sum()
    E = EXPF_ULP
    n = n_iter(V)
    arg = float((p[fin] * (M - x64[fin])).sum() / Z)
    rel = U * (n * (4 + 1 + 2 * E) + 2 * E + (1 + 2 * E) + 6 + 2 + arg) + U * (abs(x64[ns_tok] - M) + 2 * E + 1)
    return float(p[ns_tok] / Z) * rel + TINY


def compare(best, prob, ns, x, ids, V, ns_tok):
    """-> (ok, worst |error| / bound, reasons) for one row.  best must be exact; where the definition gives exactly 0 (a candidate
    at -inf) or nothing (NaN) the kernel's f32 arithmetic must give the same."""
    rb, rp, rn = reference(x, ids, V, ns_tok)
    why, worst = [], 0.0
    if int(best) != rb:
        why.append(f"best {int(best)} != {rb}")
    prob = np.asarray(prob, np.float64)
    if np.isnan(rp).any():
        if not np.isnan(prob).all():
            why.append("prob must be all NaN")
    else:
        bd = prob_bound(x, ids)
        for k in range(len(rp)):
            if bd[k] == 0.0:
                if prob[k] != 0.0:
                    why.append(f"prob[{k}] = {prob[k]!r} must be exactly 0")
                continue
            if not np.isfinite(prob[k]):
                why.append(f"prob[{k}] = {prob[k]!r}"); continue
            err = abs(prob[k] - rp[k])
            worst = max(worst, err / bd[k])
            if err > bd[k]:
                why.append(f"prob[{k}] = {prob[k]!r}, reference {rp[k]!r}, |err| {err:.3e} > bound {bd[k]:.3e}")
    if ns_tok >= 0:
        ns = float(ns)
        if np.isnan(rn):
            if not np.isnan(ns):
                why.append(f"ns = {ns!r} must be NaN")
        elif not np.isfinite(ns):
            why.append(f"ns = {ns!r}, reference {rn!r}")
        else:
            bd, err = ns_bound(x, V, ns_tok), abs(ns - rn)
            worst = max(worst, err / bd)
            if err > bd:
                why.append(f"ns = {ns!r}, reference {rn!r}, |err| {err:.3e} > bound {bd:.3e}")
    return not why, worst, why


def check_rows(best, prob, ns, logits, ids, V, ns_tok, what=""):
    """Asserts compare() for every row; prints the worst |error| / bound ratio before it asserts."""
    worst, bad = 0.0, []
    for b in range(len(best)):
        ok, w, why = compare(best[b], prob[b], ns[b] if ns is not None else float("nan"), logits[b], ids, V, ns_tok)
        worst = max(worst, w)
        if not ok:
            bad.append((b, why[:3]))
    print(f"{what}: {len(best)} rows, worst |err| / bound = {worst:.3f}")
    assert not bad, (what, bad[:3])


# ---- float32 model of the kernel, with faults to plant --------------------------------------------------------------------
def _butterfly(v):
    """f32 sum of 64 lanes by the xor butterfly (offsets 32 .. 1): every lane ends with the same bits; lane 0 is returned."""
    v = np.asarray(v, np.float32).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[np.arange(64) ^ o]).astype(np.float32)
    return v[0]


def _block_sum(v):
    v = np.asarray(v, np.float32)
    w = [_butterfly(v[64 * k:64 * k + 64]) for k in range(4)]
    return np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))


def kernel_model(x, ids, V, ns_tok, fault=None):
    """x: f32 row of ldv columns (the pad columns hold whatever lies there).  -> (best, prob [n_lang] f32, ns f32).
    fault: None or one of FAULTS -- "pad" (pad columns counted in Z), "vocab_softmax" (the language softmax normalised over the
    whole vocabulary), "tie_high" (the highest id wins a tie), "sorted_order" (probabilities written in ascending-id order instead
    of table order), "nan_wins" (a NaN candidate wins the arg-max)."""
    assert fault is None or fault in FAULTS
    f32 = np.float32
    x = np.asarray(x, f32)
    ldv = len(x)
    assert ldv % 4 == 0 and ldv >= V
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    assert 1 <= n <= LANG_IDS_MAX
    with np.errstate(invalid="ignore", over="ignore"):
        l = x[ids].copy()
        nan = np.isnan(l)
        l[nan] = -np.inf
        m = l.max()
        if fault == "nan_wins" and nan.any():
            best = int(ids[nan].min())
        elif m == -np.inf:
            best = int(ids.min())
        else:
            tied = ids[l == m]
            best = int(tied.max() if fault == "tie_high" else tied.min())
        e = np.zeros(THREADS, f32)
        e[:n] = np.exp(l - m, dtype=f32)
        S = _block_sum(e)
        # ---- the whole row, as the no-speech part walks it
        nv = ldv if fault == "pad" else V
        n_it = ((ldv >> 2) + THREADS - 1) // THREADS
        xx = np.full(n_it * THREADS * 4, -np.inf, f32)
        xx[:nv] = x[:nv]
        xx = xx.reshape(n_it, THREADS, 4)
        mt = np.full(THREADS, -np.inf, f32)
        st = np.zeros(THREADS, f32)
        for it in range(n_it):
            g = xx[it]
            mn = np.fmax(mt, np.fmax(np.fmax(g[:, 0], g[:, 1]), np.fmax(g[:, 2], g[:, 3])))
            live = mn > -np.inf
            msafe = np.where(live, mn, f32(0))
            ex = np.exp(g - msafe[:, None], dtype=f32)
            add = (((ex[:, 0] + ex[:, 1]).astype(f32) + ex[:, 2]).astype(f32) + ex[:, 3]).astype(f32)
            resc = np.where(mt > -np.inf, st * np.exp(np.where(mt > -np.inf, mt, f32(0)) - msafe, dtype=f32), f32(0)).astype(f32)
            st = np.where(live, (resc + add).astype(f32), st)
            mt = np.where(live, mn, mt)
        M = np.fmax.reduce(mt)
        part = np.where(mt > -np.inf, st * np.exp(np.where(mt > -np.inf, mt, f32(0)) - M, dtype=f32), f32(0)).astype(f32)
        Z = _block_sum(part)
        if fault == "vocab_softmax":
            prob = (np.exp(l - M, dtype=f32) / Z).astype(f32)
        else:
            prob = (e[:n] / S).astype(f32)
        if fault == "sorted_order":
            prob = prob[np.argsort(ids, kind="stable")]
        ns = f32(np.nan) if ns_tok < 0 else f32(np.exp(f32(x[ns_tok] - M), dtype=f32) / Z)
    return best, prob, ns


def crafted_rows(V, ids, ns_tok, seed=0):
    """Rows (name, x [ldv] f32 with +75 in the pad columns) for the table `ids` (distinct, NOT in ascending order when it has more
    than one entry) on which every planted fault lands far outside the bound.  Rows that need two candidates are left out for a
    table of one."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    ldv = (V + 3) & ~3
    assert ldv > V, "the pad-column fault needs a vocabulary that is no multiple of 4"
    assert n == 1 or np.any(np.diff(ids) < 0), "the table-order fault needs a table that is not sorted"
    out = []

    def row(name, body):
        x = np.empty(ldv, np.float32)
        x[:V] = body
        x[V:] = 75.0                                   # what must never count
        out.append((name, x))

    def base(scale=2.0):
        return (rng.standard_normal(V) * scale).astype(np.float32)

    body = base(); body[ids] = np.linspace(-3, 3, n, dtype=np.float32) if n > 1 else 1.0   # ascending along the TABLE
    row("best_is_last_table_entry", body)
    if n > 1:
        body = base(); body[ids] = rng.uniform(-4, 0, n).astype(np.float32)
        body[ids[0]] = 2.5; body[ids[-1]] = 2.5
        row("exact_tie", body)
    body = base(); body[ids] = rng.uniform(-2, 2, n).astype(np.float32)
    for a in (int(ids.max()) + 1, int(ids.min()) - 1):
        if 0 <= a < V and a not in set(ids.tolist()):
            body[a] = 75.0
    row("hot_non_language_neighbour", body)
    body = base(); body[ids] = rng.uniform(-2, 2, n).astype(np.float32)
    if n > 1:
        body[ids[::2]] = -np.inf
    row("minus_inf_candidates", body)
    body = base(); body[ids] = -np.inf
    row("all_candidates_minus_inf", body)
    body = rng.uniform(-60, 60, V).astype(np.float32)
    row("spread", body)
    body = base(); body[V - 1] = 30.0; body[ids] = rng.uniform(-2, 2, n).astype(np.float32)
    if ns_tok >= 0 and ns_tok not in set(ids.tolist()):
        body[ns_tok] = 29.0
    row("dominant_last_column", body)
    if n > 1:
        body = base(); body[ids] = rng.uniform(-2, 2, n).astype(np.float32)
        body[ids[n // 2]] = np.nan
        row("nan_candidate", body)
    return out


def random_rows(V, nb, seed):
    """[nb][V] f32: half of the rows N(0, 3), half spread over +-30."""
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((nb, V)) * 3).astype(np.float32)
    lg[1::2] = rng.uniform(-30, 30, (len(lg[1::2]), V)).astype(np.float32)
    return lg
