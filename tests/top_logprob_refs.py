"""Float64 reference and comparator for the alternatives of the sampler kernels (cw_set_top_logprobs; sample_partial_kernel /
sample_kernel in csrc/elementwise.hip), a float32 numpy model of the kernels' two-stage selection in which faults can be planted
(tests/test_top_logprob_refs.py proves the comparator rejects them), and the crafted rows both the CPU and the GPU tests use.

Definition.  Candidates of a row are the columns v < V with x_v > -inf on the raw f32 logits (masked tokens count, the pad columns
V .. ldv-1 and NaN never do), ordered by value descending, token id ascending on an exact tie.  top_id[j] is the j-th candidate,
top_logprob[j] = x_v - logsumexp(x[0 .. V-1]) with the normaliser of tests/token_logprob_refs.py; ranks at or beyond the number
of candidates hold -1 / NaN.

Ids.  Selection compares f32 values that are never rounded, so the ids equal the float64 reference exactly: no leeway.
Values.  The arithmetic is that of the token log-probability (the same M + logf(S), one subtraction), so the bound of
token_logprob_refs.bound holds with the alternative's id in place of the written token's.

What the kernels do: stage 1 cuts the row into 16 slices (token_logprob_refs.kernel_model has the geometry) and emits each
slice's k best, padded with (-inf, INT_MAX); stage 2 takes the k best of the 16 x k pairs."""
from __future__ import annotations

import numpy as np

from tests import token_logprob_refs as R

K_MAX = 8
NONE_ID = 0x7fffffff
FAULTS = ("pad", "tie_high", "masked", "repeat", "best_only", "processed_sum")


def reference_topk(x, V, k):
    """(ids int64 [k], logprobs float64 [k]) of one row in float64; -1 / NaN behind the last candidate.  x may carry pad columns."""
    x64 = np.asarray(x[:V], np.float64)
    cand = np.flatnonzero(x64 > -np.inf)                       # false for NaN
    if len(cand) > 4 * k:                                      # only what reaches the k-th largest value can be listed
        cand = cand[x64[cand] >= np.partition(x64[cand], -k)[-k]]
    order = cand[np.lexsort((cand, -x64[cand]))][:k]
    ids = np.full(k, -1, np.int64)
    lps = np.full(k, np.nan, np.float64)
    ids[:len(order)] = order
    if len(order):
        lps[:len(order)] = x64[order] - R.reference(x, int(order[0]), V)[1]
    return ids, lps


def compare_topk(ids, lps, x, V, k):
    """-> (ok, worst |err| / bound, why).  ids exact; every listed value through token_logprob_refs.compare with the alternative's
    id as the token; -1 / NaN exactly behind the last candidate."""
    ids = np.asarray(ids).reshape(-1)
    lps = np.asarray(lps).reshape(-1)
    if len(ids) != k or len(lps) != k:
        return False, 0.0, f"{len(ids)} ids / {len(lps)} values for k = {k}"
    want, _ = reference_topk(x, V, k)
    if ids.tolist() != want.tolist():
        return False, 0.0, f"ids {ids.tolist()} != {want.tolist()}"
    worst = 0.0
    for j in range(k):
        if want[j] < 0:
            if not np.isnan(lps[j]):
                return False, worst, f"rank {j}: value {lps[j]} behind the last candidate"
            continue
        ok, err, bd = R.compare(lps[j], x, int(want[j]), V)
        if bd > 0:
            worst = max(worst, err / bd)
        if not ok:
            return False, worst, f"rank {j} (id {want[j]}): {lps[j]} against {R.reference(x, int(want[j]), V)[0]}, bound {bd}"
    return True, worst, ""


def check_topk_rows(ids, lps, logits, V, k, what=""):
    """Asserts compare_topk for every row; prints the worst |error| / bound ratio before it asserts."""
    worst, bad = 0.0, []
    for b in range(len(logits)):
        ok, w, why = compare_topk(ids[b], lps[b], logits[b], V, k)
        worst = max(worst, w)
        if not ok:
            bad.append((b, why))
    print(f"{what}: {len(logits)} rows x {k}, worst |err| / bound = {worst:.3f}")
    assert not bad, (what, bad[:3])


# ---- float32 model of the kernels' two-stage selection, with faults to plant -------------------------------------------------
def kernel_model_topk(x, V, k, dead=None, fault=None):
    """x: f32 row of ldv columns (whatever the logits GEMV left in the pad columns behind V).  dead: bool [V], the tokens the
    processors mask (they count all the same).  fault: None or one of FAULTS --
      pad            pad columns counted as candidates
      tie_high       an exact tie resolved to the higher id
      masked         masked tokens left out of the candidates
      repeat         a slice with fewer than k candidates repeats its winner instead of padding
      best_only      the merge takes only each slice's best
      processed_sum  the value normalised with the processed sum (masked tokens left out) instead of the raw one
    -> (ids int32 [k], logprobs f32 [k])."""
    assert fault is None or fault in FAULTS
    f32 = np.float32
    x = np.asarray(x, f32)
    ldv = len(x)
    assert ldv % 4 == 0 and ldv >= V
    per4 = ((ldv >> 2) + R.NS - 1) // R.NS
    sign = -1 if fault == "tie_high" else 1

    def best(pairs):
        return sorted(pairs, key=lambda p: (-p[0], sign * p[1]))

    dead_all = np.zeros(ldv, bool)
    if dead is not None:
        dead_all[:V] = dead
    recs = []
    for sl in range(R.NS):
        lo, hi = sl * per4 * 4, min(ldv, (sl + 1) * per4 * 4)
        idx = np.arange(lo, hi)
        keep = (idx < (ldv if fault == "pad" else V)) & (x[idx] > -np.inf)
        if fault == "masked":
            keep &= ~dead_all[idx]
        c = best([(float(x[i]), int(i)) for i in idx[keep]])[:k]
        fill = c[0] if (fault == "repeat" and c) else (-np.inf, NONE_ID)
        c = c + [fill] * (k - len(c))
        recs += c[:1] if fault == "best_only" else c
    merged = best(recs)[:k]
    merged += [(-np.inf, NONE_ID)] * (k - len(merged))
    ids = np.full(k, -1, np.int32)
    lps = np.full(k, np.nan, f32)
    poisoned = bool(np.isnan(x[:V]).any())             # a NaN logit is no candidate, but the sum it enters is NaN
    for j, (val, i) in enumerate(merged):
        if val > -np.inf:
            ids[j] = i
            if not poisoned:
                lps[j] = R.kernel_model(x, i, V, dead, "masked" if fault == "processed_sum" else None)
    return ids, lps


def geometry(V):
    """(ldv, columns per slice) of the sampler for a vocabulary of V."""
    ldv = (V + 3) & ~3
    return ldv, (((ldv >> 2) + R.NS - 1) // R.NS) * 4


def crafted_rows(V, k, seed=0):
    """[(name, x [ldv] f32 with +75 in the pad columns, dead [V] bool)]: the rows on which a selection can go wrong -- exact ties
    across a slice boundary, a wave boundary (where a slice is wider than a wave's 64 float4 groups) and between two groups of one
    thread (where a thread holds more than one), all winners in one slice (and masked), winners in the last float4 next to the pad
    columns, slices with 0 / 1 / k-1 finite logits, fewer than k finite logits in the whole row, a NaN above everything."""
    rng = np.random.default_rng(seed)
    ldv, per = geometry(V)
    assert ldv > V, "the pad-column case needs a vocabulary that is no multiple of 4"
    out = []

    def noise(scale=3.0):
        return (rng.standard_normal(V) * scale).astype(np.float32)

    def row(name, body, dead=None):
        x = np.empty(ldv, np.float32)
        x[:V] = body
        x[V:] = 75.0                                   # what must never count
        out.append((name, x, np.zeros(V, bool) if dead is None else dead))

    body = noise(); body[[per - 1, per, 2 * per]] = 40.0; body[per + 5] = 39.0
    row("tie_across_slice_boundary", body)
    body = noise()
    if per > 64 * 4:                                   # lanes 63 / 64 of slice 5: two waves
        body[[5 * per + 63 * 4 + 3, 5 * per + 64 * 4]] = 41.0
    else:                                              # one wave holds the slice: neighbouring lanes
        body[[5 * per + 3, 5 * per + 4]] = 41.0
    body[5 * per + 1] = 41.0
    row("tie_across_wave_or_lane_boundary", body)
    body = noise()
    if per > 256 * 4:                                  # thread 9 of slice 2 holds groups 9 and 9 + 256
        body[[2 * per + (9 + 256) * 4 + 2, 2 * per + 9 * 4 + 2, 2 * per + (9 + 512) * 4]] = 42.0
    body[[7 * per + 8, 7 * per + 9, 7 * per + 10, 7 * per + 11]] = 42.0      # one float4 of one thread
    row("tie_inside_one_thread", body)
    body = noise()
    hot = 3 * per + rng.choice(per, K_MAX + 2, replace=False)
    body[hot] = 50.0 + np.arange(len(hot), dtype=np.float32) // 2          # pairs of ties among them
    dead = np.zeros(V, bool); dead[hot[::2]] = True
    row("all_winners_in_one_slice_half_masked", body, dead)
    body = noise(); body[V - 1] = 30.0; body[V - 2] = 31.0; body[V - 3] = 30.0
    row("winners_in_the_last_float4", body)
    body = np.full(V, -np.inf, np.float32)                                 # slice 0: nothing
    body[per + 17] = 60.0                                                  # slice 1: one
    body[2 * per + rng.choice(per, max(k - 1, 0), replace=False)] = 20.0 + np.arange(max(k - 1, 0), dtype=np.float32)
    body[3 * per:4 * per] = noise()[3 * per:4 * per]                       # slice 3: plenty
    dead = np.zeros(V, bool); dead[per + 17] = True
    row("slices_with_0_1_and_k-1_finite", body, dead)
    body = np.full(V, -np.inf, np.float32)
    n = max(k - 2, 0)
    body[rng.choice(V, n, replace=False)] = rng.uniform(-5, 5, n).astype(np.float32)
    row("fewer_than_k_finite", body)
    body = noise(); body[per + 2] = np.nan; body[3] = 12.0
    row("nan_logit", body)
    return out


# ---- the transformers fixture (tests/golden/gen_golden_top_logprobs.py writes it, tests/test_gpu_top_logprobs.py reads it) -----
GOLD_K = 5
GOLD_GAP = 8e-3                  # 2 * BOUND["float32"] (tests/test_gpu_score_vs_transformers.py)
GOLD_MAX_LEFT_OUT = 0.10


def checked_pairs(top_lp, k=GOLD_K, gap=GOLD_GAP):
    """bool [n][k]: rank j of a position is held to the golden where its golden gaps to ranks j - 1 and j + 1 both exceed ``gap``
    (top_lp [n][> k]: one more rank than is tested); a smaller gap may legitimately swap two ids."""
    lp = np.asarray(top_lp, np.float64)
    assert lp.shape[1] > k
    d = lp[:, :-1] - lp[:, 1:]                       # d[:, j] = gap between ranks j and j + 1
    ok = d[:, :k] > gap
    ok[:, 1:] &= d[:, :k - 1] > gap
    return ok
