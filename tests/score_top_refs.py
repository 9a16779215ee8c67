"""References for the alternatives of teacher-forced positions (cw_set_score_top_logprobs; score.hip TOPK forms).

* ``reference_topk``: float64.  The candidates of a row are its columns n < V with z[n] > -inf (a NaN is none), ordered by value
  descending, id ascending on an exact tie; rank j holds that id and z - lse64, lse64 the float64 logsumexp of the row's V
  columns.  z is the kernel's own f32 logits (the head's logits-storing form runs the same MFMA sequence; the row kernel is
  handed them), so the ids admit no leeway: both sides compare the same f32 numbers.
* ``check_topk``: the comparator of the GPU tests.  Ids exact, -1 / NaN at the ranks no candidate fills and at ranks >= k, rows
  behind M untouched, values within
      (sum_terms + C) u + 4 u (1 + |lse| + |z|),   u = 2^-24,
  the sum-and-subtraction part of the bound tests/test_gpu_score.py derives (the logit part is absent: z is exact).
  Head: sum_terms = V / 16, C = 400 (that file's derivation: V / 16 + 1 terms per lane, 8 shuffle merges, <= 256 partials, expf
  2 ulp, arguments |arg| <= 100 rounded once).  Row kernel (``ROWS_C``): a thread adds at most V / 256 + 1 terms, 6 shuffle steps
  and 3 adds merge them (9 u), every term one expf (2 ulp) of an argument rounded once (100 u for |arg| <= 100): relative
  (V / 256 + 112) u of the sum, i.e. absolute in its logarithm; logf's 2 ulp, the add of the maximum and the final subtraction
  are the 4 u (1 + |lse| + |z|) term.  So sum_terms = V / 256, C = 112.
* ``model_topk``: a float32 numpy model of the head's selection -- per vocabulary split a sorted list of 8 pairs with a
  threshold register, filled tile group by tile group, written out padded with the identity, merged over the splits -- in which
  faults can be planted.  ``order="tile"`` is the kernel's order of service (tile by tile, lanes ascending: a row meets its ids
  in ascending order); ``order="lane"`` serves a lane's four columns of a tile group before the next lane's, the order in
  which a threshold compared by value alone loses a tie.  tests/test_score_top_refs.py proves that the comparator rejects every
  planted fault and passes the clean model in both orders.
"""
import numpy as np

U = 2.0 ** -24
K_MAX = 8
HEAD_C, ROWS_C = 400.0, 112.0
SENT_ID, SENT_LP = -7, np.float32(7.0)          # what the callers pre-fill output buffers with
IMAX = 0x7fffffff
FAULTS = ("value_only", "tie_high", "padding_admitted", "split_not_padded", "merge_short", "row_past_m")


def lse64(z, V):
    """float64 logsumexp over columns 0 .. V-1 of every row (-inf for a row without a finite column, NaN with a NaN)."""
    z = np.asarray(z, np.float64)[:, :V]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = np.max(np.where(np.isnan(z), -np.inf, z), axis=1)
        safe = np.where(np.isfinite(mx), mx, 0.0)
        s = np.exp(z - safe[:, None]).sum(axis=1)
        out = safe + np.log(s)
    return np.where(np.isfinite(mx) | np.isnan(s), out, -np.inf)


def reference_topk(z, V, k):
    """-> ids int64 [M][K_MAX] (-1 where no candidate / rank >= k), lp float64 [M][K_MAX] (NaN likewise), lse64 [M]."""
    z = np.asarray(z)
    M = z.shape[0]
    ids = np.full((M, K_MAX), -1, np.int64)
    lp = np.full((M, K_MAX), np.nan)
    lse = lse64(z, V)
    for m in range(M):
        row = z[m, :V].astype(np.float64)
        cand = np.flatnonzero(row > -np.inf)                     # (a NaN compares false)
        order = cand[np.lexsort((cand, -row[cand]))][:k]
        ids[m, :len(order)] = order
        lp[m, :len(order)] = row[order] - lse[m]
    return ids, lp, lse


def check_topk(alt_id, alt_lp, z, V, k, sum_terms, C, M=None):
    """-> (problems: list of str, empty when everything holds; worst: the largest |error| / bound over the finite values)."""
    alt_id, alt_lp, z = np.asarray(alt_id), np.asarray(alt_lp), np.asarray(z)
    M = z.shape[0] if M is None else M
    problems = []
    if alt_id.shape[0] > M and not (np.all(alt_id[M:] == SENT_ID) and np.all(alt_lp[M:] == SENT_LP)):
        problems.append("a row behind M was written")
    ids, lp, lse = reference_topk(z[:M], V, k)
    worst = 0.0
    for m in range(M):
        if not np.array_equal(alt_id[m], ids[m]):
            problems.append(f"row {m}: ids {alt_id[m].tolist()} != {ids[m].tolist()}")
            continue
        n = int((ids[m] >= 0).sum())
        if not np.all(np.isnan(alt_lp[m, n:])):
            problems.append(f"row {m}: ranks {n} .. hold {alt_lp[m, n:].tolist()}, not NaN")
        if n == 0 or not np.isfinite(lse[m]):
            continue                                             # (a NaN in the row: the normaliser is NaN, as token_logprob's)
        zz = z[m, ids[m, :n]].astype(np.float64)
        bound = (sum_terms + C) * U + 4 * U * (1 + abs(lse[m]) + np.abs(zz))
        err = np.abs(alt_lp[m, :n].astype(np.float64) - lp[m, :n])
        if not np.all(err <= bound):                             # (a NaN value fails here)
            problems.append(f"row {m}: |error| {err.tolist()} above {bound.tolist()}")
        else:
            worst = max(worst, float((err / bound).max()))
    return problems, worst


def _better(v, i, bv, bi, high=False):
    return v > bv or (v == bv and (i > bi if high else i < bi))


def model_topk(z, V, k, tiles_per_split, fault=None, order="tile", guard=2):
    """z f32 [M][16 * tiles] -- the columns >= V are the padding columns of the last tile, which the packed image fills from its
    last row.  -> alt_id int32 / alt_lp float32 [M + guard][K_MAX], pre-filled with the sentinels behind row M - 1."""
    assert fault is None or fault in FAULTS
    z = np.asarray(z, np.float32)
    M, ncol = z.shape
    NT = ncol // 16
    ns = -(-NT // tiles_per_split)
    high = fault == "tie_high"
    out_id = np.full((M + guard, K_MAX), SENT_ID, np.int32)
    out_lp = np.full((M + guard, K_MAX), SENT_LP, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        lse = lse64(z, V).astype(np.float32)
    for m in range(M + 1 if fault == "row_past_m" else M):
        zr = z[min(m, M - 1)]
        pairs = []
        for s in range(ns):
            # the split's list: what the kernel initialises to the identity; "split_not_padded": whatever the memory held (zeros)
            lst = [(np.float32(0.0), 0) if fault == "split_not_padded" else (np.float32(-np.inf), IMAX) for _ in range(K_MAX)]
            t_end = min(NT, (s + 1) * tiles_per_split)

            def serve(offers):                                   # one lane after the other, each against the list itself
                for v, n in offers:
                    if not _better(v, n, lst[k - 1][0], lst[k - 1][1], high):
                        continue
                    p = k - 1
                    while p > 0 and _better(v, n, lst[p - 1][0], lst[p - 1][1], high):
                        lst[p] = lst[p - 1]
                        p -= 1
                    lst[p] = (v, n)

            def offers_of(cols):                                 # against the threshold register: the list's k-th pair
                kth = lst[k - 1]
                got = []
                for n in cols:
                    if n >= V and fault != "padding_admitted":
                        continue
                    v = zr[n]
                    if not v > -np.inf:
                        continue
                    if (v > kth[0]) if fault == "value_only" else _better(v, n, kth[0], kth[1], high):
                        got.append((v, n))
                return got

            for t0 in range(s * tiles_per_split, t_end, 4):
                tiles = [t for t in range(t0, t0 + 4) if t < t_end]
                if order == "tile":
                    for t in tiles:
                        serve(offers_of([t * 16 + l for l in range(16)]))
                else:
                    for l in range(16):
                        serve(offers_of([t * 16 + l for t in tiles]))
            pairs += lst[:k - 1] if fault == "merge_short" else lst
        cand = [(v, n) for v, n in pairs if v > -np.inf]
        cand.sort(key=lambda p: (-float(p[0]), -p[1] if high else p[1]))
        out_id[m], out_lp[m] = -1, np.nan
        for j, (v, n) in enumerate(cand[:k]):
            out_id[m, j] = n
            out_lp[m, j] = np.float32(v) - lse[min(m, M - 1)]
    return out_id, out_lp
