"""Float64 reference and comparator for the device half of a beam-search step (beam_topk_partial_kernel + beam_topk_merge_kernel,
the default two-stage form, and beam_topk_kernel, the single-block form, in csrc/elementwise.hip), a float32 numpy model of the
two-stage selection in which faults can be planted (tests/test_beam_refs.py proves the comparator rejects them), and the row tables
both the CPU and the GPU tests use.  No GPU in here.

Definition (float64).  lp = x[:V] - logsumexp(x[:V]) on the raw f32 logits x of a row; oracle.logits.process (pinned to the
transformers processors by tests/test_oracle_vs_golden.py) masks lp; the candidates are the finite entries in (value desc, token
asc) order, the first n_cand are kept and the rest of the list holds (-inf, -1).  The pad columns V .. Vpad-1 never count.  A NaN
logit never counts as a candidate, nor in the processors (it is -inf to them); the f32 sum it enters is NaN in both kernel forms,
so the values of such a row must be NaN (tests/top_logprob_refs.py treats the sampler the same way) while its ids stay exact.  An
all -inf row has no candidate.

Ids.  Selection compares f32 logits that are never rounded, x -> x - lse is monotone and keeps exact ties: the ids equal the
reference exactly, no leeway.  One condition: the row-wide decision "timestamp mass > best text" is taken in f32, so a row whose
oracle.logits.timestamp_mass_margin is finite and closer to zero than MARGIN_FACTOR x the value bound of the row (below, the larger
of the two forms', at the best candidate) is undecidable.  The generators replace such rows (they shift the timestamp logits until
the margin is clear), tests/test_beam_refs.py asserts no table row is undecidable, so the GPU tests leave out nothing.  The one
exception is decided exactly, not by margin: a single allowed finite timestamp equal to the best allowed text token.  Both forms
then compute tsum = expf(0) (* expf(0)) = 1 and compare logf(1) = 0 > 0: false, text stays, as in the oracle.

Values.  First-order worst-case bound in the manner of tests/token_logprob_refs.py: u = 2^-24, expf / logf within E = L = 3 ulp
(1 ulp = 2 u relative), every term a worst-case sum, nothing fitted to what a kernel returns.  A kernel stores
(x - max) - logf(S), S = sum_v exp(x_v - max) over the raw row.
  relative error of S = absolute error of log S, two-stage form (slice geometry: per = ceil(V / 16) columns per slice, 256
  threads, thread i holds columns lo + i + 256 k, k < 13):
      u * [ 13             sequential additions in the thread
          + 2 E            the expf of a term
          + 6 + 4          wave sum (6 DPP steps), the four waves' partials
          + (1 + 2 E)      the slice record rescaled by expf(rmax - gmax): one multiplication, one expf
          + 6 ]            the 16 records added by a wave sum
  single-block form (1024 threads, thread i holds columns i + 1024 k):
      u * [ ceil(V / 1024) sequential additions in the thread
          + 2 E            the expf of a term
          + 6 + 16 ]       block_sum: wave sum, the sixteen waves' partials in sequence
  both forms:
    + u * sum_v p_v (max - x_v)    the exponents' arguments: every difference of two f32 numbers is rounded once (relative u of its
                                   size, which the exponential turns into a relative error of that size); along the chain element ->
                                   slice maximum -> row maximum the sizes add up to max - x_v; an element weighs p_v = softmax(x)_v
    + 2 L u |log S|                logf
    + u (|x - max| + |lp|)         the two subtractions (x - max) - logz, each rounded once
The GPU tests print the worst |err| / bound per test.

Kernel model.  kernel_model() restates the two-stage form in float32 numpy with the kernels' slice geometry and their own copy of
the grammar predicate; FAULTS lists what can be planted in it."""
from __future__ import annotations

import functools
import math

import numpy as np

from crisperwhisper_amd import synthetic as syn
from oracle import logits as OL
from tests import sampler_cases as SC
from tests.token_logprob_refs import EXPF_ULP, LOGF_ULP, U

NS = 16                 # BT_NS: slices per row
THREADS = 256           # threads of a slice block
PER_LANE = 13           # BT_PER_LANE: loads per thread
N_CAND_MAX = 64
MARGIN_FACTOR = 100.0
N_PROMPT = SC.N_PROMPT
MAX_INITIAL = 50
HOT_PAD = 75.0          # what the hook holds in the pad columns during a launch
FORMS = ("two_stage", "single_block")
FAULTS = ("allowed_norm", "pad_norm", "tie_high", "best_only", "text_kept", "ts_norescale", "floor_repeat", "floor_next", "cap",
          "eos_unmasked", "load13", "repeat", "inf_slice")


# ---- geometry ------------------------------------------------------------------------------------------------------------------
class Gram:
    """What the selection knows about a vocabulary: sizes, special ids and the two suppress lists."""

    def __init__(self, v: syn.SynthVocab):
        self.v = v
        self.V = v.size
        self.Vpad = (self.V + 3) & ~3
        self.tb = v.timestamp_begin
        self.eos = v.eos
        self.suppress = sorted(set(v.suppress_tokens()) | {v.notimestamps})
        self.begin_suppress = list(v.begin_suppress_tokens())
        self.per = (self.V + NS - 1) // NS
        self.prompt = [v.sot, v.lang_id("en"), v.transcribe]

    def spec(self, min_new):
        v = self.v
        return OL.ProcessorSpec(eos=v.eos, no_timestamps=v.notimestamps, suppress=v.suppress_tokens(),
                                begin_suppress=v.begin_suppress_tokens(), max_initial_timestamp_index=MAX_INITIAL,
                                min_new_tokens=min_new)

    def slice_of(self, tok):
        return tok // self.per

    def bounds(self, sl):
        return sl * self.per, min(self.V, (sl + 1) * self.per)


@functools.lru_cache(maxsize=None)
def gram(which: str) -> Gram:
    """"tiny": SynthVocab.size columns; "large": the 51 866 columns of large-v3."""
    return Gram(syn.tiny_geometry()[1] if which == "tiny" else syn.large_v3_geometry()[1])


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
class Ref:
    """One row's reference: ids int64 [64] / vals float64 [64] (the first n_cand of them answer any n_cand <= 64: the order is
    total), the constants of the value bound, the timestamp-mass margin and whether the row is decidable."""


def _clean(x, V):
    x64 = np.asarray(x[:V], np.float64)
    nan = np.isnan(x64)
    return np.where(nan, -np.inf, x64), bool(nan.any())


def reference(G: Gram, ids, x, min_new) -> Ref:
    V = G.V
    ids = np.asarray(ids, np.int64)
    xc, has_nan = _clean(x, V)
    r = Ref()
    r.nan = has_nan
    r.ids = np.full(N_CAND_MAX, -1, np.int64)
    r.vals = np.full(N_CAND_MAX, -np.inf, np.float64)
    r.margin = float("nan")
    r.decidable = True
    r.bound_const = {f: 0.0 for f in FORMS}
    r.xmax = float(xc.max())
    r.n = 0
    if not np.isfinite(r.xmax):                                   # all -inf: no log-probabilities, no candidate
        r.x_of = np.zeros(0)
        return r
    p = np.exp(xc - r.xmax)
    S = p.sum()
    lse = r.xmax + math.log(S)
    lp = xc - lse
    spec = G.spec(min_new)
    with np.errstate(invalid="ignore", over="ignore"):
        out = OL.process(spec, ids[None], lp[None].astype(np.float32), N_PROMPT, N_PROMPT)[0]
        pre = OL._masked(spec, ids[None], lp[None].astype(np.float32), N_PROMPT, N_PROMPT)[0]   # the processors before the mass rule
        r.margin = float(OL.timestamp_mass_margin(spec, ids[None], lp[None].astype(np.float32), N_PROMPT, N_PROMPT)[0])
    keep = np.flatnonzero(np.isfinite(out))
    if len(keep) > 4 * N_CAND_MAX:
        keep = keep[lp[keep] >= np.partition(lp[keep], -N_CAND_MAX)[-N_CAND_MAX]]
    order = keep[np.lexsort((keep, -lp[keep]))][:N_CAND_MAX]
    r.n = len(order)
    r.ids[:r.n] = order
    r.vals[:r.n] = lp[order]
    fin = np.isfinite(xc)
    arg = float((p[fin] * (r.xmax - xc[fin])).sum() / S)
    E = EXPF_ULP
    ops = {"two_stage": PER_LANE + 2 * E + 6 + 4 + (1 + 2 * E) + 6,
           "single_block": -(-V // 1024) + 2 * E + 6 + 16}
    for f in FORMS:
        r.bound_const[f] = U * (ops[f] + arg) + 2 * LOGF_ULP * U * abs(math.log(S))
    r.x_of = xc[order]
    # decidable?
    ts_ok = np.flatnonzero(np.isfinite(pre[G.tb:]))
    text_best = pre[:G.tb].max() if G.tb else -np.inf
    exact_tie = len(ts_ok) == 1 and np.isfinite(text_best) and pre[G.tb + ts_ok[0]] == text_best and r.margin == 0.0
    if np.isfinite(r.margin) and not exact_tie:
        top = max(value_bound(r, f, 0) for f in FORMS) if r.n else max(r.bound_const.values())
        r.threshold = MARGIN_FACTOR * top
        r.decidable = abs(r.margin) >= r.threshold
    return r


def value_bound(r: Ref, form: str, j: int) -> float:
    return r.bound_const[form] + U * (abs(r.x_of[j] - r.xmax) + abs(r.vals[j]))


def compare(got_ids, got_vals, r: Ref, n_cand: int, form: str):
    """-> (ok, worst |err| / bound, why) for one row: ids exact, values within the form's bound (NaN where the row holds a NaN),
    (-inf, -1) exactly behind the last candidate."""
    got_ids = np.asarray(got_ids).reshape(-1)
    got_vals = np.asarray(got_vals).reshape(-1)
    if len(got_ids) != n_cand or len(got_vals) != n_cand:
        return False, 0.0, f"{len(got_ids)} ids / {len(got_vals)} values for n_cand = {n_cand}"
    want = r.ids[:n_cand]
    if got_ids.tolist() != want.tolist():
        j = int(np.flatnonzero(got_ids != want)[0])
        return False, 0.0, f"ids differ from rank {j}: {got_ids[j:j + 4].tolist()} != {want[j:j + 4].tolist()}"
    worst = 0.0
    for j in range(n_cand):
        g = float(got_vals[j])
        if want[j] < 0:
            if g != -np.inf:
                return False, worst, f"rank {j}: value {g} behind the last candidate"
            continue
        if r.nan:
            if not math.isnan(g):
                return False, worst, f"rank {j}: {g} in a row whose sum holds a NaN"
            continue
        bd = value_bound(r, form, j)
        if not math.isfinite(g):
            return False, float("inf"), f"rank {j} (id {want[j]}): {g}"
        err = abs(g - r.vals[j])
        worst = max(worst, err / bd)
        if err > bd:
            return False, worst, f"rank {j} (id {want[j]}): {g} against {r.vals[j]}, |err| {err:.3e} > bound {bd:.3e}"
    return True, worst, ""


def check_rows(got_ids, got_vals, refs, n_cand, form, names=None, what=""):
    """Asserts compare() for every row; prints the worst |error| / bound ratio before it asserts.  Returns the ratio."""
    worst, bad = 0.0, []
    for b, r in enumerate(refs):
        ok, w, why = compare(got_ids[b], got_vals[b], r, n_cand, form)
        worst = max(worst, w)
        if not ok:
            bad.append((names[b] if names else b, why))
    print(f"{what}: {len(refs)} rows x {n_cand} ({form}), worst |err| / bound = {worst:.3f}")
    assert not bad, (what, bad[:3])
    return worst


# ---- float32 model of the two-stage selection, with faults to plant --------------------------------------------------------------
def _dead(G: Gram, ids, min_new, fault):
    """The kernels' collapsed predicate (dead() in beam_topk_partial_kernel), restated: bool [V]."""
    V, tb, eos = G.V, G.tb, G.eos
    ids = [int(i) for i in ids]
    t = len(ids)
    n_gen = t - N_PROMPT
    last_ts = n_gen >= 1 and ids[t - 1] >= tb
    penult_ts = n_gen < 2 or ids[t - 2] >= tb
    last_tok = max([i for i in ids[N_PROMPT:] if i >= tb], default=-1)
    if last_tok >= 0:
        if last_ts and not penult_ts:
            ts_floor = last_tok + (1 if fault == "floor_repeat" else 0)
        else:
            ts_floor = last_tok + (0 if fault == "floor_next" else 1)
    else:
        ts_floor = tb
    at_begin = n_gen == 0
    ts_cap = tb + MAX_INITIAL - (1 if fault == "cap" else 0) if at_begin else 0x7fffffff
    v = np.arange(V)
    d = np.zeros(V, bool)
    d[G.suppress] = True
    if at_begin:
        d[G.begin_suppress] = True
    if n_gen < min_new and fault != "eos_unmasked":
        d[eos] = True
    if last_ts:
        d |= (v >= tb) if penult_ts else (v < eos)
    d |= (v >= tb) & (v < ts_floor)
    if at_begin:
        d |= (v < tb) | (v > ts_cap)
    return d


def _sorted_pairs(val, idx, sign):
    o = np.lexsort((sign * idx, -val))
    return val[o], idx[o]


def kernel_model(G: Gram, ids, x, min_new, n_cand, fault=None):
    """x: f32 [V] raw logits (the pad columns hold HOT_PAD, as under the hook).  -> (ids int32 [n_cand], values f32 [n_cand]) of
    the two-stage form.  fault: None or one of FAULTS --
      allowed_norm  the normaliser taken over allowed tokens only
      pad_norm      the pad columns enter the normaliser
      tie_high      an exact tie resolved to the higher id
      best_only     the merge takes only each slice's best
      text_kept     the text lists not ignored when a timestamp is forced
      ts_norescale  the timestamp mass re-based on the slice's own maximum but not rescaled to the row's
      floor_repeat  ts_floor off by one where the last timestamp may repeat
      floor_next    ts_floor off by one where timestamps must increase
      cap           ts_cap off by one
      eos_unmasked  eos not masked under min_new_tokens
      load13        the elements of a thread's 13th load (lo + 12 * 256 ..) dropped
      repeat        a slice's shorter list repeats its last entry instead of padding
      inf_slice     a slice whose logits are all -inf (its sum is expf(-inf - -inf) = NaN) enters the row's normaliser"""
    assert fault is None or fault in FAULTS
    f32 = np.float32
    V, tb, per = G.V, G.tb, G.per
    assert per <= PER_LANE * THREADS
    x = np.asarray(x, f32)
    xp = np.concatenate([x[:V], np.full(G.Vpad - V, HOT_PAD, f32)])
    dead = _dead(G, ids, min_new, fault)
    sign = -1 if fault == "tie_high" else 1
    recs, lists = [], []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for sl in range(NS):
            lo, hi = G.bounds(sl)
            idx = np.arange(lo, hi)
            if fault == "load13":
                idx = idx[idx - lo < (PER_LANE - 1) * THREADS]
            raw = xp[idx]
            xa = np.where(dead[idx] | ~(raw > -np.inf), f32(-np.inf), raw)          # NaN: no candidate
            nidx, nraw = idx, raw
            if fault == "pad_norm" and hi == V:
                nidx = np.arange(lo, G.Vpad); nraw = xp[nidx]
            if fault == "allowed_norm":
                nraw = xa
            rmax = f32(np.fmax.reduce(nraw, initial=f32(-np.inf)))
            rsum = np.exp(nraw - rmax, dtype=f32).sum(dtype=f32)
            is_ts = idx >= tb
            btext = f32(np.fmax.reduce(xa[~is_ts], initial=f32(-np.inf)))
            bts = f32(np.fmax.reduce(xa[is_ts], initial=f32(-np.inf)))
            live_ts = is_ts & (xa > -np.inf)
            tsum = np.exp(xa[live_ts] - bts, dtype=f32).sum(dtype=f32) if live_ts.any() else f32(0)
            recs.append((rmax, rsum, btext, bts, tsum))
            for kind in (0, 1):
                m = (is_ts if kind else ~is_ts) & (xa > -np.inf)
                val, ii = _sorted_pairs(xa[m], idx[m], sign)
                val, ii = val[:n_cand], ii[:n_cand]
                if fault == "repeat" and 0 < len(val) < n_cand:
                    val = np.concatenate([val, np.full(n_cand - len(val), val[-1], f32)])
                    ii = np.concatenate([ii, np.full(n_cand - len(ii), ii[-1])])
                lists.append((kind, val, ii))
        rmax = np.asarray([r[0] for r in recs], f32); rsum = np.asarray([r[1] for r in recs], f32)
        btext = np.asarray([r[2] for r in recs], f32); bts = np.asarray([r[3] for r in recs], f32)
        tsum = np.asarray([r[4] for r in recs], f32)
        gmax, gtext, gts = rmax.max(), btext.max(), bts.max()
        M = max(gtext, gts)
        lr = np.ones(NS, bool) if fault == "inf_slice" else rmax > -np.inf
        S = (rsum[lr] * np.exp(rmax[lr] - gmax, dtype=f32)).sum(dtype=f32)
        lt = bts > -np.inf
        T = (tsum[lt] if fault == "ts_norescale" else tsum[lt] * np.exp(bts[lt] - M, dtype=f32)).sum(dtype=f32)
        logz = np.log(S, dtype=f32)
        force_ts = bool(T > 0) and bool(np.log(T, dtype=f32) > gtext - M)
        vals, toks = [], []
        for kind, val, ii in lists:
            if force_ts and kind == 0 and fault != "text_kept":
                continue
            if fault == "best_only":
                val, ii = val[:1], ii[:1]
            vals.append(val); toks.append(ii)
        val = np.concatenate(vals) if vals else np.zeros(0, f32)
        ii = np.concatenate(toks) if toks else np.zeros(0, np.int64)
        val, ii = _sorted_pairs(val, ii, sign)
        val, ii = val[:n_cand], ii[:n_cand]
        out_i = np.full(n_cand, -1, np.int32)
        out_v = np.full(n_cand, -np.inf, f32)
        out_i[:len(ii)] = ii
        out_v[:len(ii)] = ((val - gmax).astype(f32) - logz).astype(f32)
    return out_i, out_v


# ---- row tables ------------------------------------------------------------------------------------------------------------------
def _states(G: Gram):
    tb, A, Bt = G.tb, ord("a"), ord("b")
    return {"text": [tb, A], "begin": [], "close": [tb, A, tb + 10], "tsts": [tb, A, tb + 10, tb + 10],
            "pair_text": [tb, A, tb + 10, tb + 10, Bt]}


def _allowed(G: Gram, gen, min_new=0):
    """bool [V]: what the processors before the mass rule leave finite in this grammar state (from the oracle)."""
    ids = np.asarray(G.prompt + list(gen), np.int64)
    return np.isfinite(OL._masked(G.spec(min_new), ids[None], np.zeros((1, G.V), np.float32), N_PROMPT, N_PROMPT)[0])


def _make_decidable(G, ids, x, mn):
    """A row whose timestamp-mass margin is too close to zero is replaced: its timestamp logits move by 0.5 until it is clear."""
    for _ in range(12):
        r = reference(G, ids, x, mn)
        if r.decidable:
            return x, r
        x = x.copy(); x[G.tb:] += np.float32(0.5)
    raise AssertionError("no decidable replacement found")


@functools.lru_cache(maxsize=None)
def table(which: str):
    """[(name, ids int64 [t], x f32 [V], min_new_tokens)] and, index-aligned, the rows' references: (rows, refs)."""
    G = gram(which)
    V, tb, per = G.V, G.tb, G.per
    rng = np.random.default_rng(11 if which == "tiny" else 12)
    st = _states(G)
    raw = []                                             # (name, gen, x, min_new)

    def noise(level=-5.0, scale=1.0):
        return (rng.standard_normal(V) * scale + level).astype(np.float32)

    def variants(name, x, gen="text", mn=0):
        """the row as crafted, with every timestamp 40 lower (text wins), and 40 higher (a timestamp is forced)"""
        for tag, d in (("", 0.0), ("/ts_low", -40.0), ("/ts_high", 40.0)):
            y = x.copy(); y[tb:] += np.float32(d)
            raw.append((name + tag, st[gen], y, mn))

    def pick(ok, lo, hi, n, want=True):
        c = lo + np.flatnonzero(ok[lo:hi] == want)
        assert len(c) >= n, (lo, hi, n, want, len(c))
        return c[:n]

    ok_text = _allowed(G, st["text"])
    sl_tb = G.slice_of(tb)
    assert G.slice_of(tb - 1) == sl_tb
    lo_tb, hi_tb = G.bounds(sl_tb)
    lo_last, hi_last = G.bounds(NS - 1)
    text_slices = [s for s in range(NS) if G.bounds(s)[1] <= tb]
    s_text = text_slices[min(1, len(text_slices) - 1)]

    # exact ties across every slice boundary: allowed and masked, text and timestamp tokens as the vocabulary has them there
    x = noise()
    for s in range(1, NS):
        x[[s * per - 1, s * per]] = 30.0
    variants("tie_across_slice_boundaries", x)
    # ... across the load boundary of one thread (lo + 255 / lo + 256; thread 9's elements i, i + 256, i + 512) where a thread holds
    # more than one element, between neighbouring threads otherwise
    x = noise()
    for s in (s_text, sl_tb, NS - 1):
        lo, hi = G.bounds(s)
        if hi - lo > 2 * THREADS + 9:
            x[[lo + 255, lo + 256, lo + 9, lo + 9 + 256, lo + 9 + 512]] = 31.0
        else:
            x[[lo + 3, lo + 4, lo + 9]] = 31.0
    variants("tie_across_load_boundary", x)
    # ... across wave boundaries (threads 63 / 64, 127 / 128)
    x = noise()
    for s in (0, s_text, sl_tb, NS - 1):
        lo, hi = G.bounds(s)
        for o in (63, 64, 127, 128):
            if lo + o < hi:
                x[lo + o] = 32.0
    variants("tie_across_wave_boundaries", x)
    # ... in the ragged tail of a slice: the first element of its last load, its last two elements
    x = noise()
    for s in (s_text, NS - 2):
        lo, hi = G.bounds(s)
        x[[lo + ((hi - lo - 1) // THREADS) * THREADS, hi - 2, hi - 1]] = 33.0
    variants("tie_in_ragged_tail", x)
    # ... in the last, shorter slice and at V - 1 / V - 2 next to the hot pad columns
    x = noise()
    x[[lo_last, (lo_last + hi_last) // 2, V - 3, V - 2, V - 1]] = 34.0
    x[V - 2] = 34.5
    variants("last_slice_and_last_columns", x)
    # the slice that holds both tb - 1 and tb: winners of both kinds in it, ties between them and with masked neighbours
    x = noise()
    tx = pick(ok_text, lo_tb, tb, 3)
    ts = pick(ok_text, tb, hi_tb, 3)
    x[tx] = [35.0, 35.0, 34.0]; x[ts] = [35.0, 34.0, 34.0]
    x[[tb - 1, tb]] = 35.0                               # <|notimestamps|> is suppressed, <|0.00|> is below ts_floor here
    x[pick(ok_text, lo_tb, tb, 1, want=False)] = 36.0
    variants("text_and_timestamp_winners_in_the_tb_slice", x)
    # all winners in one slice (a text slice and the tb slice), pairs of ties among them, masked tokens among them
    for nm, s in (("text", 0), ("tb", sl_tb)):
        lo, hi = G.bounds(s)
        x = noise()
        hot = lo + rng.choice(hi - lo, min(N_CAND_MAX + 6, hi - lo), replace=False)
        x[hot] = 40.0 + (np.arange(len(hot), dtype=np.float32) // 2) * 0.25
        variants(f"all_winners_in_the_{nm}_slice", x)
    # slices with 0, 1 and n_cand - 1 allowed tokens (n_cand = 2, 10, 64), one with plenty; masked tokens finite among them
    x = np.full(V, -np.inf, np.float32)
    free = [s for s in range(NS)]
    lo, hi = G.bounds(free[-1]); x[pick(ok_text, lo, hi, 1)] = 20.0
    lo, hi = G.bounds(free[-2]); x[pick(ok_text, lo, hi, 1)] = 21.0                                  # n_cand = 2: one
    lo, hi = G.bounds(free[-3]); x[pick(ok_text, lo, hi, 9)] = 10.0 + np.arange(9, dtype=np.float32)
    lo, hi = G.bounds(free[-4]); x[pick(ok_text, lo, hi, 63)] = 5.0 + (np.arange(63, dtype=np.float32) // 3)
    lo, hi = G.bounds(free[-5]); x[lo:hi] = noise(0.0)[lo:hi]
    x[~ok_text & (rng.random(V) < 0.5)] = 25.0                                                       # masked and finite
    for tag, d in (("", 0.0), ("/text_high", 30.0)):
        y = x.copy(); y[pick(ok_text, 0, tb, 5)] = np.float32(d) + np.arange(5, dtype=np.float32)
        raw.append(("slices_with_0_1_and_n_cand-1_allowed" + tag, st["text"], y, 0))
    # fewer than n_cand allowed in the row: five finite allowed tokens; the begin state allows 51 timestamps, no more
    x = np.full(V, -np.inf, np.float32)
    x[pick(ok_text, 0, tb, 3)] = [1.0, 1.0, -2.0]; x[pick(ok_text, tb, V, 2)] = [0.5, -3.0]
    raw.append(("five_allowed_tokens", st["text"], x, 0))
    raw.append(("begin_state_allows_51_timestamps", st["begin"], noise(0.0, 3.0), 0))
    # the other grammar states over the same geometry: ties at the slice boundaries and in the tb slice
    for gname in ("close", "tsts", "pair_text"):
        x = noise()
        for s in range(1, NS):
            x[[s * per - 1, s * per]] = 30.0
        x[[tb + 9, tb + 10, tb + 11, tb + 12]] = [31.0, 31.0, 31.0, 30.0]
        x[[G.eos, ord("a"), ord("b")]] = [31.0, 31.0, 31.0]
        raw.append((f"ties_in_state_{gname}", st[gname], x, 0))
        raw.append((f"ties_in_state_{gname}/min_new", st[gname], x, 12))
    # degenerate rows
    raw.append(("all_minus_inf", st["text"], np.full(V, -np.inf, np.float32), 0))
    x = noise(0.0, 3.0); x[pick(ok_text, per, tb, 1)] = np.nan; x[3] = 12.0
    raw.append(("nan_above_everything", st["text"], x, 0))
    # a NaN at an allowed timestamp while the other timestamps' mass forces one: the NaN stays out of the mass in both forms
    x = noise(); t4 = pick(ok_text, tb, V, 4); x[t4[:3]] = 20.0; x[t4[3]] = np.nan; x[pick(ok_text, 0, tb, 1)] = 10.0
    raw.append(("nan_at_an_allowed_timestamp", st["text"], x, 0))
    # the raw maximum is a masked token: rmax differs from the best allowed value
    x = noise(0.0, 2.0); x[G.v.notimestamps] = 50.0; x[G.v.sot] = 49.0
    variants("raw_maximum_is_masked", x)
    # every grammar state of tests/sampler_cases.py, and seeded random rows over random grammar states
    for name, ids, lg, mn in SC.cases(G.v, V):
        raw.append(("case:" + name, list(ids[N_PROMPT:]), lg, mn))
    for name, ids, lg, mn in SC.cases(G.v, V, seed=1):
        if name.startswith("random"):
            raw.append(("seed1:" + name, list(ids[N_PROMPT:]), lg, mn))

    rows, refs = [], []
    for name, gen, x, mn in raw:
        ids = np.asarray(G.prompt + [int(i) for i in gen], np.int64)
        x, r = _make_decidable(G, ids, np.asarray(x, np.float32), mn)
        x.setflags(write=False)
        rows.append((name, ids, x, int(mn)))
        refs.append(r)
    return rows, refs


def groups(rows, size):
    """Row indices in launches of up to `size` rows that share (t, min_new_tokens)."""
    by = {}
    for i, (name, ids, x, mn) in enumerate(rows):
        by.setdefault((len(ids), mn), []).append(i)
    out = []
    for key, idx in by.items():
        out += [idx[lo:lo + size] for lo in range(0, len(idx), size)]
    return out


# ---- the residual grid of the 16-bit engines (csrc/common.h: resid_grid) ------------------------------------------------------------
def resid_grid(v):
    """rintf(v * 4096) * (1 / 4096) in float32: both multiplications are by powers of two, hence exact, and numpy's rint rounds
    half to even as rintf does under the default rounding mode."""
    v = np.asarray(v, np.float32)
    return (np.rint(v * np.float32(4096.0)) * np.float32(1.0 / 4096.0)).astype(np.float32)
