"""References for per-head forced alignment (cw_align_heads): numpy / float64 only, no device.

Per-head timestamps
-------------------
`head_timestamps` is `oracle.timestamps.extract_token_timestamps`, unchanged, on `weights[:, [k]]`: the timestamp stage of one
head on its own (the head "mean" is over one head).

Similarity
----------
`similarity64` is the float64 definition.  For a row a (the normalised softmax weights of one token over the encoder frames)
and a reference interval [s, e] seconds, over the frames 0 <= j < n_cols:

    f0 = floor(s / 0.02),  f1 = max(f0 + 1, ceil(e / 0.02))
    g[j] = 1 for f0 <= j < f1;  g[f0 - k] = g[f1 - 1 + k] = 1 - k / 5 for k = 1 .. 4;  0 elsewhere
    a'[j] = a[j] for f0 - clip <= j < f1 + clip (all j when clip < 0), 0 elsewhere
    similarity = sum a' g / (sqrt(sum a'^2) sqrt(sum g^2)),  NaN when a norm is 0 or the interval is not finite

s and e reach the device as float32; the definition takes those float32 values (converted exactly to float64), so the frame
indices are those of the double-precision division the kernel performs.

`similarity_bound` is a first-order bound on |kernel - similarity64| with u = 2^-24, in the manner of
tests/token_logprob_refs.py: every term is a worst case of the arithmetic the kernel is specified to do, nothing is fitted.

* Each of the three sums (a' g, a'^2, g^2) has non-negative terms, so the relative error of a computed sum is at most the
  number of roundings on the longest path from a term to the result, times u: one rounding for the product, the per-lane chain
  of ceil(n_cols / 64) additions (one wave per row, 64 lanes, fixed order) and the 6 steps of the wave reduction:
  D = 1 + ceil(n_cols / 64) + 6.  (The kernel adds a lane's float4 chunk as a two-level tree before it joins the lane's chain,
  which is never a longer path than this count: one chunk per lane up to 256 frames costs 2 additions where the bound allows
  ceil(n_cols / 64) >= 1 and the reduction steps that add an exact zero -- lanes without frames -- round nothing: 16 live lanes
  leave 4 real steps; beyond 256 frames n chunks per lane cost n + 1 <= 4 n - 3 <= ceil(n_cols / 64).)
* g itself is one correctly rounded division ((5 - k) / 5): relative error u in g, so u more in sum a' g and 2 u more in
  sum g^2 (u after the square root).
* Two sqrtf (correctly rounded: u each; the error of the argument halves), their product (u) and the division (u).

  |err| / |similarity| <= (D + 1) u  +  (D / 2 + 1) u  +  (D / 2 + 1 + 1) u  +  2 u  =  (2 D + 6) u

An absolute 2^-126 covers a result in the subnormal range.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import timestamps as OT

U = 2.0 ** -24
FRAME = 0.02


def head_timestamps(weights, num_frames, n_prompt, width, k):
    """Token timestamps of head k of `weights` [B][Ha][L][S] on its own (oracle.timestamps.extract_token_timestamps)."""
    w = np.asarray(weights)
    return OT.extract_token_timestamps(w[:, [k]], num_frames, n_prompt, width)


def interval_frames(s, e):
    """(f0, f1) of a finite interval given as float32 seconds."""
    s64, e64 = float(np.float32(s)), float(np.float32(e))
    f0 = math.floor(s64 / FRAME)
    f1 = max(f0 + 1, math.ceil(e64 / FRAME))
    return f0, f1


def target(f0, f1, n_cols):
    g = np.zeros(max(n_cols, 0), np.float64)
    for j in range(max(0, f0 - 4), min(n_cols, f1 + 4)):
        if f0 <= j < f1:
            g[j] = 1.0
        elif j < f0:
            g[j] = 1.0 - (f0 - j) / 5.0
        else:
            g[j] = 1.0 - (j - f1 + 1) / 5.0
    return g


def similarity64(row, n_cols, s, e, clip):
    """float64 definition for one row; NaN where undefined."""
    if not (np.isfinite(np.float32(s)) and np.isfinite(np.float32(e))) or n_cols <= 0:
        return float("nan")
    f0, f1 = interval_frames(s, e)
    a = np.asarray(row, np.float32)[:n_cols].astype(np.float64)
    if clip >= 0:
        j = np.arange(n_cols)
        a = np.where((j >= f0 - clip) & (j < f1 + clip), a, 0.0)
    g = target(f0, f1, n_cols)
    na, ng = math.sqrt(float(np.dot(a, a))), math.sqrt(float(np.dot(g, g)))
    if na == 0.0 or ng == 0.0:
        return float("nan")
    return float(np.dot(a, g)) / (na * ng)


def similarity_bound(value, n_cols):
    d = 1 + math.ceil(n_cols / 64) + 6
    return abs(value) * (2 * d + 6) * U + 2.0 ** -126


def similarity_table(attn, n_cols, ref_begin, ref_end, clip):
    """attn [B][Ha][N][S] -> ([Ha][B][N] float64 similarity, [Ha][B][N] bound)."""
    a = np.asarray(attn, np.float32)
    B, Ha, N, _ = a.shape
    out = np.full((Ha, B, N), np.nan)
    bnd = np.zeros((Ha, B, N))
    for b in range(B):
        for h in range(Ha):
            for t in range(N):
                out[h, b, t] = similarity64(a[b, h, t], int(n_cols[b]), ref_begin[b][t], ref_end[b][t], clip)
                bnd[h, b, t] = 0.0 if np.isnan(out[h, b, t]) else similarity_bound(out[h, b, t], int(n_cols[b]))
    return out, bnd


def compare_similarity(got, want, bound):
    """(ok, worst |err| / bound, message): NaN exactly where the definition has NaN, the rest within the bound."""
    got = np.asarray(got, np.float64)
    if got.shape != want.shape:
        return False, float("inf"), f"shape {got.shape} vs {want.shape}"
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if not np.array_equal(nan_g, nan_w):
        i = np.argwhere(nan_g != nan_w)[0]
        return False, float("inf"), f"NaN mismatch at {tuple(i)}: got {got[tuple(i)]}, want {want[tuple(i)]}"
    ok = ~nan_w
    if not ok.any():
        return True, 0.0, ""
    ratio = np.abs(got[ok] - want[ok]) / bound[ok]
    worst = float(ratio.max())
    return worst <= 1.0, worst, f"worst |err| / bound = {worst:.3f}"


# ------------------------------------------------------------------------------------------------------------------------
# numpy model of the cw_align_heads data path, with switchable faults (tests/test_align_heads_refs.py plants each one and checks
# that the comparison against the references rejects it)
# ------------------------------------------------------------------------------------------------------------------------
def ncols_of(num_frames):
    """Frames reaching the DTW for a call's items, as the engine's token_timestamps computes them (HF's slicing, applied twice
    when every item has the same num_frames; for 0 <= num_frames <= 3000 both give min(num_frames // 2, 1500))."""
    nf = np.asarray(num_frames, np.int64)
    return np.minimum(nf // 2, 1500).astype(np.int64)


def model_align_heads(all_weights, n_heads_per_layer, heads, num_frames, n_init, n_ids, width, fault=None):
    """all_weights [B][layers * H][L][S]: the normalised cross-attention rows of every (layer, head), layer-major.  Returns token
    timestamps [len(heads)][B][L + 1 of each row] as cw_align_heads lays them out.  Rows are aligned over their own n_ids[b] - 1
    positions.  fault: None, "head_mean", "swap_layer_head", "slot_order", "ncols_item0"."""
    w = np.asarray(all_weights)
    B = w.shape[0]
    H = n_heads_per_layer
    heads = [tuple(h) for h in heads]
    slot_of = {}
    for k, (l, h) in enumerate(heads):
        idx = (h * H + l) if fault == "swap_layer_head" else (l * H + h)
        slot_of[k] = idx % w.shape[1]
    order = list(range(len(heads)))
    if fault == "slot_order":                     # heads returned by ascending (layer, head) instead of request order
        order = sorted(range(len(heads)), key=lambda k: heads[k])
    nf = np.asarray(num_frames, np.int64)
    out = []
    for k in order:
        per_item = []
        for b in range(B):
            L = int(n_ids[b]) - 1
            cap = w[b:b + 1, :, :L]
            sel = cap[:, [slot_of[k]]]
            if fault == "head_mean":              # the mean over all requested heads left in
                sel = cap[:, [slot_of[j] for j in range(len(heads))]]
            nfb = nf[[0]] if fault == "ncols_item0" else nf[[b]]
            per_item.append(OT.extract_token_timestamps(sel, nfb, n_init, width)[0])
        out.append(per_item)
    return out


def model_similarity(row, n_cols, s, e, clip, fault=None):
    """similarity64 with a planted fault: "ramp_shift" (ramp one frame late), "clip_g" (clipping applied to g instead of a),
    "f1_eq_f0" (a zero-length interval keeps f1 = f0)."""
    if not (np.isfinite(np.float32(s)) and np.isfinite(np.float32(e))) or n_cols <= 0:
        return float("nan")
    f0, f1 = interval_frames(s, e)
    if fault == "f1_eq_f0":
        f1 = max(f0, math.ceil(float(np.float32(e)) / FRAME))
    a = np.asarray(row, np.float32)[:n_cols].astype(np.float64)
    g = target(f0, f1, n_cols)
    if fault == "ramp_shift":
        g = target(f0 + 1, f1 + 1, n_cols)
    j = np.arange(n_cols)
    if clip >= 0:
        win = (j >= f0 - clip) & (j < f1 + clip)
        if fault == "clip_g":
            g = np.where(win, g, 0.0)
        else:
            a = np.where(win, a, 0.0)
    na, ng = math.sqrt(float(np.dot(a, a))), math.sqrt(float(np.dot(g, g)))
    if na == 0.0 or ng == 0.0:
        return float("nan")
    return float(np.dot(a, g)) / (na * ng)
