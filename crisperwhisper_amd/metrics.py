"""Timestamp-accuracy harness for BASELINE config 5 (word-timestamp F1 / mean IoU at a collar), to be run when
real CrisperWhisper weights and annotated DE/EN speech are available (neither is in this image).

Definition follows the reference's evaluation description (REF/README.md:78-90: "F1 Score / Avg IOU" with a collar):
reference and hypothesis word boundaries are matched one-to-one in time order; a hypothesis boundary is a hit if
it lies within ``collar`` seconds of an unmatched reference boundary.  IoU is averaged over words matched by text
alignment (same index after a longest-common-subsequence alignment of the word strings).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple


def _boundaries(words: Sequence[Dict]) -> List[float]:
    out: List[float] = []
    for w in words:
        out.extend([float(w["timestamp"][0]), float(w["timestamp"][1])])
    return sorted(out)


def boundary_f1(ref: Sequence[Dict], hyp: Sequence[Dict], collar: float = 0.2) -> Tuple[float, float, float]:
    """(precision, recall, f1) of hypothesis word boundaries against reference boundaries within +-collar."""
    r, h = _boundaries(ref), _boundaries(hyp)
    i = j = hits = 0
    while i < len(r) and j < len(h):
        if abs(r[i] - h[j]) <= collar + 1e-12:
            hits += 1; i += 1; j += 1
        elif h[j] < r[i]:
            j += 1
        else:
            i += 1
    p = hits / len(h) if h else 0.0
    rec = hits / len(r) if r else 0.0
    return p, rec, (2 * p * rec / (p + rec) if p + rec else 0.0)


def _lcs_pairs(a: List[str], b: List[str]) -> List[Tuple[int, int]]:
    n, m = len(a), len(b)
    dp = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n - 1, -1, -1):
        for j in range(m - 1, -1, -1):
            dp[i][j] = dp[i + 1][j + 1] + 1 if a[i] == b[j] else max(dp[i + 1][j], dp[i][j + 1])
    i = j = 0
    pairs = []
    while i < n and j < m:
        if a[i] == b[j]:
            pairs.append((i, j)); i += 1; j += 1
        elif dp[i + 1][j] >= dp[i][j + 1]:
            i += 1
        else:
            j += 1
    return pairs


def mean_iou(ref: Sequence[Dict], hyp: Sequence[Dict]) -> float:
    """Mean temporal IoU over words aligned by text."""
    pairs = _lcs_pairs([w["text"].strip() for w in ref], [w["text"].strip() for w in hyp])
    if not pairs:
        return 0.0
    tot = 0.0
    for i, j in pairs:
        (a0, a1), (b0, b1) = ref[i]["timestamp"], hyp[j]["timestamp"]
        inter = max(0.0, min(a1, b1) - max(a0, b0))
        union = max(a1, b1) - min(a0, b0)
        tot += inter / union if union > 0 else (1.0 if inter == 0 and a0 == b0 else 0.0)
    return tot / len(pairs)


# ---------------------------------------------------------------------------------------------------------------------------
# Alignment-head selection (CrisperWhisperPipeline.rank_alignment_heads): the word-timing quality of one head, host numpy.
#
# A head is judged by how the word chunks its own forced alignment produces compare with reference word intervals of the same
# words, index by index (the transcript is given, so there is nothing to match):
#   * mean absolute boundary error: |start - ref start| and |end - ref end| over every word, in seconds;
#   * share of boundaries within `collar` seconds of the reference;
#   * mean intersection over union of the word intervals (0 when both intervals are empty and apart, 1 when both are the same
#     point);
#   * mean similarity of the tokens' attention rows to their words' intervals (cw_align_heads; NaNs are left out).
# Heads are ranked by the share within the collar, ties broken by mean IoU, then similarity, then (layer, head).
# ---------------------------------------------------------------------------------------------------------------------------
import numpy as np

COLLAR_EPS = 1e-9           # a boundary exactly `collar` away counts as within it (timestamps are multiples of 0.02 s)


def boundary_errors(pred, ref) -> np.ndarray:
    """|pred - ref| of the word boundaries: pred / ref [W][2] (start, end) seconds -> [W][2]."""
    p, r = np.asarray(pred, np.float64).reshape(-1, 2), np.asarray(ref, np.float64).reshape(-1, 2)
    if p.shape != r.shape:
        raise ValueError(f"{p.shape[0]} predicted words against {r.shape[0]} reference words")
    return np.abs(p - r)


def interval_iou(pred, ref) -> np.ndarray:
    """Intersection over union of word intervals, [W]."""
    p, r = np.asarray(pred, np.float64).reshape(-1, 2), np.asarray(ref, np.float64).reshape(-1, 2)
    if p.shape != r.shape:
        raise ValueError(f"{p.shape[0]} predicted words against {r.shape[0]} reference words")
    ps, pe = np.minimum(p[:, 0], p[:, 1]), np.maximum(p[:, 0], p[:, 1])
    rs, re = np.minimum(r[:, 0], r[:, 1]), np.maximum(r[:, 0], r[:, 1])
    inter = np.maximum(0.0, np.minimum(pe, re) - np.maximum(ps, rs))
    union = np.maximum(pe, re) - np.minimum(ps, rs)
    same_point = (union == 0.0)
    return np.where(same_point, 1.0, inter / np.where(same_point, 1.0, union))


def head_metrics(pred_words: Sequence, ref_words: Sequence, similarity: Sequence = (), collar: float = 0.05) -> Dict[str, float]:
    """Metrics of one head over all inputs: ``pred_words`` / ``ref_words`` per input [W][2], ``similarity`` per input an array
    over the tokens (NaN: undefined)."""
    if len(pred_words) != len(ref_words):
        raise ValueError(f"{len(pred_words)} inputs predicted against {len(ref_words)} references")
    errs = [boundary_errors(p, r) for p, r in zip(pred_words, ref_words)]
    ious = [interval_iou(p, r) for p, r in zip(pred_words, ref_words)]
    e = np.concatenate([x.reshape(-1) for x in errs]) if errs else np.zeros(0)
    iou = np.concatenate(ious) if ious else np.zeros(0)
    sim = np.concatenate([np.asarray(s, np.float64).reshape(-1) for s in similarity]) if len(similarity) else np.zeros(0)
    sim = sim[np.isfinite(sim)]
    n_within = int(np.sum(e <= collar + COLLAR_EPS))
    return {"mean_abs_error": float(e.mean()) if e.size else float("nan"),
            "within_collar": n_within / e.size if e.size else float("nan"),
            "n_within": n_within, "n_boundaries": int(e.size),
            "mean_iou": float(iou.mean()) if iou.size else float("nan"),
            "mean_similarity": float(sim.mean()) if sim.size else float("nan")}


def _desc(x: float) -> float:
    return -x if np.isfinite(x) else float("inf")               # NaN sorts last


def rank_heads(heads: Sequence[Sequence[int]], metrics: Sequence[Dict[str, float]], top: int = 15) -> Dict[str, List]:
    """-> {"ranking": [{"head": [l, h], **metrics}, ...] best first, "alignment_heads": the first ``top`` heads}."""
    if len(heads) != len(metrics):
        raise ValueError(f"{len(heads)} heads with {len(metrics)} metric rows")
    if top < 1:
        raise ValueError("top must be at least 1")
    order = sorted(range(len(heads)), key=lambda k: (_desc(metrics[k]["within_collar"]), _desc(metrics[k]["mean_iou"]),
                                                     _desc(metrics[k]["mean_similarity"]), int(heads[k][0]), int(heads[k][1])))
    ranking = [dict(head=[int(heads[k][0]), int(heads[k][1])], **metrics[k]) for k in order]
    return {"ranking": ranking, "alignment_heads": [r["head"] for r in ranking[:top]]}
