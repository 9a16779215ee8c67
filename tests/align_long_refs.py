"""Float64 restatements of what cw_align_cut_tokens computes on the device (csrc/score.hip STOP forms, csrc/align.hip
align_cut_kernel), for the tests of align_long.

stop_logprob(logits, eos, tb)     logsumexp(logit[n], n in S) - logsumexp(all logits), S = {eos} + {n >= tb}; -inf for an empty S
cut(logprob, stop, mask, force)   S[n] = sum_{i<n} logprob[i] + stop[n], n = 0 .. N (N = len(logprob) - 1; the last logprob is the
                                  eos's and enters no candidate); the allowed n of the largest S[n], the lowest on an exact tie;
                                  forced: N.  The prefix sum is np.cumsum in float64 -- sequential and ascending, the order of
                                  the kernel -- over the float32 inputs; the score is S[cut] rounded once to float32.
"""
import numpy as np


def _lse(x):
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return -np.inf
    m = x.max()
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.exp(x - m).sum()))


def stop_set(V, eos, tb):
    s = np.zeros(V, bool)
    s[eos] = True
    s[tb:] = True
    return s


def stop_logprob(logits, eos, tb):
    """logits [V] or [M][V] (any float type, taken to float64) -> float64 scalar or [M]."""
    l = np.asarray(logits, np.float64)
    if l.ndim == 1:
        return _lse(l[stop_set(l.shape[0], eos, tb)]) - _lse(l)
    s = stop_set(l.shape[1], eos, tb)
    return np.array([_lse(r[s]) - _lse(r) for r in l])


def prefix_scores(logprob, stop):
    """S[0 .. N] in float64 from float32 inputs of N + 1 entries each."""
    lp = np.asarray(logprob, np.float32).astype(np.float64)
    st = np.asarray(stop, np.float32).astype(np.float64)
    assert lp.shape == st.shape and lp.ndim == 1 and lp.size >= 1
    pre = np.concatenate([[0.0], np.cumsum(lp[:-1])])
    return pre + st


def cut(logprob, stop, mask, force):
    """-> (cut, float32 cut_score).  mask: N + 1 flags.  Raises for an unforced row without an allowed candidate."""
    S = prefix_scores(logprob, stop)
    N = S.size - 1
    if force:
        return N, np.float32(S[N])
    ok = np.asarray(mask).astype(bool)
    assert ok.shape == S.shape
    if not ok.any():
        raise ValueError("no allowed cut")
    best = -1
    for n in range(N + 1):
        if ok[n] and (best < 0 or S[n] > S[best]):
            best = n
    return best, np.float32(S[best])
