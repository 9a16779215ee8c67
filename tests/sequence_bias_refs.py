"""sequence_bias in numpy: the semantics of transformers' SequenceBiasLogitsProcessor restated without torch, plus its argument
check.  tests/test_sequence_bias_refs.py holds this file to the installed processor bit for bit; the GPU tests hold the sampler
kernels (cw_set_sequence_bias) to ``fl32(logits + dense_bias)``.

At the step that writes sequence index t (``ids[:, :t]`` exist, prompt included) a sequence of length L applies to a row iff
L == 1, or L <= t and ``ids[t-L+1 .. t-1] == seq[:L-1]``.  The row's bias of token v is a float32 sum: the length-1 entry of v,
then, in table order, every longer sequence ending in v (its bias where it applies, 0.0 where it does not).

``fault`` plants one of the mistakes the comparison has to reject (None: the correct code)."""
from __future__ import annotations

import numpy as np

MAX_SEQ, MAX_LEN = 256, 16
FAULTS = ("length_minus_one_fits", "window_off_by_one", "length_one_last", "row_zero_for_all")


def validate(sequence_bias, vocab_size=None):
    """The table as an ordered list of (ids tuple, float): what the processor's ``_validate_arguments`` +
    ``_convert_list_arguments_into_dict`` leave, or ValueError.  With ``vocab_size`` also what the engine adds: ids below it,
    non-empty sequences of at most MAX_LEN tokens, at most MAX_SEQ of them, finite biases."""
    sb = sequence_bias
    if not isinstance(sb, (dict, list)) or len(sb) == 0:
        raise ValueError("sequence_bias: a non-empty dict or list")
    is_int = lambda t: isinstance(t, (int, np.integer)) and not isinstance(t, (bool, np.bool_))
    if isinstance(sb, dict):
        for key in sb:
            if not isinstance(key, tuple):
                raise ValueError("sequence_bias: dict keys are tuples")
            if len(key) == 0 or any(not is_int(t) or t < 0 for t in key):
                raise ValueError("sequence_bias: keys are non-empty tuples of non-negative integers")
        items = list(sb.items())
    else:
        for e in sb:
            if not isinstance(e, (list, tuple)) or len(e) != 2 or not isinstance(e[0], list) or len(e[0]) == 0:
                raise ValueError("sequence_bias: elements are [non-empty list of ids, float]")
            if any(not is_int(t) or t <= 0 for t in e[0]) or not isinstance(e[1], float):
                raise ValueError("sequence_bias: elements are [list of positive integers, float]")
        items = list({tuple(e[0]): e[1] for e in sb}.items())           # a repeated sequence: the last bias, the first place
    if any(not isinstance(b, float) for _, b in items):
        raise ValueError("sequence_bias: biases are floats")
    if vocab_size is not None:
        if len(items) > MAX_SEQ or any(len(k) > MAX_LEN for k, _ in items):
            raise ValueError("sequence_bias: beyond the engine's limits")
        if any(t >= vocab_size for k, _ in items for t in k) or any(not np.isfinite(b) for _, b in items):
            raise ValueError("sequence_bias: id outside the vocabulary or non-finite bias")
    return [(tuple(int(t) for t in k), float(b)) for k, b in items]


def dense_bias(ids_rows, t, table, V, fault=None):
    """float32 [nb][V]: the bias every row's logits receive at the step that writes index ``t``.  ``ids_rows`` [nb][>= t]
    (only ``[:, :t]`` is read); ``table`` as ``validate`` returns it."""
    assert fault is None or fault in FAULTS
    ids = np.asarray(ids_rows)[:, :t]
    nb = ids.shape[0]
    out = np.zeros((nb, V), np.float32)
    singles = [(s, b) for s, b in table if len(s) == 1]
    longer = [(s, b) for s, b in table if len(s) > 1]

    def add_singles():
        for s, b in singles:
            out[:, s[0]] = out[:, s[0]] + np.float32(b)

    if fault != "length_one_last":
        add_singles()
    for s, b in longer:
        L = len(s)
        if (L - 1 > t) if fault == "length_minus_one_fits" else (L > t):
            continue
        if fault == "window_off_by_one":
            win = ids[:, t - L: t - 1]
        else:
            win = ids[:, t - (L - 1): t]
        if win.shape[1] != L - 1:
            continue
        match = np.all(win == np.asarray(s[:-1])[None, :], axis=1)
        if fault == "row_zero_for_all":
            match = np.full(nb, match[0])
        out[:, s[-1]] = out[:, s[-1]] + np.where(match, np.float32(b), np.float32(0.0))
    if fault == "length_one_last":
        add_singles()
    return out


def biased(logits, ids_rows, t, table, fault=None):
    """fl32(logits + dense_bias): what every consumer of the processed scores sees (one rounded add)."""
    lg = np.asarray(logits, np.float32)
    return (lg + dense_bias(ids_rows, t, table, lg.shape[1], fault)).astype(np.float32)
