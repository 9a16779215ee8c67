"""Float64 / numpy restatement of the engine's seeded sampler (include/crisperwhisper.h, cw_set_sampling) for the tests:
Philox4x32-10, the uniform and Gumbel transforms, the logits processors of the greedy path, and the check that a sampled token
is the float64 argmax of the perturbed scores unless the two best are closer than the kernel's f32 arithmetic can tell apart."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32 values in any integer dtype) -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
    return np.stack(c, axis=-1).astype(np.uint32)


def gumbel_noise(V, t, seed, stream):
    """g_v, v = 0 .. V-1, in float64: key (seed_lo, seed_hi), counter (v >> 2, t, stream_lo, stream_hi), word v & 3,
    u = ((x >> 8) + 0.5) * 2^-24, g = -log(-log(u)) (-log(u) through log1p(-(1 - u)) in the upper half, where 1 - u is the
    better conditioned form in float64 too)."""
    n4 = (V + 3) // 4
    ctr = np.zeros((n4, 4), np.uint64)
    ctr[:, 0] = np.arange(n4)
    ctr[:, 1] = t
    ctr[:, 2] = stream & MASK
    ctr[:, 3] = (stream >> 32) & MASK
    key = np.zeros((n4, 2), np.uint64)
    key[:, 0] = seed & MASK
    key[:, 1] = (seed >> 32) & MASK
    x = philox4x32_10(ctr, key).reshape(-1)[:V]
    n = (x >> np.uint32(8)).astype(np.float64)
    low = n < 2.0 ** 23
    e = np.where(low, -np.log((n + 0.5) * 2.0 ** -24), -np.log1p(-((2.0 ** 24 - n - 0.5) * 2.0 ** -24)))
    return -np.log(e)


def processed_scores(spec, logits, ids, n_prompt, min_new_tokens=0):
    """The logits processors of the greedy path on one row (MinNewTokensLength, SuppressTokensAtBegin, SuppressTokens,
    WhisperTimeStamp: TF/generation/logits_process.py:203-260, 1816-2047), in float64.  ``ids``: prompt + tokens so far.
    Returns (scores with -inf at every token that is not allowed, force_ts)."""
    s = np.asarray(logits, np.float64).copy()
    tb, eos = spec.timestamp_begin, spec.eos_token_id
    seq = list(ids[n_prompt:])
    n_gen = len(seq)
    s[list(spec.suppress_tokens)] = -np.inf
    s[spec.no_timestamps_token_id] = -np.inf
    if n_gen == 0:
        s[list(spec.begin_suppress_tokens)] = -np.inf
    if n_gen < min_new_tokens:
        s[eos] = -np.inf
    last_ts = n_gen >= 1 and seq[-1] >= tb
    penult_ts = n_gen < 2 or seq[-2] >= tb
    if last_ts:
        if penult_ts:
            s[tb:] = -np.inf
        else:
            s[:eos] = -np.inf
    stamps = [t for t in seq if t >= tb]
    if stamps:
        floor = stamps[-1] if (last_ts and not penult_ts) else stamps[-1] + 1
        s[tb:floor] = -np.inf
    if n_gen == 0:
        s[:tb] = -np.inf
        if spec.max_initial_timestamp_index is not None:
            s[tb + spec.max_initial_timestamp_index + 1:] = -np.inf
    m = s.max()
    force_ts = False
    if np.isfinite(m):
        ts_mass = np.exp(s[tb:] - m).sum()
        text_max = s[:tb].max()
        force_ts = bool(ts_mass > 0.0 and np.log(ts_mass) > text_max - m)
    if force_ts:
        s[:tb] = -np.inf
    return s, force_ts


# The kernel's f32 arithmetic on one candidate, fl(fl(s / T) + g32), against the exact s / T + g:
#   fl(s / T): correctly rounded division, relative error <= 2^-24;
#   e = -logf(u) or -log1pf(-(1 - u)) on an exactly represented argument: <= 2 ulp, relative error <= 2^-22;
#   g32 = -logf(e): the relative error of e becomes an absolute 2^-22 in log(e); the call itself adds <= 2 ulp of |g|,
#        |g| <= -log(-log(1 - 2^-25)) < 17.4, so <= 2^-22 * 17.4; together < 18.4 * 2^-22 = 4.4e-6;
#   the final sum: relative error <= 2^-24.
# The two best candidates can therefore change places only when the exact scores differ by less than the sum of their two errors.
LOG_TERM = 18.4 * 2.0 ** -22


def candidate_error(a_over_t, perturbed):
    return 2.0 ** -24 * (abs(a_over_t) + abs(perturbed)) + LOG_TERM


def check_token(spec, logits, ids, n_prompt, token, temperature, seed, stream, min_new_tokens=0):
    """Returns ("ok" | "close" | "wrong", detail).  "close": the float64 margin between the two best perturbed scores is below
    the bound derived above, the step says nothing."""
    s, force_ts = processed_scores(spec, logits, ids, n_prompt, min_new_tokens)
    t = len(ids)
    g = gumbel_noise(s.shape[0], t, seed, stream)
    a = s / temperature
    p = a + g
    order = np.argsort(-p, kind="stable")
    b0, b1 = int(order[0]), int(order[1])
    margin = p[b0] - p[b1] if np.isfinite(p[b1]) else np.inf
    bound = candidate_error(a[b0], p[b0]) + (candidate_error(a[b1], p[b1]) if np.isfinite(p[b1]) else 0.0)
    assert bound < 2e-3, bound                      # the issue's "order 1e-3": a wider bound would be a wrong bound
    if margin < bound:
        return "close", (margin, bound)
    if token == b0:
        return "ok", (margin, bound)
    return "wrong", {"t": t, "token": int(token), "want": b0, "margin": float(margin), "bound": float(bound), "force_ts": force_ts,
                     "p_token": float(p[token]), "p_want": float(p[b0])}
