"""The seeded sampler of the decode step (cw_set_sampling; sample_partial_kernel / sample_kernel in csrc/elementwise.hip) on the
device: every sampled token against the float64 argmax of the perturbed scores, the distribution of the draws, independence of
the batch layout, and the greedy path left bit for bit as it was.

Exactness bound.  The token is argmax_v fl(fl(s_v / T) + g_v), g_v = -logf(-logf(u_v)) in f32 (tests/sampling_ref.py restates
the definition of include/crisperwhisper.h in numpy).  Against the exact s_v / T + g_v one candidate is off by at most
    2^-24 |s/T|            the correctly rounded division,
  + 18.4 * 2^-22           the two logarithms: the inner one (logf, or log1pf on 1 - u where u itself is not an f32 number) is
                           good to 2 ulp, a relative 2^-22 that the outer logarithm turns into an absolute 2^-22; the outer call
                           adds 2 ulp of |g| <= 17.4 (u >= 2^-25),
  + 2^-24 |s/T + g|        the rounding of the sum,
and the kernel can only prefer the second best token when the float64 margin between the two best is below the sum of their two
errors.  With |s / T| of order 100 that is about 2e-5 (asserted < 2e-3 per step).  Steps inside the bound are left out; the
gap between the two largest perturbed scores has density at most 1, so at most about one step in 10^4 may be -- the test allows
1 %.  The timestamp rule itself is evaluated by the kernel in f32 on the unperturbed scores, as in the greedy path."""
import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from crisperwhisper_amd.generation import stream_id
from tests import helpers as Hh
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
TEMPS = [0.2, 0.6, 1.0]
CHI2_7_1E6 = 40.521831234179864       # upper 1e-6 quantile of chi-square with 7 degrees of freedom


@pytest.fixture(scope="module")
def tiny():
    return Hh.tiny_setup()


@pytest.fixture(scope="module")
def engines(tiny):
    g, v, W, spec = tiny
    out = {}
    for dt in DTYPES:
        e = Engine(spec, dtype=dt, max_batch=64)
        e.load_state_dict(W)
        out[dt] = e
    yield out
    for e in out.values():
        e.close()


def _prompt(v, nb):
    return np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (nb, 1))


def _clips(nb, secs=2):
    kinds = ("noise", "chirp", "mixed")
    return [syn.synth_audio(100 + b, secs * 16000, kinds[b % 3]) for b in range(nb)]


def _tally(results):
    wrong = [d for r, d in results if r == "wrong"]
    close = sum(1 for r, _ in results if r == "close")
    print(f"steps {len(results)} left out {close} wrong {len(wrong)}")
    assert not wrong, wrong[:3]
    assert close <= 0.01 * len(results), (close, len(results))


@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("nb", [1, 8, 64])
@pytest.mark.parametrize("dt", DTYPES)
def test_hook_tokens_are_the_float64_argmax(tiny, engines, dt, nb, temp):
    """cw_test_sample_seeded on random logits and histories that reach every branch of the timestamp grammar."""
    g, v, W, spec = tiny
    eng = engines[dt]
    rng = np.random.default_rng(1000 * nb + int(temp * 10))
    tb, V = spec.timestamp_begin, spec.vocab_size
    results = []
    for hist in ([], [tb + 3], [tb + 3, 40], [tb + 3, 40, 41], [tb + 3, 40, tb + 9], [tb + 3, 40, tb + 9, tb + 9]):
        ids = np.tile(np.array([v.sot, v.lang_id("en"), v.transcribe] + hist, np.int32), (nb, 1))
        logits = (rng.standard_normal((nb, V)) * 4.0).astype(np.float32)
        logits[:, tb:] += np.float32(rng.uniform(-6, 2))           # both outcomes of the timestamp rule occur
        streams = [stream_id(7 + b, 100 * b, b % 16) for b in range(nb)]
        seed = int(rng.integers(0, 2 ** 63))
        tok = eng.test_sample_seeded(logits, ids, 3, temp, seed, streams)
        for b in range(nb):
            results.append(R.check_token(spec, logits[b], list(ids[b]), 3, int(tok[b]), temp, seed, streams[b]))
    _tally(results)


@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("nb", [1, 5, 64])
@pytest.mark.parametrize("dt", DTYPES)
def test_decoded_tokens_are_the_float64_argmax(tiny, engines, dt, nb, temp):
    """A real sampled cw_decode under cw_set_logits_capture: every generated token from the logits of its own step."""
    g, v, W, spec = tiny
    eng = engines[dt]
    steps = 10
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    streams = [stream_id(b, 0, 3) for b in range(nb)]
    seed = 0x1234567890ABCDEF + nb
    eng.set_sampling(temp, seed, streams)
    cap = eng.capture_logits(nb, steps)
    try:
        seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + steps)
        cap = cap.copy()
    finally:
        eng.stop_capture()
        eng.set_sampling(0.0)
    results = []
    for b in range(nb):
        for k in range(int(lens[b]) - 3):
            ids = list(seqs[b, :3 + k])
            results.append(R.check_token(spec, cap[k, b], ids, 3, int(seqs[b, 3 + k]), temp, seed, streams[b]))
    assert len(results) >= nb
    _tally(results)


@pytest.mark.parametrize("force_ts", [False, True])
def test_draws_follow_the_softmax(tiny, engines, force_ts):
    """20 000 fixed seeds on one row whose processors leave 8 tokens to draw from (with the timestamp rule fired: 8 timestamps,
    the text tokens take no part): chi-square of the counts against the float64 softmax(s / T)."""
    g, v, W, spec = tiny
    eng = engines["f32"]
    tb, V, temp = spec.timestamp_begin, spec.vocab_size, 0.6
    logits = np.full((1, V), -np.inf, np.float32)
    free = [t for t in range(33, spec.eos_token_id) if t not in set(spec.suppress_tokens) | set(spec.begin_suppress_tokens)]
    if force_ts:
        toks = [tb + 20 + 3 * i for i in range(8)]
        logits[0, toks] = [2.0, 1.5, 1.0, 0.7, 0.3, 0.0, -0.4, -1.0]
        logits[0, free[:3]] = [1.9, 0.5, 0.2]                    # allowed text, below the timestamps' log-sum-exp
    else:
        toks = free[::len(free) // 8][:8]
        logits[0, toks] = [1.2, 0.8, 0.5, 0.1, 0.0, -0.3, -0.9, -1.5]
    ids = np.array([[v.sot, v.lang_id("en"), v.transcribe, tb + 3, free[5]]], np.int32)
    s, fired = R.processed_scores(spec, logits[0], list(ids[0]), 3)
    assert fired == force_ts and sorted(np.flatnonzero(np.isfinite(s))) == sorted(toks)
    z = s[toks] / temp
    prob = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
    n = 20000
    counts = np.zeros(8)
    idx = {t: i for i, t in enumerate(toks)}
    for seed in range(n):
        counts[idx[int(eng.test_sample_seeded(logits, ids, 3, temp, seed, [5])[0])]] += 1
    chi2 = float((((counts - n * prob) ** 2) / (n * prob)).sum())
    print("counts", counts.tolist(), "expected", (n * prob).round(1).tolist(), "chi2", chi2)
    assert chi2 < CHI2_7_1E6, (chi2, counts.tolist(), (n * prob).tolist())


def test_tokens_do_not_depend_on_the_batch_layout(tiny, engines):
    """The same 8 windows decoded at batch 8, batch 8 in shuffled order, batch 3 (+ 3 + 2) and batch 1: identical tokens per window."""
    g, v, W, spec = tiny
    eng = engines["f32"]
    clips = _clips(8)
    seed, temp = 99, 0.8

    def run(order):
        eng.mel([clips[w] for w in order])
        eng.encode(list(range(len(order))), [0] * len(order), [3000] * len(order))
        eng.set_sampling(temp, seed, [stream_id(w, 0, 1) for w in order])
        try:
            seqs, lens, _ = eng.decode(_prompt(v, len(order)), max_length=3 + 16)
        finally:
            eng.set_sampling(0.0)
        return {w: seqs[r, :lens[r]].tolist() for r, w in enumerate(order)}

    base = run(list(range(8)))
    assert len({tuple(s) for s in base.values()}) > 1
    for groups in ([[5, 2, 7, 0, 3, 6, 1, 4]], [[6, 1, 3], [0, 7, 4], [2, 5]], [[w] for w in (3, 0, 7, 1, 6, 2, 5, 4)]):
        got = {}
        for grp in groups:
            got.update(run(grp))
        assert got == base, groups
    # the draw is not the greedy choice, and another seed draws differently
    eng.mel(clips)
    eng.encode(list(range(8)), [0] * 8, [3000] * 8)
    greedy, glens, _ = eng.decode(_prompt(v, 8), max_length=3 + 16)
    assert any(greedy[w, :glens[w]].tolist() != base[w] for w in range(8))
    seed = 100
    assert run(list(range(8))) != base


@pytest.mark.parametrize("dt", DTYPES)
def test_temperature_zero_is_the_greedy_path_bit_for_bit(tiny, engines, dt):
    """Tokens, log-probability sums and alignment rows of a greedy decode before cw_set_sampling was ever called on a fresh
    context, after sampling was switched on and off again, and with temperature 0 set explicitly."""
    g, v, W, spec = tiny
    eng = Engine(spec, dtype=dt, max_batch=8)
    try:
        eng.load_state_dict(W)
        nb = 6
        eng.mel(_clips(nb))
        eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
        eng.set_thresholds(-1.0, None)

        def greedy():
            seqs, lens, _ = eng.decode(_prompt(v, nb), max_length=3 + 20)
            return seqs.copy(), lens.copy(), eng.avg_logprobs(nb).copy(), eng.alignment(nb, int(lens.max()) - 1).copy()

        first = greedy()
        eng.set_sampling(0.7, 3, [stream_id(b, 0, 2) for b in range(nb)])
        sampled, slens, _ = eng.decode(_prompt(v, nb), max_length=3 + 20)
        assert sampled.tolist() != first[0].tolist()
        eng.set_sampling(0.0, 3, [stream_id(b, 0, 2) for b in range(nb)])
        for again in (greedy(), (eng.set_sampling(0.0), greedy())[1]):
            for a, b in zip(first, again):
                assert a.tobytes() == b.tobytes()
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(Exception):
                eng.set_sampling(bad, 0, [0] * nb)
    finally:
        eng.close()


def test_masked_rows_keep_their_ids_and_logprob_sums(tiny, engines):
    g, v, W, spec = tiny
    eng = engines["f32"]
    nb = 4
    eng.mel(_clips(nb))
    eng.encode(list(range(nb)), [0] * nb, [3000] * nb)
    eng.set_thresholds(-1.0, None)
    try:
        seqs0, lens0, _ = eng.decode(_prompt(v, nb), max_length=3 + 16)
        alp0 = eng.avg_logprobs(nb).copy()
        streams = [stream_id(b, 0, 4) for b in range(nb)]
        eng.set_sampling(0.9, 11, streams)
        cap = eng.capture_logits(nb, 16)
        try:
            seqs1, lens1, _ = eng.decode(_prompt(v, nb), max_length=3 + 16, row_active=[1, 0, 1, 0])
            cap = cap.copy()
        finally:
            eng.stop_capture()
            eng.set_sampling(0.0)
        alp1 = eng.avg_logprobs(nb)
        for b in (1, 3):                                   # masked: as the decode before left them
            assert seqs1[b].tolist() == seqs0[b].tolist() and lens1[b] == 0
            assert alp1[b].tobytes() == alp0[b].tobytes()
        results = []
        for b in (0, 2):                                   # live: sampled, and their sums are those of the new tokens
            assert lens1[b] > 3
            for k in range(int(lens1[b]) - 3):
                results.append(R.check_token(spec, cap[k, b], list(seqs1[b, :3 + k]), 3, int(seqs1[b, 3 + k]), 0.9, 11, streams[b]))
            lp = []
            for k in range(int(lens1[b]) - 3):
                s, _ = R.processed_scores(spec, cap[k, b], list(seqs1[b, :3 + k]), 3)
                m = s.max()
                lp.append(s[seqs1[b, 3 + k]] - (m + np.log(np.exp(s - m).sum())))
            assert abs(float(alp1[b]) - float(np.mean(lp))) <= 1e-4 * max(1.0, abs(float(np.mean(lp)))), (alp1[b], np.mean(lp))
        _tally(results)
        assert seqs1[[0, 2]].tolist() != seqs0[[0, 2]].tolist()
        with pytest.raises(Exception):
            eng.decode(_prompt(v, nb), max_length=3 + 16, row_active=[0, 0, 0, 0])
        seqs2, lens2, _ = eng.decode(_prompt(v, nb), max_length=3 + 16)
        assert seqs2.tolist() == seqs0.tolist() and eng.avg_logprobs(nb).tobytes() == alp0.tobytes()
    finally:
        eng.set_thresholds(None, None)
