"""GPU parity tests of the log-mel front end (csrc/mel.hip) against plain numpy float64 (tests/mel_refs.py), stage by stage and in
the form the encoder reads: the raw log spectrum from before the clip floor (d_logspec), the clip maximum as the ordered-uint
atomicMax leaves it (d_gmax), the HF-layout f32 features, and the time-major copy in the engine's activation type that conv1
consumes (d_feats_tm), read back through cw_test_mel_stages.  Both kernels (mel_mfma_kernel by default, mel_kernel under the
test option "mel_valu"), the f32 / bf16 / f16 engines at 128 mels and a bf16 engine at 80 mels (the mel stage alone runs there).

Cases (mel_refs.CASES, four to a batch): silence, unit impulses at the clip's first sample, at 5119 and at its last sample, DC, tones
on bin 100, on bin 200 and between bins at full scale, quiet noise (negative clip maximum), loud noise, and a length ladder around
the hop, the half window, the window, the 32-frame block and the clip's end (0 .. 480000 samples).

Tolerance (mel_refs.TOL; derived on the CPU, not from the kernels): the float64 reference and its emulation with the kernels' three
f32 roundings differ by at most 1.27e-6 over every case; the bar is four times that, 5.08e-6, on the raw log spectrum and the clip
maximum and a quarter of it, 1.27e-6, on the features.  Measured on MI355X (CW_TEST_ERRLOG=<file> records every figure), the same
for both kernels: raw 1.84e-6 (loud noise), clip maximum 1.28e-6, feats_hf 4.1e-7 ("Front end")."""
import dataclasses
import os

import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine, EngineError
from tests import helpers as Hh
from tests import mel_refs as R

pytestmark = pytest.mark.gpu

ENGINES = {"f32": ("f32", 128), "bf16": ("bf16", 128), "f16": ("f16", 128), "bf16_80mels": ("bf16", 80)}
KERNELS = ("mfma", "valu")
BATCHES = [R.CASE_NAMES[i:i + 4] for i in range(0, len(R.CASE_NAMES), 4)]
LADDER_NAMES = tuple(f"len_{n}" for n in R.LADDER)
OTHER_NAMES = tuple(n for n in R.CASE_NAMES if n not in LADDER_NAMES)


def _log(what, e):
    log = os.environ.get("CW_TEST_ERRLOG")                       # tolerance audit: CW_TEST_ERRLOG=<file> records every measured error
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}\t{what}\t{e:.3e}\n")
    return e


def _new_engine(ekey):
    dt, n_mels = ENGINES[ekey]
    g, v, _, _ = Hh.tiny_setup()
    return Engine(syn.model_spec(dataclasses.replace(g, n_mels=n_mels), v, 3), dtype=dt, max_batch=4)


@pytest.fixture(scope="module")
def engines():
    out = {k: _new_engine(k) for k in ENGINES}
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(scope="module", params=[(e, k) for e in ENGINES for k in KERNELS], ids=lambda p: "%s-%s" % p)
def mode(request, engines):
    """(engine key, kernel, engine) with the kernel selected for the process; the environment's choice comes back afterwards"""
    ekey, kernel = request.param
    eng = engines[ekey]
    assert eng.lib.cw_test_set_option(b"mel_valu", 1 if kernel == "valu" else 0) == 0
    yield ekey, kernel, eng
    eng.lib.cw_test_set_option(b"mel_valu", -1)


def _mel(eng, clips):
    """one cw_mel over the clips -> per clip (raw [3000][n_mels], gmax, feats_hf [n_mels][3000], feats_tm [3000][n_mels], n_frames)"""
    feats, nf = eng.mel(list(clips), return_features=True)
    raw, gmax, tm = eng.test_mel_stages(len(clips))
    return [(raw[i], gmax[i], feats[i], tm[i], int(nf[i])) for i in range(len(clips))]


@pytest.fixture(scope="module")
def run(mode):
    """every case through the engine once, four to a batch, in table order (so a slot sees loud, quiet, long and short clips in turn)"""
    ekey, kernel, eng = mode
    got = {}
    for names in BATCHES:
        for name, r in zip(names, _mel(eng, [R.clip(n) for n in names])):
            got[name] = r
    return got


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(a, b):
    """two results of _mel for one clip agree bit for bit in every stage, and in n_frames"""
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def _check_raw_and_feats(mode, run, names):
    ekey, kernel, eng = mode
    n_mels = ENGINES[ekey][1]
    worst_raw = worst_feats = 0.0
    for name in names:
        raw, gmax, hf, tm, nf = run[name]
        ref_raw, ref_cmax, ref_feats = R.case_reference(name, n_mels)
        assert raw.shape == ref_raw.shape and hf.shape == ref_feats.T.shape
        e_raw = float(np.abs(raw - ref_raw).max())
        e_feats = float(np.abs(hf.T - ref_feats).max())
        print(f"{ekey} {kernel} {name}: raw {e_raw:.3e} (bar {R.TOL:.3e})  feats_hf {e_feats:.3e} (bar {R.TOL_FEATS:.3e})")
        worst_raw, worst_feats = max(worst_raw, e_raw), max(worst_feats, e_feats)
        assert e_raw < R.TOL, (ekey, kernel, name, "raw", e_raw)
        assert e_feats < R.TOL_FEATS, (ekey, kernel, name, "feats_hf", e_feats)
    _log("raw", worst_raw)
    _log("feats_hf", worst_feats)


def test_raw_and_features_against_float64(mode, run):
    """the full raw tensor (before the max - 8 floor: the deep bins of the folded DFT count) and feats_hf, every case but the ladder"""
    _check_raw_and_feats(mode, run, OTHER_NAMES)


def test_length_ladder(mode, run):
    """n_frames = ceil(n / 160), raw and features at every length: the reflected left edge, the zero padding behind the clip, the
    reflected right edge (frame 2999 reads 40 samples past the clip), the dead frames of the last block"""
    for n in R.LADDER:
        assert run[f"len_{n}"][4] == (n + 159) // 160, n
    _check_raw_and_feats(mode, run, LADDER_NAMES)


def test_too_long_a_clip_is_refused(engines):
    with pytest.raises(EngineError):
        engines["f32"].mel([np.zeros(480001, np.float32)], return_features=True)
    with pytest.raises(EngineError):
        engines["f32"].mel([np.zeros(10, np.float32), np.zeros(480001, np.float32)])


def test_80_mels_run_the_mel_stage_and_the_encoder_is_refused_by_name(engines):
    """conv1's implicit GEMM needs n_mels % 64 == 0: at 80 its weight and cw_encode are refused with a message, never run"""
    eng = engines["bf16_80mels"]
    with pytest.raises(EngineError, match="multiple of 64"):
        eng.load_tensor("model.encoder.conv1.weight", np.zeros((eng.spec.d_model, 80, 3), np.float32))
    with pytest.raises(EngineError, match="multiple of 64"):
        eng.encode([0], [0], [3000])


def test_clip_maximum(mode, run):
    """The decoded maximum is the maximum of the kernel's own raw tensor bit for bit and within the bar of the reference's; silence
    (and the empty clip) are exactly -10 / -1.5: the negative branch of the ordered encoding; quiet clips have negative maxima."""
    ekey, kernel, eng = mode
    n_mels = ENGINES[ekey][1]
    worst = 0.0
    for name in R.CASE_NAMES:
        raw, gmax, hf, tm, nf = run[name]
        assert np.float32(gmax).view(np.uint32) == raw.max().view(np.uint32), (name, float(gmax), float(raw.max()))
        e = abs(float(gmax) - R.case_reference(name, n_mels)[1])
        worst = max(worst, e)
        assert e < R.TOL, (name, float(gmax), e)
    _log("gmax", worst)
    for name in ("silence", "len_0"):
        raw, gmax, hf, tm, nf = run[name]
        assert float(gmax) == -10.0 and np.all(raw == -10.0), (name, float(gmax), float(raw.min()), float(raw.max()))
        assert np.all(hf == -1.5) and np.all(tm == -1.5), name
    for name in ("quiet_noise", "impulse_479999", "impulse_0", "len_1"):
        assert float(run[name][1]) < 0.0, (name, float(run[name][1]))
    assert -7.2 < float(run["quiet_noise"][1]) < -6.4 and -3.7 < float(run["impulse_479999"][1]) < -3.2
    assert float(run["loud_noise"][1]) > 10.0


def test_feats_tm_is_what_conv1_should_read(mode, run):
    """d_feats_tm, the buffer conv1 gathers from: on the f32 engine feats_hf transposed, exactly; on the 16-bit engines the engine's
    own feats_hf rounded by the engine's rule (nearest even), exactly, and the reference rounded to the type to one unit in the last
    place (mel_refs.tm16_violations).  Frames differ from each other and channels differ from each other in the noise cases."""
    ekey, kernel, eng = mode
    dt, n_mels = ENGINES[ekey]
    for name in R.CASE_NAMES:
        raw, gmax, hf, tm, nf = run[name]
        want = np.ascontiguousarray(hf.T)
        if dt == "f32":
            assert np.array_equal(tm.view(np.uint32), want.view(np.uint32)), (name, float(np.abs(tm - want).max()))
        else:
            assert np.array_equal(tm, R.round16(dt, want)), (name, float(np.abs(tm - R.round16(dt, want)).max()))
            bad = R.tm16_violations(dt, tm, R.case_reference(name, n_mels)[2])
            assert bad == 0, (name, bad)
    x = run["len_480000"][3]                                  # a transposition cannot pass: neither axis is constant
    assert np.all(x.std(axis=0) > 0.01) and np.all(x.std(axis=1) > 0.01)


def test_batch_position(mode, run):
    """the same clip in slot 0 and in slot 3, next to other clips than in the table run: identical bits everywhere"""
    ekey, kernel, eng = mode
    for name, others in (("len_479999", ("silence", "loud_noise")), ("quiet_noise", ("dc", "len_161"))):
        c = R.clip(name)
        r = _mel(eng, [c, R.clip(others[0]), R.clip(others[1]), c])
        assert _same(r[0], r[3]), name
        assert _same(r[0], run[name]), name


def test_no_stale_state_in_a_batch_slot(mode):
    """loud noise, then quiet noise through slot 0; a 480000-sample clip, then a 201-sample one: the second results are those of a
    fresh engine, bit for bit (the clip maximum is reset, the samples behind a short clip are zeroed)"""
    ekey, kernel, _ = mode
    a, b = _new_engine(ekey), _new_engine(ekey)
    try:
        fresh_quiet = _mel(a, [R.clip("quiet_noise")])[0]
        fresh_short = _mel(b, [R.clip("len_201")])[0]
        _mel(a, [R.clip("loud_noise")])
        assert _same(_mel(a, [R.clip("quiet_noise")])[0], fresh_quiet)
        _mel(a, [R.clip("len_480000")])
        assert _same(_mel(a, [R.clip("len_201")])[0], fresh_short)
        _mel(b, [R.clip("loud_noise"), R.clip("len_480000")])
        r = _mel(b, [R.clip("len_201"), R.clip("quiet_noise")])
        assert _same(r[0], fresh_short)
        assert _same(r[1], fresh_quiet)
    finally:
        a.close()
        b.close()
