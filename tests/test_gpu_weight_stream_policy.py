"""GPU tests of the weight-stream policy of the <= 16-row decode GEMVs (csrc/gemm.hip: gemv2_bf16_kernel<.., WNT>, csrc/decfuse.hip:
gemv_stack_kernel<.., UNI, WNT>, csrc/declayer.hip: qkv_self_kernel<.., WNT>): packed weights that exactly one block of the launch reads
are streamed with non-temporal loads; CW_NO_WNT=1 (a context), option "no_wnt" (cw_set_option: a context; cw_test_set_option: the
cw_test_gemv_* hooks) select the default-policy instantiations.  A cache-policy bit changes no value, so everything a launch writes, and every sentinel it must leave alone, has to be identical bit for bit in both positions.  The K-split forms accumulate with f32
atomics whose order differs from run to run: exact operands (order-independent) are compared bit for bit, Gaussian ones against float64
within the bound of tests/decode_gemv_refs.py, under both settings, as tests/test_gpu_decode_gemv.py does.

Shapes: rows 1 / 5 / 8 (two rows per wave) and 9 / 16 (four); K = 128 and 1280 (one and three weight slots per wave; 5120 for fc2: the
K split (40, 5)); N with a last partial 16-column tile (N % 16 != 0) and an odd tile count where a block takes two tiles."""
import os

import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from tests import decode_gemv_refs as G
from tests import decode_stage_refs as R
from tests import helpers as Hh
from tests.test_gpu_decode_gemv import CAP, Options, check_gauss, launch
from tests.test_gpu_decode_stages import launch_stack

pytestmark = pytest.mark.gpu

ROWS = [1, 5, 8, 9, 16]
DT = "bf16"


@pytest.fixture(scope="module")
def eng():
    g, v, W, spec = Hh.tiny_setup()
    e = Engine(spec, dtype=DT, max_batch=64)
    yield e
    e.lib.cw_test_set_option(b"no_wnt", 0)
    e.close()


class Policy:
    """the hooks' weight-stream policy (cw_test_set_option "no_wnt"), restored on exit"""

    def __init__(self, e, no_wnt):
        self.e, self.v = e, no_wnt

    def __enter__(self):
        assert self.e.lib.cw_test_set_option(b"no_wnt", self.v) == 0

    def __exit__(self, *exc):
        self.e.lib.cw_test_set_option(b"no_wnt", 0)


def both(e, o, **kw):
    res = []
    for no_wnt in (0, 1):
        with Policy(e, no_wnt):
            res.append(launch(e, o, **kw))
    return res


def assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{what}: {k} differs between the two policies"


# ---- op 0, LayerNorm + GELU: the fc1 form -------------------------------------------------------------------------------------------------
# N = 4139: 259 tiles -> two tiles per block (130 blocks, the last with one tile, and that one partial); N = 283: one tile per block
@pytest.mark.parametrize("N", [283, 4139])
@pytest.mark.parametrize("K", [128, 1280])
@pytest.mark.parametrize("Mb", ROWS)
def test_fc1_form(eng, Mb, K, N):
    for epi in (1, 7):                                              # 16-bit rows for an x16 fc2, and f32 rows
        o = G.gemv_operands("gauss", DT, epi=epi, Mb=Mb, N=N, K=K, ldo=N + 5, wpk=1, ln="folded")
        a, b = both(eng, o)
        assert_same(a, b, f"fc1 epi={epi} Mb={Mb} K={K} N={N}")
        ref = G.gemv64(DT, o)
        G.assert_equal(a["out"][:, N:], ref["out"][:, N:], "columns N .. ldo")


# ---- the in-place K-split residual form: fc2 --------------------------------------------------------------------------------------------
# K, N, 16-bit input rows, slices of the bound (None: K / 128 at most).  2091: 131 tiles; 5120 x 1280: the engine's fc2, grid (40, 5), two
# tiles per block, behind a 16-bit and behind an f32 fc1
FC2 = [(128, 43, False, None), (1280, 2091, False, None), (5120, 1280, True, 5), (5120, 1280, False, 5)]


@pytest.mark.parametrize("K,N,x16,slices", FC2)
@pytest.mark.parametrize("Mb", ROWS)
def test_fc2_form(eng, Mb, K, N, x16, slices):
    ldo = N + 5 if N % 16 else N
    shape = dict(epi=2, Mb=Mb, N=N, K=K, ldo=ldo, wpk=1, inplace=True, x16=x16)
    o = G.gemv_operands("exact", DT, **shape)                       # order-independent sums: bit for bit
    a, b = both(eng, o)
    assert_same(a, b, f"fc2 exact Mb={Mb} K={K} N={N}")
    G.assert_equal(a["out"], G.gemv64(DT, o)["out"], "fc2 exact against float64")
    o = G.gemv_operands("gauss", DT, **shape)
    for no_wnt in (0, 1):
        with Policy(eng, no_wnt):
            check_gauss(DT, eng, o, f"fc2 gauss no_wnt={no_wnt} Mb={Mb} K={K} N={N}", slices=slices or max(K // 128, 1))


# ---- the q/k/v cache epilogue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [2, 20])
@pytest.mark.parametrize("Mb", ROWS)
def test_qkv_cache_form(eng, Mb, H):
    D = H * 64
    o = G.gemv_operands("gauss", DT, epi=6, Mb=Mb, N=3 * D, K=D, wpk=1, H=H, cap=CAP, ln="folded")
    a, b = both(eng, o)
    assert_same(a, b, f"qkv Mb={Mb} H={H}")                         # q, and both caches with every untouched row


# ---- gemv_stack_kernel ------------------------------------------------------------------------------------------------------------------
def stack_both(e, W, segs, Mb, K, nt):
    res = []
    for no_wnt in (0, 1):
        with Policy(e, no_wnt):
            args, zero, _ = launch_stack(e, W, segs, Mb, K, nt, True)
            res.append(args)
    return res


def assert_stack_same(a, b, what):
    for i, (sa, sb) in enumerate(zip(a, b)):
        for k in ("out", "out2", "pstats"):
            if sa.get(k) is not None:
                assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), f"{what}: segment {i} {k} differs between the two policies"


@pytest.mark.parametrize("Mb", ROWS)
def test_stack(eng, Mb):
    """the engine's X1 layout, K = 1280 (80 tiles per segment: the UNI form takes the policy) at one, two and three tiles per block
    (three: 27 blocks per segment, the last with two tiles), and K = 128 (never UNI: default-policy either way)"""
    W, segs = R.stack_gauss_case(DT, Mb)
    for nt in (1, 2, 3):
        a, b = stack_both(eng, W, segs, Mb, 1280, nt)
        assert_stack_same(a, b, f"stack K=1280 Mb={Mb} nt={nt}")
    W, segs, _ = R.stack_exact_case(128, R.STACK_K[128], "x1", rows=16)
    a, b = stack_both(eng, W, segs, Mb, 128, 2)
    assert_stack_same(a, b, f"stack K=128 Mb={Mb}")


# ---- launches that keep the default policy either way -----------------------------------------------------------------------------------
def test_default_policy_launches(eng):
    """Row groups (the combining out-projection's gridDim.z, gemv_stack_kernel's 16-row groups) and 17..64 rows (gemv_mt_kernel) re-read
    a weight tile by design and keep the default policy; row-major weights too.  The switch must leave them as they are."""
    for Mb in (8, 13):                                              # combining out-projection in row groups
        o = G.comb_operands("exact", DT, Mb=Mb, K=1280, H=20, N=1280)
        with Options(eng, comb_rowgroups=1):
            a, b = both(eng, o)
        assert_same(a, b, f"combine row groups Mb={Mb}")
    for Mb in (17, 40):
        W, segs = R.stack_gauss_case(DT, Mb)
        a, b = stack_both(eng, W, segs, Mb, 1280, 2)
        assert_stack_same(a, b, f"stack row groups Mb={Mb}")
        o = G.gemv_operands("gauss", DT, epi=5, Mb=Mb, N=272, K=1280, ldo=280, wpk=1, ln="folded")   # gemv_prep + gemv_mt
        a, b = both(eng, o)
        assert_same(a, b, f"mt Mb={Mb}")
        o = G.gemv_operands("exact", DT, epi=2, Mb=Mb, N=1280, K=5120, wpk=1, inplace=True)
        a, b = both(eng, o)
        assert_same(a, b, f"mt fc2 Mb={Mb}")
    for Mb in (8, 40):                                              # row-major weights: <= 16 rows, and groups of 16 (m_base > 0)
        o = G.gemv_operands("gauss", DT, epi=7, Mb=Mb, N=283, K=1280, ldo=288, wpk=0, ln="folded")
        a, b = both(eng, o)
        assert_same(a, b, f"row-major Mb={Mb}")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def run_engine(spec, W, v, env, rows, T, n_clip_seed):
    os.environ.update(env)
    try:
        e = Engine(spec, dtype=DT, max_batch=rows)
    finally:
        for k in env:
            os.environ.pop(k, None)
    try:
        e.load_state_dict(W)
        clips = [syn.synth_audio(n_clip_seed + i, 480000 - 20000 * i, ("noise", "chirp", "mixed")[i % 3]) for i in range(rows)]
        prompt = np.tile(np.array([[v.sot, v.lang_id("en"), v.transcribe]], np.int32), (rows, 1))
        out = []
        for call in range(2):                                       # the second call replays the captured step graph
            e.mel(clips)
            e.encode(list(range(rows)), [0] * rows, [3000] * rows)
            cap = e.capture_logits(rows, 12) if call == 0 else None
            seqs, lens, _ = e.decode(prompt, max_length=T, min_new_tokens=T - 3)
            if cap is not None:
                e.stop_capture()
            out.append((seqs[:, :T].copy(), None if cap is None else cap[:12].copy(), e.token_timestamps(rows, T - 1, 3, [3000] * rows).copy()))
        if not env:                                                 # the context's own option: off and on again, graphs dropped each time
            assert e.lib.cw_set_option(e.ctx, b"no_wnt", 1) == 0
            e.mel(clips)
            e.encode(list(range(rows)), [0] * rows, [3000] * rows)
            seqs, lens, _ = e.decode(prompt, max_length=T, min_new_tokens=T - 3)
            out.append((seqs[:, :T].copy(), None, e.token_timestamps(rows, T - 1, 3, [3000] * rows).copy()))
            assert e.lib.cw_set_option(e.ctx, b"no_wnt", 0) == 0
            e.mel(clips)
            e.encode(list(range(rows)), [0] * rows, [3000] * rows)
            seqs, lens, _ = e.decode(prompt, max_length=T, min_new_tokens=T - 3)
            out.append((seqs[:, :T].copy(), None, e.token_timestamps(rows, T - 1, 3, [3000] * rows).copy()))
        return out
    finally:
        e.close()


def compare_runs(a, b):
    for (sa, ca, ta), (sb, cb, tb) in zip(a, b):
        assert np.array_equal(sa, sb), int((sa != sb).sum())
        if ca is not None:
            assert np.array_equal(ca.view(np.uint32), cb.view(np.uint32))
        assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
    for s, _, t in a[2:]:                                           # option "no_wnt" = 1, then 0 again, on the first engine = its own earlier runs
        assert np.array_equal(s, a[1][0]) and np.array_equal(t, a[1][2])


@pytest.mark.parametrize("rows", [8, 12])
def test_end_to_end_tiny(rows):
    """two tiny-geometry engines in one process, one created under CW_NO_WNT=1: the same clips, greedy, 8 rows (qkv_self_kernel, fc1 /
    fc2 with two rows per wave) and 12 rows (the 9..16-row forms): identical sequences, token timestamps and captured logits"""
    g, v, W, spec = Hh.tiny_setup()
    T = 40
    compare_runs(run_engine(spec, W, v, {}, rows, T, 300), run_engine(spec, W, v, {"CW_NO_WNT": "1"}, rows, T, 300))


def test_end_to_end_wide():
    """the same at d_model = 1280 (two decoder layers), where the layer runs the three-slot instantiations and the UNI stack kernel"""
    g, v = syn.large_v3_geometry()
    g.enc_layers, g.dec_layers = 1, 2
    spec = syn.model_spec(g, v, n_align=4)
    spec.alignment_heads = [[1, 0], [1, 3], [1, 7], [1, 19]]
    W = syn.random_weights(g, seed=5)
    compare_runs(run_engine(spec, W, v, {}, 8, 24, 500), run_engine(spec, W, v, {"CW_NO_WNT": "1"}, 8, 24, 500))
