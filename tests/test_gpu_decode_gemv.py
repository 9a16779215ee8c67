"""GPU tests of the decode GEMV dispatcher (csrc/gemm.hip: cw_launch_gemv, cw_launch_rows_combine, cw_launch_gemv_own,
cw_launch_gemv_lna) as decode_step launches it, through cw_test_gemv_epi, each form against a float64 reference of its own operation
(tests/decode_gemv_refs.py; tests/test_decode_gemv_refs.py shows on the CPU that every comparison used here rejects a subtly wrong
kernel, that the exact operands are exact and that the case table reaches every branch of the launchers).

Exact operands: bit equality on everything the launch writes and the sentinel everywhere else (columns N .. ldo, every cache row but
pos[b], the statistics of rows >= Mb; the fragment-major pad rows and the guards behind every buffer are checked by the hook).
Gaussian operands: the derived per-element bounds of the reference module; the two measured yardsticks are printed by
test_yardsticks.  The cases follow decode_gemv_refs.case_table(), whose launcher coverage the CPU module proves (test_table_is_run)."""
import os

import numpy as np
import pytest

from crisperwhisper_amd.engine import Engine, EngineError
from tests import decode_gemv_refs as G
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16"]
F = np.float32
CAP = 24                    # cache rows of the epi 6 cases


@pytest.fixture(scope="module")
def engines():
    g, v, W, spec = Hh.tiny_setup()
    out = {dt: Engine(spec, dtype=dt, max_batch=64) for dt in DTS}
    out["f32"] = Engine(spec, dtype="f32", max_batch=2)
    yield out
    for e in out.values():
        e.close()


class Options:
    """process-wide launcher switches (cw_test_set_option), restored on exit"""
    DEFAULT = {"gemv_loop": 1, "comb_rowgroups": -1, "mt_variant": -1}

    def __init__(self, eng, **sw):
        self.eng, self.sw = eng, sw

    def __enter__(self):
        for k, v in self.sw.items():
            assert self.eng.lib.cw_test_set_option(k.encode(), v) == 0
        return self

    def __exit__(self, *exc):
        for k in self.sw:
            self.eng.lib.cw_test_set_option(k.encode(), self.DEFAULT[k])


def f32(a):
    return None if a is None else np.ascontiguousarray(a, F)


def launch(eng, o, frag_in=False):
    """one op 0 call on the operand dict o -> dict of the downloaded in / out buffers"""
    out = f32(o["out0"]).copy()
    kw = dict(op=0, epi=o["epi"], Mb=o["Mb"], N=o["N"], K=o["K"], ldo=o["ldo"], wpk=o["wpk"], x16=o["x16"], inplace=o["inplace"],
              frag_in=frag_in, W=o["W"], bias=o.get("bias"), out=out)
    if o.get("part_o") is not None:
        kw.update(part_o=o["part_o"], part_ml=o["part_ml"], H=o["H"])
    else:
        kw["x"] = o["x"]
    if o.get("ln") is not None:
        kw.update(ln_g=o["ln_g"], ln_b=o.get("ln_b"))
    if o["epi"] == 2 and not o["inplace"]:
        kw["resid"] = o["resid"]
    res = {"out": out}
    if o["epi"] == 6:
        res["sk"], res["sv"] = f32(o["sk0"]).copy(), f32(o["sv0"]).copy()
        kw.update(H=o["H"], cap=o["cap"], d_model=o["d_model"], pos=o["pos"], sk=res["sk"], sv=res["sv"])
    info = eng.test_gemv_epi(**kw)
    assert info["frag_tail_ok"], "the launch wrote into the pad rows of a fragment-major buffer"
    return res


def check_exact(dt, eng, o, what, frag_in=False):
    got = launch(eng, o, frag_in)
    ref = G.gemv64(dt, o)
    G.assert_equal(got["out"], ref["out"], what + " out")
    if o["epi"] == 6:
        assert np.abs(ref["acc"]).max() < 120, "the exact k / v rows must stay 8-bit numbers"
        G.assert_equal(got["sk"], ref["sk"], what + " k cache")
        G.assert_equal(got["sv"], ref["sv"], what + " v cache")
    return got


def check_gauss(dt, eng, o, what, slices=1, frag_in=False):
    """Gaussian operands within the derived bound; everything the launch does not write keeps the sentinel"""
    got = launch(eng, o, frag_in)
    ref = G.gemv64(dt, o)
    e_act = None
    if o.get("ln") is not None:
        e_act = G.ln_e_act(o["x"], o["ln_g"] if o["ln"] == "affine" else None, o.get("ln_b"))
    elif o.get("part_o") is not None:
        e_act = G.COMB_YARDSTICK * G.comb_unit(o["part_o"], o["part_ml"])
    b = G.out_bound(dt, o, ref, e_act, slices)
    N, epi = o["N"], o["epi"]
    if epi == 6:
        d, H, Mb = o["d_model"], o["H"], o["Mb"]
        G.assert_within(got["out"], ref["out"], b[:, :d], what + " q")
        for name, lo in (("sk", d), ("sv", 2 * d)):
            r, g_ = ref[name], got[name]
            written = np.zeros(r.shape, bool)
            written[np.arange(Mb), :, o["pos"]] = True
            G.assert_equal(g_[~written], r[~written], what + f" {name}: rows other than pos[b]")
            rr = r[np.arange(Mb), :, o["pos"]].reshape(Mb, d)
            G.assert_act16(dt, g_[np.arange(Mb), :, o["pos"]].reshape(Mb, d), rr, b[:, lo:lo + d], what + " " + name)
    elif epi in (1, 8):
        G.assert_act16(dt, got["out"][:, :N], ref["out"][:, :N], G.out_bound(dt, o, ref, e_act, slices, stored=False), what)
        G.assert_equal(got["out"][:, N:], ref["out"][:, N:], what + " columns N .. ldo")
    else:
        G.assert_within(got["out"][:, :N], ref["out"][:, :N], b, what)
        G.assert_equal(got["out"][:, N:], ref["out"][:, N:], what + " columns N .. ldo")
    return got


# ---- K-split residual form, <= 16 rows ------------------------------------------------------------------------------------------------
KSPLIT = [("ksplit N=16", dict(N=16, K=1024), None), ("ksplit NT2", dict(N=2080, K=1024), None),
          ("fc2", dict(N=1280, K=5120), 5), ("fc2 x16", dict(N=1280, K=5120, x16=True), 5),
          ("x16 N=48", dict(N=48, K=2560, x16=True), None), ("ksplit clamped", dict(N=43, K=1024, ldo=48), None)]


@pytest.mark.parametrize("name,shape,slices", KSPLIT, ids=[k[0].replace(" ", "_") for k in KSPLIT])
@pytest.mark.parametrize("wpk", [0, 1])
@pytest.mark.parametrize("dt", DTS)
def test_ksplit_residual(engines, dt, wpk, name, shape, slices):
    """gemv2_bf16_kernel ATOMIC (and its NT = 2 and X16 forms), row-major and packed weights.  Exact: every slice dense (no ties: the
    value is independent of the split), and x non-zero in slice 0 only with grid ties in both directions.  Gaussian: K / 128 slices
    at most, except fc2, whose grid (40, 5) is the launcher's documented rule."""
    K = shape["K"]
    for Mb in G.ROWS16:
        what = f"{name} {dt} wpk={wpk} Mb={Mb}"
        check_exact(dt, engines[dt], G.gemv_operands("exact", dt, epi=2, Mb=Mb, wpk=wpk, inplace=True, **shape), what + " exact dense")
        check_exact(dt, engines[dt], G.gemv_operands("exact", dt, epi=2, Mb=Mb, wpk=wpk, inplace=True, ties=True, head_only=True, **shape),
                    what + " exact ties")
        check_gauss(dt, engines[dt], G.gemv_operands("gauss", dt, epi=2, Mb=Mb, wpk=wpk, inplace=True, **shape), what + " gauss",
                    slices=slices or K // 128)


# ---- LayerNorm forms ------------------------------------------------------------------------------------------------------------------
LNF = [("LN NT2", 4112, 256, 1, {}), ("LN NT3 row-major", 16400, 128, 0, {}), ("LN NT3 row-major", 16411, 128, 0, {}),
       ("LN NT3 packed", 16400, 128, 1, {"gemv_loop": 0}), ("LN NT3 packed", 16411, 128, 1, {"gemv_loop": 0}),
       ("LN loop", 16400, 128, 1, {"gemv_loop": 1}), ("LN loop", 16411, 128, 1, {"gemv_loop": 1}),
       ("LN loop", 16400, 1280, 1, {"gemv_loop": 1}), ("LN loop", 16411, 1280, 1, {"gemv_loop": 1})]


@pytest.mark.parametrize("name,N,K,wpk,sw", LNF, ids=[f"{k[0].replace(' ', '_')}-{k[1]}-{k[2]}" for k in LNF])
@pytest.mark.parametrize("ln", ["affine", "folded"])
@pytest.mark.parametrize("dt", DTS)
def test_layernorm_forms(engines, dt, ln, name, N, K, wpk, sw):
    """the wide LayerNorm forms NT = 2 / NT = 3 (tail tile, clamped columns) and gemv_loop_kernel against float64; the loop must also
    equal the three-tile launch bit for bit"""
    eng = engines[dt]
    for Mb in (1, 8, 13):
        o = G.gemv_operands("gauss", dt, epi=5, Mb=Mb, N=N, K=K, ldo=N + 5, wpk=wpk, ln=ln)
        with Options(eng, **sw):
            got = check_gauss(dt, eng, o, f"{name} {dt} {ln} N={N} K={K} Mb={Mb}")
        if sw.get("gemv_loop") == 1:
            with Options(eng, gemv_loop=0):
                other = launch(eng, o)
            G.assert_equal(got["out"], other["out"], f"{name}: loop against three tiles per block")


# ---- epilogues at <= 16 rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mb", [5, 13])
@pytest.mark.parametrize("dt", DTS)
def test_epilogues(engines, dt, Mb):
    """epi 1 (16-bit row-major GELU), 5, 7 behind a folded LayerNorm, and epi 2 with a separate residual, ldo > N"""
    for epi in (1, 5, 7):
        for wpk in (0, 1):
            for K in (128, 640):                                 # (at K = 128 the bound is narrower than the distance to the tanh form of GELU)
                o = G.gemv_operands("gauss", dt, epi=epi, Mb=Mb, N=272, K=K, ldo=280, wpk=wpk, ln="folded")
                check_gauss(dt, engines[dt], o, f"epi {epi} {dt} wpk={wpk} Mb={Mb} K={K}")
    for wpk in (0, 1):
        check_exact(dt, engines[dt], G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=272, K=640, ldo=280, wpk=wpk, ties=True),
                    f"epi 2 separate resid exact {dt} wpk={wpk} Mb={Mb}")
        check_gauss(dt, engines[dt], G.gemv_operands("gauss", dt, epi=2, Mb=Mb, N=272, K=640, ldo=280, wpk=wpk),
                    f"epi 2 separate resid {dt} wpk={wpk} Mb={Mb}")
        check_exact(dt, engines[dt], G.gemv_operands("exact", dt, epi=5, Mb=Mb, N=272, K=640, ldo=280, wpk=wpk),
                    f"epi 5 exact {dt} wpk={wpk} Mb={Mb}")


@pytest.mark.parametrize("H", [2, 20])
@pytest.mark.parametrize("Mb", [5, 13])
@pytest.mark.parametrize("dt", DTS)
def test_qkv_cache(engines, dt, Mb, H):
    """EPI_QKV_CACHE: q as f32, k / v appended at pos[b] (distinct per row, 0 and cap - 1 included; the row is requested at kernel
    entry); every other cache row keeps the sentinel"""
    D = H * 64
    for wpk in (0, 1):
        check_exact(dt, engines[dt], G.gemv_operands("exact", dt, epi=6, Mb=Mb, N=3 * D, K=D, wpk=wpk, H=H, cap=CAP),
                    f"qkv exact {dt} wpk={wpk} Mb={Mb} H={H}")
    check_gauss(dt, engines[dt], G.gemv_operands("gauss", dt, epi=6, Mb=Mb, N=3 * D, K=D, wpk=1, H=H, cap=CAP, ln="folded"),
                f"qkv folded {dt} Mb={Mb} H={H}")
    check_gauss(dt, engines[dt], G.gemv_operands("gauss", dt, epi=6, Mb=Mb, N=3 * D, K=D, wpk=0, H=H, cap=CAP, ln="affine"),
                f"qkv affine row-major {dt} Mb={Mb} H={H}")


# ---- activation readout: W = I -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mb", [5, 13, 40])
@pytest.mark.parametrize("wpk", [0, 1])
@pytest.mark.parametrize("ln", ["affine", "folded"])
@pytest.mark.parametrize("dt", DTS)
def test_layernorm_readout(engines, dt, ln, wpk, Mb):
    """With W = I an epi 5 launch returns a16 exactly: the LayerNorm stage of gemv2 (<= 8 / 9..16 rows), of the groups of 16 (row-major,
    40 rows) and of gemv_prep_kernel (packed, 40 rows) against round16(LN64(x)), apart from the accumulation"""
    for K in (256, 1280):
        o = G.gemv_operands("gauss", dt, epi=5, Mb=Mb, N=K, K=K, wpk=wpk, ln=ln, identity=True)
        got = launch(engines[dt], o)["out"]
        act = G.activation64(dt, o)
        e = G.ln_e_act(o["x"], o["ln_g"] if ln == "affine" else None, o.get("ln_b"))
        what = f"LN readout {dt} {ln} wpk={wpk} Mb={Mb} K={K}"
        G.assert_act16(dt, got, act, e, what)
        G.assert_fold16_where_derived(dt, got, act, e, what)


# ---- combine ----------------------------------------------------------------------------------------------------------------------------
COMB = [("combine rowgroups", 1280, 1280, 20, [2, 8, 12, 13, 16]), ("combine G=6", 640, 1280, 20, [13, 16]),
        ("combine one row per group", 64, 1024, 16, [3, 8])]


def comb_case(dt, eng, N, K, H, Mb, what):
    """exact and Gaussian partials through the row-group grid and through the plain (N / 16, ksplit) grid: both equal to the
    reference, and to each other bit for bit"""
    for kind in ("exact", "gauss"):
        o = G.comb_operands(kind, dt, Mb=Mb, K=K, H=H, N=N)
        res = []
        for on in (1, 0):
            with Options(eng, comb_rowgroups=on):
                res.append((check_exact if kind == "exact" else check_gauss)(dt, eng, o, f"{what} {kind} rowgroups={on}",
                                                                             **({} if kind == "exact" else {"slices": K // 128})))
        G.assert_equal(res[0]["out"], res[1]["out"], what + f" {kind}: row groups against the plain grid")


@pytest.mark.parametrize("name,N,K,H,rows", COMB, ids=[k[0].replace(" ", "_") for k in COMB])
@pytest.mark.parametrize("dt", DTS)
def test_combine(engines, dt, name, N, K, H, rows):
    for Mb in rows:
        comb_case(dt, engines[dt], N, K, H, Mb, f"{name} {dt} Mb={Mb}")


@pytest.mark.parametrize("Mb", [2, 8, 13, 16])
@pytest.mark.parametrize("dt", DTS)
def test_combine_readout(engines, dt, Mb):
    """W = I, in place: out - resid = grid12(a16) = a16 (|a| in [1, 8): the 16-bit spacing is coarser than the grid), the combined
    rows of the <= 16-row kernels against round16(combine64) within the measured yardstick"""
    o = G.comb_operands("gauss", dt, Mb=Mb, K=1280, H=20, readout=True)
    got = launch(engines[dt], o)["out"].astype(np.float64) - o["out0"]
    act = G.combine64(o["part_o"], o["part_ml"])
    assert np.abs(act).min() >= 1 and np.abs(act).max() < 8
    G.assert_act16(dt, got, act, G.COMB_YARDSTICK * G.comb_unit(o["part_o"], o["part_ml"]), f"combine readout {dt} Mb={Mb}")


@pytest.mark.parametrize("dt", DTS)
def test_combine_nt2(request, engines, dt):
    """CW_COMB_NT2=1 (two column tiles per block over 256-wide K slices; read from the environment once per process: a child
    process)"""
    if not os.environ.get("CW_COMB_NT2"):
        return Hh.run_in_child(request, {"CW_COMB_NT2": "1"}, lambda p: True)
    for Mb in (8, 13):
        for kind in ("exact", "gauss"):
            o = G.comb_operands(kind, dt, Mb=Mb, K=1280, H=20)
            (check_exact if kind == "exact" else check_gauss)(dt, engines[dt], o, f"comb NT2 {kind} {dt} Mb={Mb}",
                                                              **({} if kind == "exact" else {"slices": 5}))


# ---- 17..64 rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mb", G.ROWS64)
@pytest.mark.parametrize("dt", DTS)
def test_rows64_packed(engines, dt, Mb):
    """gemv_prep_kernel + gemv_mt_kernel: MT 2 / 3 / 4, NSLOT 1 / 2 / 3, ATOMIC, the cache epilogue, the fragment-major GELU rows, the
    producer form x == null and the combine"""
    eng = engines[dt]
    for K in (512, 1024, 1280):
        check_gauss(dt, eng, G.gemv_operands("gauss", dt, epi=5, Mb=Mb, N=272, K=K, ldo=280, ln="folded", wpk=1), f"mt store {dt} Mb={Mb} K={K}")
        check_exact(dt, eng, G.gemv_operands("exact", dt, epi=5, Mb=Mb, N=272, K=K, ldo=280, wpk=1), f"mt store exact {dt} Mb={Mb} K={K}")
    for N, K in ((16, 1024), (1280, 5120)):
        what = f"mt ksplit {dt} Mb={Mb} N={N} K={K}"
        check_exact(dt, eng, G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=N, K=K, wpk=1, inplace=True), what + " exact dense")
        check_exact(dt, eng, G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=N, K=K, wpk=1, inplace=True, ties=True, head_only=True), what + " exact ties")
        check_gauss(dt, eng, G.gemv_operands("gauss", dt, epi=2, Mb=Mb, N=N, K=K, wpk=1, inplace=True), what, slices=K // 128)
    o = G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=1280, K=5120, wpk=1, inplace=True)
    a = check_exact(dt, eng, o, f"mt frag_in exact {dt} Mb={Mb}", frag_in=True)
    o = G.gemv_operands("gauss", dt, epi=2, Mb=Mb, N=1280, K=5120, wpk=1, inplace=True)
    a, b = check_gauss(dt, eng, o, f"mt frag_in {dt} Mb={Mb}", slices=40, frag_in=True), launch(eng, o)
    G.assert_equal(a["out"], b["out"], "the producer form against the preparation launch")
    check_exact(dt, eng, G.gemv_operands("exact", dt, epi=6, Mb=Mb, N=384, K=128, wpk=1, H=2, cap=CAP), f"mt qkv exact {dt} Mb={Mb}")
    check_gauss(dt, eng, G.gemv_operands("gauss", dt, epi=6, Mb=Mb, N=384, K=128, wpk=1, H=2, cap=CAP, ln="affine"), f"mt qkv {dt} Mb={Mb}")
    check_gauss(dt, eng, G.gemv_operands("gauss", dt, epi=8, Mb=Mb, N=512, K=128, wpk=1, ln="folded"), f"mt gelu frag {dt} Mb={Mb}")
    for kind in ("exact", "gauss"):
        o = G.comb_operands(kind, dt, Mb=Mb, K=1280, H=20)
        (check_exact if kind == "exact" else check_gauss)(dt, eng, o, f"mt combine {kind} {dt} Mb={Mb}",
                                                          **({} if kind == "exact" else {"slices": 10}))


@pytest.mark.parametrize("Mb", G.ROWS64)
@pytest.mark.parametrize("dt", DTS)
def test_rows64_variants(engines, dt, Mb):
    """mt_variant -1 / 0 / 1 / 2 (one tile per block, two row groups, two row groups x two column tiles): equal bits, and the reference"""
    eng = engines[dt]
    for spec in (dict(epi=5, N=288, K=256, ln="affine"), dict(epi=2, N=1280, K=1280, inplace=True), dict(epi=6, N=384, K=128, H=2, cap=CAP, ln="folded")):
        o = G.gemv_operands("gauss", dt, Mb=Mb, wpk=1, **spec)
        res = []
        for var in (-1, 0, 1, 2):
            with Options(eng, mt_variant=var):
                res.append(check_gauss(dt, eng, o, f"mt_variant {var} {dt} Mb={Mb} epi={spec['epi']}", slices=spec["K"] // 128))
        for r in res[1:]:
            for k in res[0]:
                G.assert_equal(r[k], res[0][k], f"mt_variant: {k} differs between block shapes")


@pytest.mark.parametrize("Mb", [17, 40, 64])
@pytest.mark.parametrize("dt", DTS)
def test_rows64_rowmajor(engines, dt, Mb):
    """row-major weights at 17..64 rows: groups of 16 on gemv2_bf16_kernel with m_base > 0 -- the split residual form, the cache
    epilogue (row_pos[m_base + ...]) and GELU"""
    eng = engines[dt]
    check_exact(dt, eng, G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=16, K=1024, wpk=0, inplace=True), f"groups ksplit exact {dt} Mb={Mb}")
    check_exact(dt, eng, G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=16, K=1024, wpk=0, inplace=True, ties=True, head_only=True),
                f"groups ksplit ties {dt} Mb={Mb}")
    check_gauss(dt, eng, G.gemv_operands("gauss", dt, epi=2, Mb=Mb, N=16, K=1024, wpk=0, inplace=True), f"groups ksplit {dt} Mb={Mb}", slices=8)
    check_exact(dt, eng, G.gemv_operands("exact", dt, epi=6, Mb=Mb, N=384, K=128, wpk=0, H=2, cap=CAP), f"groups qkv exact {dt} Mb={Mb}")
    check_gauss(dt, eng, G.gemv_operands("gauss", dt, epi=6, Mb=Mb, N=384, K=128, wpk=0, H=2, cap=CAP, ln="folded"), f"groups qkv {dt} Mb={Mb}")
    check_gauss(dt, eng, G.gemv_operands("gauss", dt, epi=7, Mb=Mb, N=272, K=640, wpk=0, ln="folded"), f"groups gelu {dt} Mb={Mb}")


# ---- the 33..64-row chain pieces -------------------------------------------------------------------------------------------------------
def rows_combine(eng, o, pstats=None, n_pstats=0):
    out = f32(o["out0"]).copy()
    cvec = None if pstats is None else np.full(o["Mb"], G.SENTINEL, F)
    info = eng.test_gemv_epi(op=1, Mb=o["Mb"], N=o["K"], K=o["K"], H=o["H"], part_o=o["part_o"], part_ml=o["part_ml"],
                             pstats=pstats, n_pstats=n_pstats, out=out, cvec=cvec)
    assert info["frag_tail_ok"]
    return out, cvec


@pytest.mark.parametrize("n_pstats", [1, 40, 80])
@pytest.mark.parametrize("dt", DTS)
def test_rows_combine(engines, dt, n_pstats):
    """cw_launch_rows_combine: the partials -> 16-bit fragment-major rows, and cvec from the planes"""
    for Mb in (17, 40, 64):
        for H in (2, 20):
            K = H * 64
            ps = G.pstats_operands(Mb, K, n_pstats)
            o = G.comb_operands("exact", dt, Mb=Mb, K=K, H=H, op=1)
            out, cvec = rows_combine(engines[dt], o, ps, n_pstats)
            what = f"rows_combine {dt} Mb={Mb} H={H} n_pstats={n_pstats}"
            G.assert_equal(out, G.combine64(o["part_o"], o["part_ml"]), what + " exact")
            c = G.cvec64(ps, n_pstats, Mb, K)
            G.assert_within(cvec, c, G.U32 * np.abs(c), what + " cvec")
            o = G.comb_operands("gauss", dt, Mb=Mb, K=K, H=H, op=1)
            out, _ = rows_combine(engines[dt], o)
            G.assert_act16(dt, out, G.combine64(o["part_o"], o["part_ml"]), G.COMB_YARDSTICK * G.comb_unit(o["part_o"], o["part_ml"]), what)


def own(eng, o):
    out, y = f32(o["out0"]).copy(), np.full((o["Mb"], o["N"]), G.SENTINEL, F)
    stats = np.full((o["N"] // 16, 64, 2), G.SENTINEL, F)       # sized for nt = 1; nt = 2 uses the first half
    info = eng.test_gemv_epi(op=2, Mb=o["Mb"], N=o["N"], K=o["K"], wpk=1, x=o["x"], W=o["W"], bias=o["bias"], cvec_in=o["cvec"], out=out,
                             y=y, stats=stats)
    assert info["frag_tail_ok"] and info["nt"] in (1, 2)
    return out, y, stats[:o["N"] // (16 * info["nt"])], info["nt"]


@pytest.mark.parametrize("D", [128, 1280])
@pytest.mark.parametrize("Mb", [17, 33, 64])
@pytest.mark.parametrize("dt", DTS)
def test_gemv_own(engines, dt, Mb, D):
    """gemv_mt_kernel OWN: the new residual, the centred 16-bit rows y = x_new - c and the per-block (sum y, sum y^2)"""
    for kind in ("exact", "gauss"):
        o = G.own_operands(kind, dt, Mb=Mb, N=D, K=D)
        out, y, stats, nt = own(engines[dt], o)
        ref = G.own64(dt, o, nt)
        what = f"own {kind} {dt} Mb={Mb} D={D} nt={nt}"
        if kind == "exact":
            G.assert_equal(out, ref["out"], what + " out")
            G.assert_equal(y, ref["y"], what + " y")
            G.assert_equal(stats, ref["stats"], what + " stats")
        else:
            b_out, b_y, b_st = G.own_bounds(dt, o, ref, nt)
            G.assert_within(out, ref["out"], b_out, what + " out")
            G.assert_act16(dt, y, ref["y_f32"], b_y, what + " y")
            G.assert_equal(stats[:, Mb:], ref["stats"][:, Mb:], what + " stats of rows >= Mb")
            G.assert_within(stats[:, :Mb], ref["stats"][:, :Mb], b_st[:, :Mb], what + " stats")


def lna(eng, o):
    out = f32(o["out0"]).copy()
    info = eng.test_gemv_epi(op=3, Mb=o["Mb"], N=o["N"], K=o["K"], wpk=1, x=o["x"], W=o["W"], bias=o["bias"], stats_in=o["stats_in"],
                             n_stats=o["n_stats"], wsum=o["wsum"], out=out)
    assert info["frag_tail_ok"]
    return out


LNA = [(64, 128, 8), (5120, 1280, 80), (64, 1280, 96)]


@pytest.mark.parametrize("N,K,n_stats", LNA)
@pytest.mark.parametrize("Mb", [33, 48, 64])
@pytest.mark.parametrize("dt", DTS)
def test_gemv_lna(engines, dt, Mb, N, K, n_stats):
    """gemv_mt_kernel LNA: the LayerNorm applied on the accumulator from the partial sums.  |mean_y| <= 0.5 sigma, as the column-owning
    stage in front guarantees (y = x_new - c with c the row's mean one stage earlier)."""
    o = G.lna_operands(dt, Mb=Mb, N=N, K=K, n_stats=n_stats)
    ref = G.lna64(dt, o)
    assert (np.abs(ref["mean"]) <= 0.51 * np.sqrt(ref["var"])).all()
    got = lna(engines[dt], o)
    G.assert_act16(dt, got, ref["out"], G.lna_bound(dt, o, ref), f"lna {dt} Mb={Mb} N={N} K={K} n_stats={n_stats}")


def test_yardsticks(engines, capsys):
    """Prints the two measured yardsticks (module docstring of the reference module) and asserts that the recorded measurements are
    not exceeded by more than the 4 x margin's half: a kernel change that doubles the error shows here first."""
    worst_c = worst_l = 0.0
    for dt in DTS:
        for Mb, H in ((17, 2), (40, 16), (64, 20)):
            o = G.comb_operands("gauss", dt, Mb=Mb, K=H * 64, H=H, op=1)
            out, _ = rows_combine(engines[dt], o)
            need = G.needed_err16(dt, out, G.combine64(o["part_o"], o["part_ml"]))
            worst_c = max(worst_c, float((need / G.comb_unit(o["part_o"], o["part_ml"])).max()))
        for Mb in (33, 48, 64):
            for N, K, n_stats in LNA:
                o = G.lna_operands(dt, Mb=Mb, N=N, K=K, n_stats=n_stats)
                ref = G.lna64(dt, o)
                need = G.needed_err16(dt, lna(engines[dt], o), ref["out"])
                derived = G.gelu_bound(ref["v"], G.lna_derived_bound(dt, o, ref))
                worst_l = max(worst_l, float((np.maximum(need - derived, 0) / (1.13 * (n_stats + 2) * G.lna_unit(ref) + 1e-300)).max()))
    with capsys.disabled():
        print(f"\nyardsticks: combine {worst_c:.3f} comb_unit (recorded {G.COMB_MEASURED}), LNA {worst_l:.3f} lna_unit beyond the derived bound "
              f"(recorded {G.LNA_MEASURED})")
    assert worst_c <= 2 * G.COMB_MEASURED and worst_l <= 2 * G.LNA_MEASURED


# ---- f32 engine -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mb,N,K", [(3, 200, 256), (8, 128, 128)])
def test_f32_engine(engines, Mb, N, K):
    """gemv_f32_kernel's other epilogues within 1e-6 of the largest reference element; epi 6 at N = 192 = 3 d_model, the nearest
    column count the epilogue takes"""
    eng = engines["f32"]
    for epi in (2, 5, 7):
        for inplace in ((False, True) if epi == 2 else (False,)):
            o = G.gemv_operands("gauss", "f32", epi=epi, Mb=Mb, N=N, K=K, ldo=N + 3, wpk=0, inplace=inplace)
            got, ref = launch(eng, o), G.gemv64("f32", o)
            G.assert_within(got["out"][:, :N], ref["out"][:, :N], 1e-6 * np.abs(ref["out"][:, :N]).max(), f"f32 epi {epi}")
            G.assert_equal(got["out"][:, N:], ref["out"][:, N:], f"f32 epi {epi} columns N .. ldo")
    o = G.gemv_operands("gauss", "f32", epi=6, Mb=Mb, N=192, K=K, wpk=0, H=1, cap=CAP)
    got, ref = launch(eng, o), G.gemv64("f32", o)
    for k in ("out", "sk", "sv"):
        m = ref[k] != G.SENTINEL
        G.assert_equal(got[k][~m], ref[k][~m], f"f32 epi 6 {k} untouched")
        G.assert_within(got[k][m], ref[k][m], 1e-6 * np.abs(ref[k][m]).max(), f"f32 epi 6 {k}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_refusals(engines, dt):
    """every CW_ERR_INVALID path of the hook and of the launchers behind it; nothing is launched"""
    e = engines[dt]
    z = lambda *s: np.zeros(s, F)
    base = dict(op=0, epi=5, Mb=4, N=32, K=128, W=z(32, 128), x=z(4, 128), out=z(4, 32))

    def refused(match, eng=e, **kw):
        a = dict(base)
        a.update(kw)
        with pytest.raises(EngineError, match=match):
            eng.test_gemv_epi(**a)
    refused("op 7", op=7)
    refused("epi 3", epi=3)
    refused("size < 1", Mb=0)
    refused("size < 1", N=0)
    refused("Mb=65 > 64", Mb=65, x=z(65, 128), out=z(65, 32))
    refused("multiple of 128", K=192, W=z(32, 192), x=z(4, 192))
    refused("multiple of 128", K=5248, W=z(32, 5248), x=z(4, 5248))
    refused("N=70000", N=70000)
    refused("null buffer W", W=None)
    refused("null buffer x", x=None)
    refused("null buffer out", out=None)
    refused("ldo=16 < N=32", ldo=16)
    refused("ln_b without ln_g", ln_b=z(128))
    refused("inplace / resid with epi 5", inplace=True)
    refused("null buffer resid", epi=2)
    refused("inplace with a separate resid", epi=2, inplace=True, resid=z(4, 32))
    refused("part_o and part_ml", epi=2, inplace=True, part_o=z(6, 4, 128))
    refused("H \\* 64 != K", epi=2, inplace=True, part_o=z(6, 4, 128), part_ml=z(4, 3, 6, 2), H=3)
    refused("in front of a LayerNorm", epi=2, inplace=True, part_o=z(6, 4, 128), part_ml=z(4, 2, 6, 2), H=2, ln_g=z(128))
    refused("frag_in with a combine", epi=2, inplace=True, part_o=z(6, 4, 128), part_ml=z(4, 2, 6, 2), H=2, frag_in=True)
    refused("epi 8 takes ldo == N", epi=8, Mb=20, x=z(20, 128), out=z(20, 32), ldo=40)
    q = dict(epi=6, N=384, W=z(384, 128), out=z(4, 128), H=2, cap=8, d_model=128, pos=[0, 1, 2, 3], sk=z(4, 2, 8, 64), sv=z(4, 2, 8, 64))
    refused("d_model=100", **dict(q, d_model=100))
    refused("N=384 != 3 d_model", **dict(q, d_model=64, H=1))
    refused("H \\* 64 != d_model", **dict(q, H=3))
    refused("cap=0", **dict(q, cap=0))
    refused("epi 6 takes pos, sk and sv", **dict(q, pos=None))
    refused("pos\\[2\\]=8 outside", **dict(q, pos=[0, 1, 8, 3]))
    refused("pos\\[1\\]=-1 outside", **dict(q, pos=[0, -1, 2, 3]))
    # what the launchers refuse, reported as their refusal
    refused("launch rejected", x16=True)                                         # 16-bit rows: the K-split residual form only
    refused("launch rejected", frag_in=True)                                     # the producer form at <= 16 rows
    refused("launch rejected", frag_in=True, Mb=20, x=z(20, 128), out=z(20, 32), wpk=0)   # ... and without packed weights
    refused("launch rejected", epi=1, Mb=20, x=z(20, 128), out=z(20, 32))        # 16-bit row-major GELU beyond 16 rows
    refused("launch rejected", epi=8)                                            # fragment-major GELU at <= 16 rows
    refused("launch rejected", epi=5, part_o=z(6, 4, 128), part_ml=z(4, 2, 6, 2), H=2)   # a combine with another epilogue
    refused("launch rejected", epi=5, K=2560, W=z(32, 2560), x=z(4, 2560), wpk=1)        # K > 1280 without the in-place split, packed
    # op 1 .. 3
    c = dict(op=1, Mb=20, N=128, K=128, H=2, part_o=z(6, 20, 128), part_ml=z(20, 2, 6, 2), out=z(20, 128), x=None)
    refused("part_o and part_ml", **dict(c, part_ml=None))
    refused("H \\* 64 != K", **dict(c, H=1))
    refused("n_pstats in 1 .. 256", **dict(c, pstats=z(2, 300, 16, 2), n_pstats=300, cvec=z(20)))
    refused("n_pstats in 1 .. 256", **dict(c, pstats=z(2, 4, 16, 2), n_pstats=4))
    w = dict(op=2, Mb=20, N=128, K=128, wpk=1, W=z(128, 128), x=z(20, 128), out=z(20, 128), cvec_in=z(20), y=z(20, 128), stats=z(8, 64, 2))
    refused("op 2 takes x, cvec_in, y and stats", **dict(w, y=None))
    refused("launch rejected", **dict(w, Mb=16, x=z(16, 128), out=z(16, 128), cvec_in=z(16), y=z(16, 128)))
    refused("launch rejected", **dict(w, wpk=0))
    refused("launch rejected", **dict(w, N=48, W=z(48, 128), out=z(20, 48), y=z(20, 48), stats=z(3, 64, 2)))
    refused("launch rejected", **dict(w, K=1664, W=z(128, 1664), x=z(20, 1664)))
    n = dict(op=3, Mb=40, N=64, K=128, wpk=1, W=z(64, 128), x=z(40, 128), out=z(40, 64), stats_in=z(8, 64, 2), n_stats=8, wsum=z(64))
    refused("op 3 takes x, stats_in and wsum", **dict(n, wsum=None))
    refused("n_stats=0 < 1", **dict(n, n_stats=0))
    refused("launch rejected", **dict(n, n_stats=97, stats_in=z(97, 64, 2)))
    refused("launch rejected", **dict(n, Mb=32, x=z(32, 128), out=z(32, 64)))
    refused("launch rejected", **dict(n, wpk=0))
    # the f32 engine
    f = engines["f32"]
    for kw in (dict(epi=1), dict(wpk=1), dict(ln_g=z(128)), dict(op=3), dict(x16=True), dict(epi=2, inplace=True, part_o=z(6, 4, 128), part_ml=z(4, 2, 6, 2), H=2)):
        refused("the f32 engine takes", eng=f, **kw)


def test_table_is_run():
    """every case of the table that the coverage proof (tests/test_decode_gemv_refs.py) stands on is launched by a test above"""
    names = {name for name, _, _ in G.case_table()}
    declared = {"ksplit N=16", "ksplit NT2", "fc2", "fc2 x16", "x16 N=48", "ksplit clamped", "LN NT2", "LN NT3 row-major", "LN NT3 packed",
                "LN loop", "epilogue", "separate resid", "qkv cache", "qkv cache exact", "combine rowgroups", "combine plain grid",
                "combine G=6", "combine one row per group", "combine NT2", "mt store", "mt ksplit N=16", "mt fc2", "mt fc2 frag_in", "mt qkv",
                "mt gelu frag", "mt combine", "mt variants", "row-major groups ksplit", "row-major groups qkv", "row-major groups gelu",
                "rows_combine cvec", "own", "lna", "lna limit"}
    assert names == declared, (names ^ declared)
