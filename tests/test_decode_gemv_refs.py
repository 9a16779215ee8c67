"""CPU proofs of tests/decode_gemv_refs.py (no GPU): every comparison tests/test_gpu_decode_gemv.py makes rejects each planted fault
at each shape family it is used on; the exact operands are exact in two f32 summation orders and in both 16-bit types; the derived
activation bound holds an f32 restatement of the kernel's LayerNorm in two orders; the reference inputs stay under the cap on excused
elements; and the case table reaches every branch of the launchers that decode_step reaches."""
import numpy as np
import pytest

from tests import decode_gemv_refs as G

DTS = ["bf16", "f16"]
CAP = 24


def rejected(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


# ---- the comparisons of op 0 -----------------------------------------------------------------------------------------------------------
def exact_families(dt):
    """(name, operands, faults that must show)"""
    W_FAULTS = ["w_kslice_shift", "packed_as_rowmajor"]
    for Mb in (5, 13):
        yield ("ksplit dense", G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=48, K=1024, wpk=1, inplace=True),
               W_FAULTS + ["bias_every_slice", "bias_none"])
        yield ("ksplit ties", G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=48, K=1024, wpk=1, inplace=True, ties=True, head_only=True),
               W_FAULTS + ["bias_every_slice", "bias_none", "grid_after_resid"])
        yield ("separate resid", G.gemv_operands("exact", dt, epi=2, Mb=Mb, N=272, K=640, ldo=280, wpk=1, ties=True),
               W_FAULTS + ["bias_none", "grid_after_resid"])
        yield ("store", G.gemv_operands("exact", dt, epi=5, Mb=Mb, N=272, K=640, ldo=280, wpk=1), W_FAULTS + ["bias_none"])
    for Mb in (5, 13, 40):
        yield ("qkv", G.gemv_operands("exact", dt, epi=6, Mb=Mb, N=384, K=128, wpk=1, H=2, cap=CAP),
               W_FAULTS + ["pos_last_row", "pos_plus_one", "qkv_swapped"])
    for Mb in (2, 13, 40):
        yield ("combine", G.comb_operands("exact", dt, Mb=Mb, K=1280, H=20),
               W_FAULTS + ["ml_next_head", "ml_next_row_last_group", "plane_group_stride", "bias_none"])


def exact_check(dt, o, out):
    ref = G.gemv64(dt, o)
    G.assert_equal(out["out"], ref["out"])
    if o["epi"] == 6:
        G.assert_equal(out["sk"], ref["sk"])
        G.assert_equal(out["sv"], ref["sv"])


@pytest.mark.parametrize("dt", DTS)
def test_exact_comparison_rejects_every_fault(dt):
    for name, o, faults in exact_families(dt):
        exact_check(dt, o, G.gemv64(dt, o))                       # the reference passes its own comparison
        for f in faults:
            slices = 2 if f == "bias_every_slice" else 1
            assert rejected(exact_check, dt, o, G.gemv64(dt, o, fault=f, slices=slices)), (name, o["Mb"], f)


def gauss_families(dt):
    W_FAULTS = ["w_kslice_shift", "packed_as_rowmajor"]
    # rows rounded before centring: in f16 the fault moves a normalised element of a 40-spreads-offset row by 2^-12 40 = 0.01, which the
    # readout comparison rejects (test_readout_comparison_rejects_every_fault), but summed over K in quadrature it stays inside the
    # worst-case flip allowance of those rows (e_act ~ one f16 spacing, summed linearly); bf16 rounds eight times coarser
    LN_FAULTS = ["no_eps"] + (["round_before_centring"] if dt == "bf16" else [])
    for Mb in (5, 13):
        yield ("ksplit", G.gemv_operands("gauss", dt, epi=2, Mb=Mb, N=48, K=1024, wpk=1, inplace=True), 8, W_FAULTS + ["bias_every_slice", "bias_none"])
        yield ("LN store", G.gemv_operands("gauss", dt, epi=5, Mb=Mb, N=272, K=256, wpk=1, ln="affine"), 1, W_FAULTS + LN_FAULTS)
        yield ("LN store", G.gemv_operands("gauss", dt, epi=5, Mb=Mb, N=272, K=1280, wpk=1, ln="folded"), 1, W_FAULTS + LN_FAULTS)
        for epi in (1, 7):
            # (K = 128: at K = 640 the worst-case accumulation bound 2 K u sum |a w| is wider than the 4.7e-4 between the two GELU forms)
            yield ("gelu", G.gemv_operands("gauss", dt, epi=epi, Mb=Mb, N=272, K=128, wpk=1, ln="folded"), 1, W_FAULTS + ["gelu_tanh", "no_eps"])
            yield ("gelu", G.gemv_operands("gauss", dt, epi=epi, Mb=Mb, N=272, K=640, wpk=1, ln="folded"), 1, W_FAULTS + ["no_eps"])
        yield ("qkv", G.gemv_operands("gauss", dt, epi=6, Mb=Mb, N=384, K=128, wpk=1, H=2, cap=CAP, ln="folded"), 1,
               W_FAULTS + ["pos_last_row", "pos_plus_one", "qkv_swapped", "no_eps"])
        yield ("combine", G.comb_operands("gauss", dt, Mb=Mb, K=1280, H=20), 10,
               W_FAULTS + ["ml_next_head", "ml_next_row_last_group", "plane_group_stride"])
    yield ("gelu frag", G.gemv_operands("gauss", dt, epi=8, Mb=40, N=512, K=128, wpk=1, ln="folded"), 1, W_FAULTS + ["gelu_tanh", "no_eps"])
    yield ("combine", G.comb_operands("gauss", dt, Mb=40, K=1280, H=20), 10, W_FAULTS + ["ml_next_head", "ml_next_row_last_group"])


def gauss_check(dt, o, out, slices):
    """the comparisons of test_gpu_decode_gemv.check_gauss on a dict of outputs"""
    ref = G.gemv64(dt, o)
    e_act = None
    if o.get("ln") is not None:
        e_act = G.ln_e_act(o["x"], o["ln_g"] if o["ln"] == "affine" else None, o.get("ln_b"))
    elif o.get("part_o") is not None:
        e_act = G.COMB_YARDSTICK * G.comb_unit(o["part_o"], o["part_ml"])
    b = G.out_bound(dt, o, ref, e_act, slices)
    N, epi = o["N"], o["epi"]
    if epi == 6:
        d, Mb = o["d_model"], o["Mb"]
        G.assert_within(out["out"], ref["out"], b[:, :d])
        for name, lo in (("sk", d), ("sv", 2 * d)):
            written = np.zeros(ref[name].shape, bool)
            written[np.arange(Mb), :, o["pos"]] = True
            G.assert_equal(out[name][~written], ref[name][~written])
            G.assert_act16(dt, G.round16(dt, out[name][np.arange(Mb), :, o["pos"]].reshape(Mb, d)),
                           ref[name][np.arange(Mb), :, o["pos"]].reshape(Mb, d), b[:, lo:lo + d])
    elif epi in (1, 8):
        G.assert_act16(dt, G.round16(dt, out["out"][:, :N]), ref["out"][:, :N], G.out_bound(dt, o, ref, e_act, slices, stored=False))
    else:
        G.assert_within(out["out"][:, :N], ref["out"][:, :N], b)


@pytest.mark.parametrize("dt", DTS)
def test_gauss_comparison_rejects_every_fault(dt):
    for name, o, slices, faults in gauss_families(dt):
        gauss_check(dt, o, G.gemv64(dt, o), slices)
        for f in faults:
            assert rejected(gauss_check, dt, o, G.gemv64(dt, o, fault=f, slices=2 if f == "bias_every_slice" else 1), slices), (name, o["Mb"], f)


@pytest.mark.parametrize("dt", DTS)
def test_readout_comparison_rejects_every_fault(dt):
    """W = I: the LayerNorm readout (assert_act16 + assert_fold16) and the combine readout"""
    for ln in ("affine", "folded"):
        for Mb, K in ((5, 256), (13, 1280), (40, 256)):
            o = G.gemv_operands("gauss", dt, epi=5, Mb=Mb, N=K, K=K, wpk=1, ln=ln, identity=True)
            act = G.activation64(dt, o)
            e = G.ln_e_act(o["x"], o["ln_g"] if ln == "affine" else None, o.get("ln_b"))

            def check(got):
                G.assert_act16(dt, got, act, e)
                G.assert_fold16_where_derived(dt, got, act, e)
            check(G.gemv64(dt, o)["out"])
            for f in ("no_eps", "round_before_centring", "w_kslice_shift", "packed_as_rowmajor"):
                assert rejected(check, G.gemv64(dt, o, fault=f)["out"]), (ln, Mb, K, f)
            if ln == "folded":                                   # gamma used although folded
                assert rejected(check, G.round16(dt, act * 7.0))
    for Mb in (2, 13):
        o = G.comb_operands("gauss", dt, Mb=Mb, K=1280, H=20, readout=True)
        act = G.combine64(o["part_o"], o["part_ml"])
        e = G.COMB_YARDSTICK * G.comb_unit(o["part_o"], o["part_ml"])
        G.assert_act16(dt, G.gemv64(dt, o)["out"] - o["out0"], act, e)
        for f in ("ml_next_head", "ml_next_row_last_group", "plane_group_stride"):
            assert rejected(G.assert_act16, dt, G.gemv64(dt, o, fault=f)["out"] - o["out0"], act, e), (Mb, f)
        # one position off in a handful of elements that are nowhere near a boundary
        got = G.round16(dt, act)
        far = np.argwhere(G.boundary_distance16(dt, act) > 10 * e)[:3]
        for i in far:
            got[tuple(i)] += G.ulp16(dt, got[tuple(i)])
        assert rejected(G.assert_act16, dt, got, act, e)


# ---- the chain pieces ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_rows_combine_comparison(dt):
    for Mb, H in ((17, 2), (40, 20)):
        K = H * 64
        o = G.comb_operands("exact", dt, Mb=Mb, K=K, H=H, op=1)
        ref = G.combine64(o["part_o"], o["part_ml"])
        assert np.array_equal(G.round16(dt, ref), ref), "the exact combination is a 16-bit number"
        for f in ("ml_next_head", "ml_next_row_last_group", "plane_group_stride"):
            assert rejected(G.assert_equal, G.combine64(o["part_o"], o["part_ml"], f), ref), (Mb, H, f)
        o = G.comb_operands("gauss", dt, Mb=Mb, K=K, H=H, op=1)
        ref, e = G.combine64(o["part_o"], o["part_ml"]), G.COMB_YARDSTICK * G.comb_unit(o["part_o"], o["part_ml"])
        G.assert_act16(dt, G.round16(dt, ref), ref, e)
        for f in ("ml_next_head", "ml_next_row_last_group", "plane_group_stride"):
            assert rejected(G.assert_act16, dt, G.round16(dt, G.combine64(o["part_o"], o["part_ml"], f)), ref, e), (Mb, H, f)
        for n_pstats in (1, 40, 80):
            ps = G.pstats_operands(Mb, K, n_pstats)
            c = G.cvec64(ps, n_pstats, Mb, K)
            assert np.isfinite(c).all()
            s = np.nan_to_num(ps.astype(np.float32))[..., 0]      # the sums are exact in f32 in both orders
            for order in (1, -1):
                tot = np.cumsum(s[:, ::order], axis=1, dtype=np.float32)[:, -1]
                m = np.arange(Mb)
                assert np.array_equal(tot[m >> 4, m & 15].astype(np.float64) / K, c)
            for f in (["cvec_short"] if n_pstats > 1 else []) + ["cvec_squares"]:
                assert rejected(G.assert_within, G.cvec64(ps, n_pstats, Mb, K, f), c, G.U32 * np.abs(c)), (n_pstats, f)


OWN_FAULTS = ["w_kslice_shift", "packed_as_rowmajor", "bias_none", "grid_after_resid", "y_about_new_mean", "stats_slot_next_block"]


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_own_comparison_rejects_every_fault(dt, nt):
    for Mb, D in ((17, 128), (33, 1280), (64, 128)):
        o = G.own_operands("exact", dt, Mb=Mb, N=D, K=D)
        ref = G.own64(dt, o, nt)
        assert np.array_equal(ref["y"], ref["y_f32"]) and np.array_equal(G.round16(dt, o["x"]), o["x"])
        assert np.abs(ref["y"]).max() < 128 and np.array_equal(ref["y"] * 2, np.rint(ref["y"] * 2)), "y: a few halves"
        for f in OWN_FAULTS:
            bad = G.own64(dt, o, nt, f)
            assert any(rejected(G.assert_equal, bad[k], ref[k]) for k in ("out", "y", "stats")), (Mb, D, f)
        o = G.own_operands("gauss", dt, Mb=Mb, N=D, K=D)
        ref = G.own64(dt, o, nt)
        b_out, b_y, b_st = G.own_bounds(dt, o, ref, nt)

        def check(r):
            G.assert_within(r["out"], ref["out"], b_out)
            G.assert_act16(dt, r["y"], ref["y_f32"], b_y)
            G.assert_equal(r["stats"][:, Mb:], ref["stats"][:, Mb:])
            G.assert_within(r["stats"][:, :Mb], ref["stats"][:, :Mb], b_st[:, :Mb])
        check(ref)
        for f in OWN_FAULTS:
            if f == "grid_after_resid":                          # within a grid step of the reference: an exact-operand fault
                continue
            assert rejected(check, G.own64(dt, o, nt, f)), (Mb, D, f)


@pytest.mark.parametrize("dt", DTS)
def test_lna_comparison_rejects_every_fault(dt):
    for Mb, N, K, n_stats in ((33, 64, 128, 8), (48, 640, 1280, 80), (64, 64, 1280, 96)):
        o = G.lna_operands(dt, Mb=Mb, N=N, K=K, n_stats=n_stats)
        ref = G.lna64(dt, o)
        assert (np.abs(ref["mean"]) <= 0.51 * np.sqrt(ref["var"])).all(), "|mean_y| <= 0.5 sigma"
        b = G.lna_bound(dt, o, ref)
        G.assert_act16(dt, G.round16(dt, ref["out"]), ref["out"], b)
        # the statistics the kernel sums are those of the row: the f32 slot sums, added in either order, within the derived bound
        st = np.asarray(o["stats_in"], np.float32)[:, :Mb]
        for order in (1, -1):
            s = np.cumsum(st[::order], axis=0, dtype=np.float32)[-1].astype(np.float64)
            assert np.allclose(s[:, 0] / K, ref["mean"], rtol=0, atol=(n_stats + 2) * G.U32 * np.abs(o["x"]).mean(-1))
            assert np.allclose(s[:, 1] / K, ref["ex2"], rtol=(n_stats + 2) * G.U32, atol=0)
        for f in ("w_kslice_shift", "packed_as_rowmajor", "lna_mean_short", "wsum_unrounded", "gelu_tanh", "no_eps"):
            if f == "no_eps" and ref["var"].min() > 1e-3:
                continue
            if f in ("wsum_unrounded", "gelu_tanh") and K > 128:
                # both move an output by ~1e-3 at most (sum_k (w - w16) mean_y rstd; 4.7e-4 between the GELU forms): inside the
                # worst-case accumulation bound 2 K u sum |y w| at K = 1280, outside it at K = 128
                continue
            assert rejected(G.assert_act16, dt, G.round16(dt, G.lna64(dt, o, f)["out"]), ref["out"], b), (Mb, N, K, f)


# ---- exactness ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_exact_operands_are_exact(dt):
    """two f32 summation orders (and two slice counts of the in-place form) give the float64 value bit for bit; operands and 16-bit
    results are numbers of both 16-bit types"""
    cases = [G.gemv_operands("exact", dt, epi=2, Mb=16, N=48, K=5120, wpk=1, inplace=True),
             G.gemv_operands("exact", dt, epi=2, Mb=16, N=48, K=1024, wpk=1, inplace=True, ties=True, head_only=True),
             G.gemv_operands("exact", dt, epi=2, Mb=13, N=272, K=640, ldo=280, ties=True),
             G.gemv_operands("exact", dt, epi=5, Mb=64, N=272, K=1280)]
    for o in cases:
        for other in DTS:
            assert np.array_equal(G.round16(other, o["x"]), o["x"]) and np.array_equal(G.round16(other, o["W"]), o["W"])
        ref = G.gemv64(dt, o)["out"][:, :o["N"]]
        for order in (0, 1):
            for slices in ((1, 4) if o["epi"] == 2 and o["inplace"] else (1,)):
                assert np.array_equal(G.f32_gemv_restatement(dt, o, order, slices), ref), (o["epi"], o["K"], order, slices)
        if o["epi"] == 2 and o["inplace"]:                       # ... and the float64 value does not depend on the split either
            for slices in (2, 5, 8):
                assert np.array_equal(G.gemv64(dt, o, slices=slices)["out"][:, :o["N"]], ref)
    ties = cases[1]
    t = (ties["bias"] * 8192) % 2 == 1
    assert t.any() and (~t).any()
    up = np.asarray(ties["bias"])[t] * 8192 % 4
    assert {1.0, 3.0} <= set(up.tolist()), "ties in both directions"
    for H, Mb in ((2, 13), (20, 13), (2, 64)):
        o = G.gemv_operands("exact", dt, epi=6, Mb=Mb, N=3 * H * 64, K=H * 64, wpk=1, H=H, cap=CAP)
        ref = G.gemv64(dt, o)
        assert len(set(o["pos"].tolist())) == min(Mb, CAP) and {0, CAP - 1} <= set(o["pos"].tolist())
        for other in DTS:
            for k in ("sk", "sv"):
                assert np.array_equal(G.round16(other, ref[k]), ref[k]), "the exact k / v rows are 16-bit numbers"
    for Mb in (2, 13, 40):
        o = G.comb_operands("exact", dt, Mb=Mb, K=1280, H=20)
        w, l = G.comb_weights(o["part_ml"])
        L = (w * l).sum(-1)
        assert (w == 1).all() and np.array_equal(np.log2(L), np.rint(np.log2(L))), "e^0 and a power-of-two L"
        assert (L[:, :-1] != L[:, 1:]).all() and (Mb == 1 or (L[:-1] != L[1:]).all()), "L differs between neighbouring heads and rows"
        a = G.combine64(o["part_o"], o["part_ml"])
        po32 = o["part_o"].astype(np.float32)
        for order in (1, -1):                                    # the f32 sum over the splits in both orders, times 1 / L
            s = np.cumsum(po32[::order], axis=0, dtype=np.float32)[-1].astype(np.float64)
            assert np.array_equal(s.reshape(Mb, 20, 64) / L[..., None], a.reshape(Mb, 20, 64))
        assert np.array_equal(a * 4, np.rint(a * 4)) and np.abs(a).max() <= 3


# ---- the derived activation bound --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_layernorm_bound_holds_the_f32_restatement(dt):
    """an f32 evaluation of the kernel's statistics in two summation orders stays inside e_act; the reference inputs stay under the
    cap on the share of elements a comparison may excuse"""
    for ln in ("affine", "folded"):
        for Mb, K in ((13, 128), (13, 256), (40, 1280)):
            o = G.gemv_operands("gauss", dt, epi=5, Mb=Mb, N=16, K=K, ln=ln)
            g, b = (o["ln_g"], o["ln_b"]) if ln == "affine" else (None, None)
            act = G.ln64(o["x"], g, b)
            e = G.ln_e_act(o["x"], g, b)
            for order in (0, 1):
                err = np.abs(G.ln_f32_restatement(o["x"], g, b, order) - act)
                assert (err <= e).all(), (ln, Mb, K, order, float((err / e).max()))
            plain = ~G.centred_rows(Mb)
            plain[0] = False
            assert G.near_share(dt, act[plain], e[plain]) <= 1.25 * G.flip_share_cap(dt, act[plain], e[plain]) + 0.01


def test_needed_err16():
    for dt in DTS:
        x = np.asarray([1.0, 1.0, -2.0, 0.0, 0.3])
        u = G.ulp16(dt, x)
        assert np.array_equal(G.needed_err16(dt, G.round16(dt, x), x), np.zeros(5))
        up = G.round16(dt, x) + np.where(x >= 0, 1, -1) * u       # one position away from zero
        need = G.needed_err16(dt, up, x)
        assert np.allclose(need[:3], 0.5 * u[:3], rtol=1e-12) and (need[3:] > 0).all()
        below_one = 1.0 - G.ulp16(dt, 0.75)                      # the neighbour below a power of two is half a spacing closer
        assert np.isclose(G.needed_err16(dt, below_one, 1.0), 0.5 * G.ulp16(dt, 0.75))


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_launcher_branch():
    got = G.table_branches()
    assert G.REQUIRED_BRANCHES <= got, sorted(G.REQUIRED_BRANCHES - got)


def test_launcher_restatement_spot_checks():
    """the documented grids of csrc/gemm.hip: fc2 (40, 5) with two column tiles per block; the out-projection's row groups"""
    fc2 = dict(op=0, epi=2, Mb=8, N=1280, K=5120, wpk=1, inplace=True)
    assert {"gemv2.ATOMIC", "gemv2.NSLOT3"} <= G.launcher_branches(fc2)
    comb = dict(op=0, epi=2, Mb=8, N=1280, K=1280, wpk=1, inplace=True, part_o=True)
    assert {"gemv2.COMBINE.rowgroups.RPW1", "gemv2.COMBINE.G3"} <= G.launcher_branches(comb)
    assert "gemv2.COMBINE.(N/16,ksplit)" in G.launcher_branches(comb, comb_rowgroups=0)
    assert {"gemv2.COMBINE.rowgroups.RPW2", "gemv2.COMBINE.G3"} <= G.launcher_branches(dict(comb, Mb=16))
    logits = dict(op=0, epi=5, Mb=8, N=51866, K=1280, wpk=1, ln="affine", inplace=False)
    assert "gemv_loop" in G.launcher_branches(logits) and "gemv2.LN.NT3" in G.launcher_branches(logits, gemv_loop=0)
