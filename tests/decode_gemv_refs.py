"""Float64 / numpy references, input builders, bounds and the case table of the decode GEMV dispatcher tests
(tests/test_gpu_decode_gemv.py): cw_launch_gemv, cw_launch_rows_combine, cw_launch_gemv_own and cw_launch_gemv_lna of csrc/gemm.hip as
decode_step launches them, through the hook cw_test_gemv_epi.  Kept apart from the GPU module so that tests/test_decode_gemv_refs.py
can show on a CPU-only machine that every comparison rejects a subtly wrong kernel (the `fault` arguments plant one), that the exact
operands are exact, and that the case table reaches every branch of the launchers.

The references restate the documented operation on the operands the kernel multiplies, not its instruction order:

    a16 = round16(act),  act = x | LN(x) (affine, or folded: no gamma / beta) | combine(part_o, part_ml)
    acc = a16 round16(W)^T
    epi 2   out = resid + grid12(acc + bias);  with K slices  resid + sum_s grid12(acc_s + [s = 0] bias)
    epi 5   out = acc + bias            epi 7 / 1 / 8   gelu(acc + bias)  (f32 / 16-bit row-major / 16-bit fragment-major)
    epi 6   v = acc + bias:  q = v[:, :d],  k / v rows appended to the caches at row pos[b]

Exact operands: x in {-1, 0, 1}, W in {-1, -1/2, 0, 1/2, 1}, bias in halves: every term is a multiple of 1/2 and sum |terms| <= K
<= 5120 -- exact in f32 in any order, and a result below 128 has at most 8 significant bits, a number of bf16 and of f16.  With the
in-place K-split form every slice's partial sum is already on the 2^-12 grid, so the expected value does not depend on the split.  Grid
ties (acc + bias at odd multiples of 2^-13, both directions) are planted through the bias where the launch has one K slice, or where x
is non-zero only in its first 128 columns (slice 0 of every split: the other slices add grid12(0) = 0).

Derived bounds of the Gaussian comparisons (per output element; u = 2^-24)
  * f32 accumulation: 2 K u sum |a16 w16| (the form of decode_stage_refs.stack_elem_bound), final additions 2 u |result|.
  * the 2^-12 grid: 2^-13 per K slice that contributes, and 2^-13 for the reference, which rounds the whole sum once.  The slice
    count is K / 128 at most (a slice holds at least one 128-column step); the case table says where the launcher's documented
    rule fixes it (fc2 at <= 16 rows: K = 5120, N = 1280 -> grid (40, 5), five slices).
  * 16-bit flips of the activation.  The kernel's f32 LayerNorm value differs from the float64 one by at most e_act; an element
    whose float64 value lies farther than e_act from every 16-bit rounding boundary rounds to the same number, any other may land
    floor(e_act / ulp16) + 1 positions off and adds that many |w16| ulp16 to the output's bound (flip_allowance).
    e_act of the LayerNorm, from the kernel's operation count: the sum of K terms in any order errs by (K - 1) u sum |x|, the
    division by K by one more rounding: d_mu = K u mean|x|.  Every centred value d = x - mu carries d_mu + u |d|.  The K squares and
    their sum: relative (K + 2) u on sum d^2, plus 2 d_mu sum |d| + K d_mu^2 from the error of d; the division, the addition of
    epsilon, the square root and the reciprocal one rounding each: e_rstd = ((K + 3) u sum d^2 + 2 d_mu sum |d| + K d_mu^2) /
    (2 K (var + eps)) + 3 u, relative.  The two multiplies and the addition of the affine part one rounding each:
        e_act = rstd |g| (d_mu + u |d|) + |n g| (e_rstd + 3 u) + u |n g + b|,     n = d rstd.
    ln_f32_restatement evaluates the kernel's statistics in float32 in two summation orders; test_decode_gemv_refs.py shows that
    both stay inside e_act.
  * GELU: |erf error| <= 1.5e-7 (csrc/common.h) through 0.5 v (1 + erf): 0.5 |v| 1.5e-7, the rounding of v / sqrt(2) through erf's
    slope (<= 0.5 u |v| 1.13), three more roundings 3 u |gelu|, and the input error through |gelu'| <= 1.13.  16-bit outputs (epi 1 /
    8, the caches of epi 6) add the one rounding of the stored value, half a spacing at |ref| + bound.

Two allowances cannot be derived from documentation and are measured on MI355X against the float64 reference (never against
the code under test), with a 4 x margin: COMB_YARDSTICK (the combine's __expf, sums and division) and LNA_YARDSTICK (the s2 / K - mean^2
variance of gemv_mt_kernel LNA).  See the constants."""
import functools
import math

import numpy as np

from tests.decode_stage_refs import (SENTINEL, SIG, U32, assert_equal, assert_fold16, assert_within, centred_rows, dyadic,  # noqa: F401
                                     fold_ulp_cap, frag_index, grid12, ordinal16, round16, ulp16, wfrag_image)
from tests.encoder_refs import gelu64

ATT_NS = 6
LN_EPS = 1e-5
ERF_ERR = 1.5e-7

# Measured on MI355X (tests/test_gpu_decode_gemv.py::test_yardsticks prints the figures and fails when one exceeds twice its record):
# the smallest f32 error of the kernel's value that explains the 16-bit rows it stored (needed_err16), over every element of the
# Gaussian cases of the op, in units of the derived f32 error unit.  The allowance is 4 x the record: a handful of seeds undersamples
# the tail.  Measured: combine 2.187 units; LNA 0.000 units beyond the derived accumulation and GELU bound (no stored value needed
# more than the derived part explains, so the variance term adds no allowance).
#   COMB: unit = u sum_s w_s |o_s| / L of the element (comb_unit).  op 1, rows 17 / 40 / 64, H = 2 / 16 / 20, bf16 and f16.
#   LNA:  unit = u E[y^2] / (var + eps) |v - bias| of the element (lna_unit: one rounding of s2 / K against the variance), on top of
#         the derived accumulation and GELU bound.  op 3, rows 33 / 48 / 64, K = 128 / 1280, n_stats 8 / 80 / 96.
COMB_MEASURED = 2.19
COMB_YARDSTICK = 4 * COMB_MEASURED
LNA_MEASURED = 0.0
LNA_YARDSTICK = 4 * LNA_MEASURED


# ---- number formats ------------------------------------------------------------------------------------------------------------------
def needed_err16(dt, got, ref64):
    """The smallest error of the value in front of the ONE 16-bit rounding that explains the stored number: 0 where got is
    round16(ref64), else the distance from ref64 to the rounding interval of got"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    sg = np.where(got != 0, np.sign(got), np.where(ref < 0, -1.0, 1.0))
    ag, ar = np.abs(got), ref * sg
    up = ag + 0.5 * ulp16(dt, ag)
    lo = np.where(ag > 0, ag - 0.5 * ulp16(dt, ag * (1 - 2.0 ** -13)), -0.5 * ulp16(dt, 0.0))
    return np.maximum(0.0, np.maximum(lo - ar, ar - up))


def boundary_distance16(dt, ref64):
    """distance of every value to the nearest 16-bit rounding boundary (the midpoint of two neighbouring numbers)"""
    ref = np.abs(np.asarray(ref64, np.float64))
    r = round16(dt, ref)
    up = r + 0.5 * ulp16(dt, r)
    lo = np.where(r > 0, r - 0.5 * ulp16(dt, r * (1 - 2.0 ** -13)), -0.5 * ulp16(dt, 0.0))
    return np.minimum(up - ref, ref - lo)


def flip_allowance(dt, act64, e_act):
    """per element: 0 where the float64 activation is farther than e_act from every rounding boundary, else the largest distance
    between the kernel's 16-bit number and round16(act64): (floor(e_act / ulp16) + 1) ulp16, the spacing taken at |act| + e_act"""
    act64, e_act = np.asarray(act64, np.float64), np.broadcast_to(np.asarray(e_act, np.float64), np.shape(act64))
    sp = ulp16(dt, np.abs(act64) + e_act)
    near = boundary_distance16(dt, act64) <= e_act
    return np.where(near, (np.floor(e_act / sp) + 1) * sp, 0.0)


def near_share(dt, act64, e_act):
    return float((boundary_distance16(dt, act64) <= e_act).mean())


def flip_share_cap(dt, ref64, e):
    """The share of elements a 16-bit comparison may excuse as not being round16(ref64), from the reference alone: a value changes
    sides only within e of a rounding boundary, and boundaries are ulp16 apart -- mean over the elements of min(1, 2 e / ulp16), the
    form of fold_ulp_cap with the value's own error in place of a rounding count.  A condition, not a measurement."""
    r = 2.0 * np.broadcast_to(np.asarray(e, np.float64), np.shape(ref64)) / ulp16(dt, np.asarray(ref64, np.float64))
    return float(np.minimum(1.0, r).mean())


def assert_fold16_where_derived(dt, got, ref64, e, what=""):
    """assert_fold16 on the elements where "at most one position off" follows from the bound: e <= ulp16 / 2.  (Near zero the spacing
    falls below any absolute error of the value in front of the rounding; assert_act16 holds those elements to e itself.)"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    ok = np.broadcast_to(np.asarray(e, np.float64), ref64.shape) <= 0.5 * ulp16(dt, ref64)
    assert ok.any(), (what, "the bound is wider than half a spacing everywhere")
    assert_fold16(dt, got[ok], ref64[ok], flip_share_cap(dt, ref64[ok], np.broadcast_to(e, ref64.shape)[ok]), what)


def assert_act16(dt, got, ref64, e, what=""):
    """every stored 16-bit number is the rounding of a value within e of the float64 one (so an element farther than e from every
    boundary must BE round16(ref64)), and no more than the share flip_share_cap (+ 3 sigma of that count + 2) differ from it"""
    got = np.asarray(got, np.float64)
    assert got.shape == np.shape(ref64), (what, got.shape, np.shape(ref64))
    assert np.isfinite(got).all(), (what, "not finite")
    need = needed_err16(dt, got, ref64)
    bad = np.argwhere(need > e)
    assert len(bad) == 0, (what, dt, f"{len(bad)} of {got.size} 16-bit values not explained by an error within the bound; first at "
                                     f"{bad[:4].tolist()}: needs {need[tuple(bad[0])]:.3e}, bound "
                                     f"{np.broadcast_to(e, need.shape)[tuple(bad[0])]:.3e}")
    n = got.size * flip_share_cap(dt, ref64, e)
    off = int((got != round16(dt, ref64)).sum())
    assert off <= math.ceil(n + 3 * math.sqrt(n)) + 2, (what, dt, f"{off} of {got.size} values off round16(float64), cap {n:.1f}")


# ---- activations ---------------------------------------------------------------------------------------------------------------------
def ln64(x, g=None, b=None, fault=None, dt=None):
    """LayerNorm over the last axis, biased variance, eps = 1e-5; g = b = None: the folded form (no affine part)"""
    x = np.asarray(x, np.float64)
    if fault == "round_before_centring":
        x = round16(dt, x)
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(-1, keepdims=True)
    n = d / np.sqrt(var + (0.0 if fault == "no_eps" else LN_EPS))
    if g is not None:
        n = n * np.asarray(g, np.float64)
    if b is not None:
        n = n + np.asarray(b, np.float64)
    return n


def ln_e_act(x, g=None, b=None):
    """the derived bound of |f32 LayerNorm - float64 LayerNorm| per element (module docstring)"""
    x = np.asarray(x, np.float64)
    K = x.shape[-1]
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    d_mu = K * U32 * np.abs(x).mean(-1, keepdims=True)
    sd, sd2 = np.abs(d).sum(-1, keepdims=True), (d * d).sum(-1, keepdims=True)
    e_rstd = ((K + 3) * U32 * sd2 + 2 * d_mu * sd + K * d_mu ** 2) / (2 * K * (var + LN_EPS)) + 3 * U32
    gg = 1.0 if g is None else np.abs(np.asarray(g, np.float64))
    ng = np.abs(d * rstd) * gg
    res = ng if b is None else np.abs(d * rstd * (1.0 if g is None else np.asarray(g, np.float64)) + np.asarray(b, np.float64))
    return rstd * gg * (d_mu + U32 * np.abs(d)) + ng * (e_rstd + 3 * U32) + U32 * res


def ln_f32_restatement(x, g, b, order):
    """the kernel's LayerNorm arithmetic in float32: order 0 sums left to right, order 1 right to left in four interleaved lanes
    that are added at the end"""
    f = np.float32
    x = np.asarray(x, f)
    K = x.shape[-1]

    def total(v):
        if order == 0:
            return np.cumsum(v, -1, dtype=f)[..., -1]
        parts = [np.cumsum(v[..., ::-1][..., i::4], -1, dtype=f)[..., -1] for i in range(4)]
        return ((parts[0] + parts[1]).astype(f) + (parts[2] + parts[3]).astype(f)).astype(f)
    mean = (total(x) / f(K)).astype(f)
    d = (x - mean[..., None]).astype(f)
    q = (total((d * d).astype(f)) / f(K)).astype(f)
    rstd = (f(1) / np.sqrt((q + f(LN_EPS)).astype(f)).astype(f)).astype(f)
    n = (d * rstd[..., None]).astype(f)
    if g is not None:
        n = (n * np.asarray(g, f)).astype(f)
    if b is not None:
        n = (n + np.asarray(b, f)).astype(f)
    return n.astype(np.float64)


def comb_weights(part_ml):
    ml = np.asarray(part_ml, np.float64)
    m, l = ml[..., 0], ml[..., 1]
    w = np.exp(m - m.max(-1, keepdims=True))
    return w, l


def last_group_rows(Mb):
    """rows of the last of min(3, Mb) row groups of ceil(Mb / groups) rows (the launcher's (N / 32, ksplit, G) grid at 160 blocks)"""
    G = min(3, Mb)
    rpb = -(-Mb // G)
    return np.arange(((Mb - 1) // rpb) * rpb, Mb), rpb


def combine64(part_o, part_ml, fault=None):
    """a[b][h 64 + j] = sum_s e^(m_s - M) o_s[b][h 64 + j] / sum_s e^(m_s - M) l_s,  (m_s, l_s) = part_ml[b][h][s],  M = max_s m_s"""
    po = np.asarray(part_o, np.float64)
    ml = np.asarray(part_ml, np.float64)
    NS, Mb, K = po.shape
    H = K // 64
    assert ml.shape == (Mb, H, NS, 2)
    if fault == "ml_next_head":
        ml = np.roll(ml, -1, axis=1)
    if fault == "ml_next_row_last_group":
        rows, _ = last_group_rows(Mb)
        ml = ml.copy()
        ml[rows] = np.asarray(part_ml, np.float64)[np.minimum(rows + 1, Mb - 1) if len(rows) > 1 else np.maximum(rows - 1, 0)]
    if fault == "plane_group_stride":
        rows, rpb = last_group_rows(Mb)                           # plane stride rpb K instead of Mb K
        flat = po.reshape(-1)
        s, b, k = np.meshgrid(np.arange(NS), np.arange(Mb), np.arange(K), indexing="ij")
        po = flat[np.minimum(s * rpb * K + b * K + k, flat.size - 1)]
    w, l = comb_weights(ml)                                      # [Mb][H][NS]
    L = (w * l).sum(-1)                                          # [Mb][H]
    o = po.reshape(NS, Mb, H, 64)
    return (np.einsum("bhs,sbhj->bhj", w, o) / L[..., None]).reshape(Mb, K)


def comb_unit(part_o, part_ml):
    """the f32 error unit of a combined element: u sum_s w_s |o_s| / L"""
    po = np.abs(np.asarray(part_o, np.float64))
    NS, Mb, K = po.shape
    w, l = comb_weights(part_ml)
    L = (w * l).sum(-1)
    return U32 * (np.einsum("bhs,sbhj->bhj", w, po.reshape(NS, Mb, K // 64, 64)) / L[..., None]).reshape(Mb, K)


def cvec64(pstats, n_pstats, Mb, K, fault=None):
    """c[m] = sum over the n_pstats slots of pstats[m / 16][slot][m % 16][0] / K"""
    ps = np.asarray(pstats, np.float64).reshape(-1, n_pstats, 16, 2)
    m = np.arange(Mb)
    n = n_pstats - 1 if fault == "cvec_short" else n_pstats
    comp = 1 if fault == "cvec_squares" else 0
    return ps[m >> 4, :n, m & 15, comp].sum(1) / K


# ---- the GEMV ------------------------------------------------------------------------------------------------------------------------
def gelu_tanh64(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1 + np.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))


_W16 = {}


def w16_of(dt, W):
    """round16(dt, W); cached for the shared read-only matrices of _weights"""
    if getattr(W, "flags", None) is None or W.flags.writeable:
        return round16(dt, W)
    key = (id(W), dt)
    if key not in _W16:
        if len(_W16) >= 4:
            _W16.clear()
        _W16[key] = (W, round16(dt, W))                           # W kept alive: its id stays its own
    return _W16[key][1]


def weights_seen(dt, W, wpk, fault=None):
    """round16(W), or what a kernel with a wrong weight address multiplies"""
    W16 = w16_of(dt, W)
    N, K = W16.shape
    if fault == "w_kslice_shift" and wpk:                        # one 32-wide K step further in the packed image (the last wraps)
        return np.roll(W16, -32, axis=1)
    if fault == "packed_as_rowmajor" and wpk:
        return wfrag_image(W16, N, K)[:N * K].reshape(N, K)
    return W16


def activation64(dt, o, fault=None):
    """act64 of the operand dict o: x, LN(x) or the combination"""
    if o.get("part_o") is not None:
        return combine64(o["part_o"], o["part_ml"], fault)
    x = np.asarray(o["x"], np.float64)
    if o.get("ln") is None:
        return x
    lf = fault if fault in ("no_eps", "round_before_centring") else None
    if o["ln"] == "affine":
        return ln64(x, o["ln_g"], o["ln_b"], lf, dt)
    return ln64(x, None, None, lf, dt)


def gemv64(dt, o, fault=None, slices=1, round_act=True):
    """Reference of one cw_launch_gemv call on the operand dict o (gemv_operands / comb_operands): -> dict with a16 (the rounded
    activations; round_act = False keeps them unrounded), acc, and the expected contents of every in / out buffer: out [Mb][ldo] (epi 6:
    q [Mb][d_model]), sk, sv.  slices: K slices of the in-place residual form (equal contiguous parts)."""
    epi, Mb, N, K, ldo = o["epi"], o["Mb"], o["N"], o["K"], o["ldo"]
    act = activation64(dt, o, fault)
    a16 = round16(dt, act) if round_act else act
    Ws = weights_seen(dt, o["W"], o["wpk"], fault)
    bias = np.zeros(N) if o.get("bias") is None else np.asarray(o["bias"], np.float64)
    res = {"a16": a16, "act": act}
    out = np.asarray(o["out0"], np.float64).copy()
    if epi == 2 and dt == "f32":                                 # the parity engine: out = resid + acc + bias, no grid, no K split
        resid = out[:, :N] if o["inplace"] else np.asarray(o["resid"], np.float64)[:, :N]
        res["acc"] = a16 @ Ws.T
        out[:, :N] = resid + res["acc"] + bias
    elif epi == 2:
        resid = out[:, :N] if o["inplace"] else np.asarray(o["resid"], np.float64)[:, :N]
        edges = np.linspace(0, K, slices + 1).astype(int)
        parts = [a16[:, s:e] @ Ws[:, s:e].T for s, e in zip(edges[:-1], edges[1:])]
        if fault == "grid_after_resid":
            v = grid12(resid + sum(parts) + bias)
        else:
            v = resid.copy()
            for s, p in enumerate(parts):
                add = bias if (s == 0 or fault == "bias_every_slice") and fault != "bias_none" else 0.0
                if fault == "bias_every_slice" and slices == 1:
                    add = 2 * bias
                v = v + grid12(p + add)
        out[:, :N] = v
        res["acc"] = sum(parts)
    else:
        acc = a16 @ Ws.T
        v = acc + (0.0 if fault == "bias_none" else bias)
        res["acc"] = acc
        if epi in (1, 7, 8):
            v = gelu_tanh64(v) if fault == "gelu_tanh" else gelu64(v)
        if epi == 6:
            d, H, cap = o["d_model"], o["H"], o["cap"]
            pos = np.asarray(o["pos"])
            if fault == "pos_last_row":
                pos = np.full(Mb, pos[Mb - 1])
            if fault == "pos_plus_one":
                pos = (pos + 1) % cap
            grp = [v[:, :d], v[:, d:2 * d], v[:, 2 * d:]]
            if fault == "qkv_swapped":
                grp = [grp[0], grp[2], grp[1]]
            out[:, :d] = grp[0]
            sk, sv = np.asarray(o["sk0"], np.float64).copy(), np.asarray(o["sv0"], np.float64).copy()
            b = np.arange(Mb)
            sk[b, :, pos] = grp[1].reshape(Mb, H, 64)
            sv[b, :, pos] = grp[2].reshape(Mb, H, 64)
            res["sk"], res["sv"] = sk, sv
        else:
            out[:, :N] = v
    res["out"] = out
    return res


def gelu_bound(v, dv):
    """|f32 gelu_erf(v') - gelu64(v)| for |v' - v| <= dv (module docstring)"""
    v = np.abs(np.asarray(v, np.float64))
    return 1.13 * dv + 0.5 * v * (ERF_ERR + 0.6 * U32 * v) + 3 * U32 * np.abs(gelu64(v))


def acc_bound(dt, o, ref, e_act=None):
    """bound of |kernel accumulator + bias - (acc + bias)|: the f32 accumulation, the flips of the activation (e_act: per element
    bound of the kernel's f32 activation against act64; None: the activation is an input, rounded alike on both sides)"""
    W16 = np.abs(w16_of(dt, o["W"]))
    b = 2 * o["K"] * U32 * (np.abs(ref["a16"]) @ W16.T) + 2 * U32 * np.abs(ref["acc"])
    if e_act is not None:
        b = b + flip_allowance(dt, ref["act"], e_act) @ W16.T
    return b


def out_bound(dt, o, ref, e_act=None, slices=1, stored=True):
    """the derived bound of every element of `out` (epi 6: of v = [q | k | v] before placement and before the 16-bit store of k / v)
    -- module docstring.  stored = False: epi 1 / 8 without the rounding of the 16-bit store (the bound assert_act16 takes)"""
    b = acc_bound(dt, o, ref, e_act)
    epi = o["epi"]
    bias = 0.0 if o.get("bias") is None else np.asarray(o["bias"], np.float64)
    v = ref["acc"] + bias
    if epi == 2:
        # every slice's grid rounding, and that of the reference (evaluated with one slice)
        return b + (slices + 1) * 2.0 ** -13 + 2 * U32 * np.abs(ref["out"][:, :o["N"]])
    if epi in (1, 7, 8):
        b = gelu_bound(v, b + U32 * np.abs(v))
        if epi != 7 and stored:
            b = b + 0.5 * ulp16(dt, np.abs(gelu64(v)) + b)
        return b
    return b + U32 * np.abs(v)


def stored16_bound(dt, ref64, b):
    """a value within b of ref64, stored with one 16-bit rounding"""
    return b + 0.5 * ulp16(dt, np.abs(ref64) + b)


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def f32r(a):
    return np.asarray(a, np.float32).astype(np.float64)


def sentinel(*shape):
    return np.full(shape, SENTINEL, np.float64)


@functools.lru_cache(maxsize=4)
def _weights(kind, N, K, seed):
    """W [N][K], bias [N] of a shape, shared by its row counts (read-only)"""
    rng = np.random.default_rng([59, N, K, seed, kind == "exact"])
    if kind == "exact":
        W, bias = rng.integers(-2, 3, (N, K)) / 2.0, rng.integers(-8, 9, N) / 2.0
    else:
        W = f32r(0.05 * rng.standard_normal((N, K)).astype(np.float32) * 2.0 ** rng.integers(-2, 3, N)[:, None])
        bias = f32r(0.1 * rng.standard_normal(N))
    W.setflags(write=False)
    bias.setflags(write=False)
    return W, bias


def gemv_operands(kind, dt, *, epi, Mb, N, K, ldo=None, wpk=0, ln=None, inplace=False, x16=False, ties=False, head_only=False,
                  H=0, cap=0, identity=False, seed=0):
    """Operands of one op 0 call without a combine.  kind "exact" (module docstring; no LayerNorm) or "gauss": rows N(0, 1) with an
    outlier channel (30) on every other row; LayerNorm inputs: every third row (centred_rows) a mean 40 x its spread, row 0 a spread
    of 3e-3 (var ~ eps); W 0.05 N(0, 1) times a power of two per output column in 1/4 .. 4; bias 0.1 N(0, 1); gamma 1 + 0.1 N(0, 1),
    beta 0.1 N(0, 1) (folded: gamma holds 7.0, which the kernel must not use); the residual on the 2^-12 grid.  identity: W = I (N =
    K), no bias: the activation readout.  epi 6: distinct pos per row including 0 and cap - 1, d_model = N / 3."""
    ldo = N if ldo is None else ldo
    rng = np.random.default_rng([61, epi, Mb, N % 9973, K, wpk, int(inplace) + 2 * int(x16) + 4 * int(ties), seed, kind == "exact"])
    o = {"op": 0, "epi": epi, "Mb": Mb, "N": N, "K": K, "ldo": ldo, "wpk": int(wpk), "ln": ln, "inplace": bool(inplace), "x16": bool(x16),
         "kind": kind}
    if kind == "exact":
        assert ln is None
        x = rng.integers(-1, 2, (Mb, K)).astype(np.float64)
        if head_only:
            x[:, 128:] = 0
        W, bias = _weights("exact", N, K, seed)
        if ties:
            bias = bias + rng.choice([-1.0, 0.0, 1.0], N) * 2.0 ** -13
        resid = rng.integers(-8192, 8193, (Mb, ldo)) / 4096.0
    else:
        x = rng.standard_normal((Mb, K))
        x[1::2, 7 % K] = 30.0
        if ln is not None:
            cen = centred_rows(Mb)
            x[cen] = 40.0 * 0.25 + 0.25 * x[cen]
            x[0] *= 3e-3
        x = f32r(x)
        W, bias = _weights("gauss", N, K, seed)
        resid = np.rint(rng.standard_normal((Mb, ldo)) * 4096) / 4096
    if identity:
        assert N == K
        W, bias = np.eye(N), None
    if x16:
        x = round16(dt, x)
    o.update(x=x, W=W, bias=bias)
    if ln == "affine":
        o.update(ln_g=f32r(1 + 0.1 * rng.standard_normal(K)), ln_b=f32r(0.1 * rng.standard_normal(K)))
    elif ln == "folded":
        o.update(ln_g=np.full(K, 7.0), ln_b=None)
    if epi == 2:
        if inplace:
            o["out0"] = resid
        else:
            o.update(resid=resid, out0=sentinel(Mb, ldo))
    elif epi == 6:
        d = N // 3
        pos = (np.arange(Mb) * 7) % (cap - 2) + 1                 # distinct among any cap - 2 consecutive rows
        pos[0] = cap - 1
        pos[min(1, Mb - 1)] = 0 if Mb > 1 else cap - 1
        o.update(d_model=d, H=H, cap=cap, pos=pos.astype(np.int32), out0=sentinel(Mb, d), sk0=sentinel(Mb, H, cap, 64),
                 sv0=sentinel(Mb, H, cap, 64), ldo=d)
    else:
        o["out0"] = sentinel(Mb, ldo)
    return o


def comb_operands(kind, dt, *, Mb, K, H, N=None, wpk=1, op=0, readout=False, seed=0):
    """Partials of a combine (op 0 epi 2 in place, or op 1).  "exact": equal maxima per (row, head), l powers of two that sum to L
    in {8, 16, 32, 64} -- L differs between neighbouring heads and neighbouring rows -- and o_s = L / 4 times ints in [-2, 2]: e^0 = 1,
    L, 1 / L and a = sum_s ints / 4 (|a| <= 3, five bits) are exact.  "gauss": maxima N(0, 2), one split of every third (row, head)
    dominant by 8; l in [1, 50); o_s = l_s v with |v| in [1, 8): the combined |a| lies in [1, 8), where the 16-bit spacing is coarser
    than the 2^-12 grid.  readout: W = I, no bias."""
    assert H * 64 == K
    N = K if N is None else N
    rng = np.random.default_rng([67, Mb, K, H, N % 9973, op, seed, kind == "exact"])
    b, h = np.meshgrid(np.arange(Mb), np.arange(H), indexing="ij")
    ml = np.zeros((Mb, H, ATT_NS, 2))
    if kind == "exact":
        Lx = (b + 2 * h) % 4                                     # L = 8 << Lx
        ml[..., 0] = rng.integers(-3, 4, (Mb, H))[..., None].astype(np.float64)
        pat = np.asarray([1, 1, 1, 1, 2, 2], np.float64)         # sums to 8
        for s in range(ATT_NS):
            ml[..., s, 1] = pat[(s + b + h) % ATT_NS] * 2.0 ** Lx
        L = ml[..., 1].sum(-1)
        assert np.array_equal(L, 8.0 * 2.0 ** Lx)
        ints = rng.integers(-2, 3, (ATT_NS, Mb, H, 64)).astype(np.float64)
        po = (ints * (L / 4.0)[None, :, :, None]).reshape(ATT_NS, Mb, K)
    else:
        ml[..., 0] = 2.0 * rng.standard_normal((Mb, H, ATT_NS))
        dom = ((b * H + h) % 3 == 0)
        ml[dom, (b + h)[dom] % ATT_NS, 0] += 8.0
        ml[..., 1] = rng.uniform(1.0, 50.0, (Mb, H, ATT_NS))
        ml = f32r(ml)
        sign = rng.choice([-1.0, 1.0], (Mb, H, 64))
        v = rng.uniform(1.0, 8.0, (ATT_NS, Mb, H, 64)) * sign[None]
        po = f32r((v * ml[..., 1].transpose(2, 0, 1)[..., None]).reshape(ATT_NS, Mb, K))
    o = {"op": op, "epi": 2, "Mb": Mb, "N": N, "K": K, "ldo": N, "wpk": int(wpk), "ln": None, "inplace": True, "x16": False, "H": H,
         "part_o": po, "part_ml": ml, "kind": kind}
    if op == 1:
        o["out0"] = sentinel(Mb, K)
        return o
    if readout:
        W, bias = np.eye(K), None
    elif kind == "exact":
        W, bias = rng.integers(-2, 3, (N, K)) / 2.0, rng.integers(-8, 9, N) / 2.0
    else:
        W = f32r(0.05 * rng.standard_normal((N, K)) * 2.0 ** rng.integers(-2, 3, N)[:, None])
        bias = f32r(0.1 * rng.standard_normal(N))
    resid = rng.integers(-8192, 8193, (Mb, N)) / 4096.0
    o.update(W=W, bias=bias, out0=resid)
    return o


def pstats_operands(Mb, K, n_pstats, seed=0):
    """planes [ceil(Mb / 16)][n_pstats][16][2] of f32 numbers on a 2^-6 grid (their sums are exact in f32 in any order); rows beyond
    Mb hold NaN"""
    rng = np.random.default_rng([71, Mb, K, n_pstats, seed])
    g = (Mb + 15) // 16
    ps = rng.integers(-2048, 2049, (g, n_pstats, 16, 2)) / 64.0
    m = np.arange(g * 16)
    ps[m[Mb:] >> 4, :, m[Mb:] & 15] = np.nan
    return ps


# ---- the 33..64-row chain pieces -----------------------------------------------------------------------------------------------------
def own_operands(kind, dt, *, Mb, N, K, seed=0):
    """cw_launch_gemv_own: rows a (already 16-bit), W, bias, the residual in place, the centres c.  "exact": a in {-1, 0, 1}, W in
    halves with 16 dense and about 8 further non-zero columns per row of a, bias in halves (+- 2^-13: grid ties in both directions,
    which resolve onto the halves), resid = c + halves in [-2, 2] with c an integer in [-8, 8] plus an odd multiple of 2^-12 (the
    residual sits on odd grid points: rounding after the residual add resolves the ties the other way): x_new, y = x_new - c (a few
    halves: a number of both 16-bit types) and the block sums of y and y^2 are exact in f32.  "gauss": a N(0, 1) rounded, c the row mean of the residual to within a few percent of its
    spread."""
    rng = np.random.default_rng([73, Mb, N, K, seed, kind == "exact"])
    if kind == "exact":
        a = rng.integers(-1, 2, (Mb, K)).astype(np.float64)
        a[:, 16:] *= (rng.random((Mb, K - 16)) < 8.0 / K)          # about 8 further non-zeros per row: |acc| stays small
        W = rng.integers(-2, 3, (N, K)) / 2.0
        bias = rng.integers(-2, 3, N) / 2.0 + rng.choice([-1.0, 0.0, 1.0], N) * 2.0 ** -13
        c = rng.integers(-8, 9, Mb) + (2 * rng.integers(0, 64, Mb) + 1) / 4096.0
        resid = c[:, None] + rng.integers(-4, 5, (Mb, N)) / 2.0
    else:
        a = round16(dt, rng.standard_normal((Mb, K)))
        W = f32r(0.05 * rng.standard_normal((N, K)) * 2.0 ** rng.integers(-2, 3, N)[:, None])
        bias = f32r(0.1 * rng.standard_normal(N))
        mean = 3.0 * rng.standard_normal(Mb)
        resid = np.rint((mean[:, None] + rng.standard_normal((Mb, N))) * 4096) / 4096
        c = f32r(mean + 0.05 * rng.standard_normal(Mb))
    return {"op": 2, "Mb": Mb, "N": N, "K": K, "wpk": 1, "x": a, "W": W, "bias": bias, "out0": resid, "cvec": c, "kind": kind}


def own64(dt, o, nt, fault=None):
    """x_new = resid + grid12(a16 w16^T + b);  y16 = round16(f32(x_new) - f32(c)), ONE float32 subtraction;  stats[block][row] =
    (sum y16, sum y16^2) over the block's 16 nt columns, rows beyond Mb untouched.  -> out, y, stats [N / (16 nt)][64][2], y_f32"""
    Mb, N = o["Mb"], o["N"]
    a16 = round16(dt, o["x"])
    Ws = weights_seen(dt, o["W"], 1, fault)
    acc = a16 @ Ws.T
    bias = np.asarray(o["bias"], np.float64)
    resid = np.asarray(o["out0"], np.float64)
    xn = grid12(resid + acc + bias) if fault == "grid_after_resid" else resid + grid12(acc + (0.0 if fault == "bias_none" else bias))
    c = np.asarray(o["cvec"], np.float32)
    if fault == "y_about_new_mean":
        c = xn.mean(-1).astype(np.float32)
    yf = (xn.astype(np.float32) - c[:, None]).astype(np.float64)   # one f32 subtraction
    y16 = round16(dt, yf)
    cols = 16 * nt
    nb = N // cols
    st = sentinel(nb, 64, 2)
    yb = y16.reshape(Mb, nb, cols)
    st[:, :Mb, 0] = yb.sum(-1).T
    st[:, :Mb, 1] = (yb * yb).sum(-1).T
    if fault == "stats_slot_next_block":
        st = np.roll(st, 1, axis=0)
    return {"out": xn, "y": y16, "stats": st, "y_f32": yf, "acc": acc, "a16": a16}


def own_bounds(dt, o, ref, nt):
    """out: the accumulation + half a grid step each for the kernel's rounding and the reference's (their sums in front of the grid
    differ, so they may round to neighbouring grid points);  y: a value within that of y_f32 (+ the subtraction's rounding) in front
    of the 16-bit store;  stats: the block's sums of values each within the y bound of y16 -- the kernel sums its f32 y, the reference the
    rounded y16: half a spacing per element on top -- plus the f32 summation of 16 nt terms"""
    W16 = np.abs(round16(dt, o["W"]))
    b_out = 2 * o["K"] * U32 * (np.abs(ref["a16"]) @ W16.T) + 2 * U32 * np.abs(ref["acc"]) + 2 * 2.0 ** -13
    b_yf = b_out + U32 * np.abs(ref["y_f32"])
    b_y = b_yf                                                  # of the value in front of the 16-bit store (assert_act16 against y_f32)
    cols = 16 * nt
    Mb, N = o["Mb"], o["N"]
    nb = N // cols
    e = (b_yf + 0.5 * ulp16(dt, np.abs(ref["y_f32"]) + b_yf)).reshape(Mb, nb, cols)
    ay = np.abs(ref["y"]).reshape(Mb, nb, cols)
    b_st = np.zeros((nb, 64, 2))
    b_st[:, :Mb, 0] = (e.sum(-1) + cols * U32 * ay.sum(-1)).T
    b_st[:, :Mb, 1] = ((2 * ay * e + e * e).sum(-1) + (cols + 1) * U32 * ((ay + e) ** 2).sum(-1)).T
    return b_out, b_y, b_st


def lna_operands(dt, *, Mb, N, K, n_stats, seed=0):
    """cw_launch_gemv_lna: rows y (16-bit) with |mean_y| <= 0.5 sigma, as the column-owning stage in front guarantees (y = x_new - c,
    c the row's mean one stage earlier) -- row m has the mean (m % 5 - 2) / 4 of its standard deviation, an outlier channel on every
    other row; stats_in [n_stats][64][2] = the f32 sums of
    y16 and y16^2 over n_stats column blocks (rows beyond Mb: NaN); wsum = the f32 row sums of the rounded weights."""
    rng = np.random.default_rng([79, Mb, N, K, n_stats, seed])
    sig = rng.uniform(0.5, 2.0, Mb)
    z = rng.standard_normal((Mb, K))
    z[1::2, 7] = 10.0                                            # the outlier channel
    z = (z - z.mean(-1, keepdims=True)) / z.std(-1, keepdims=True)
    y16 = round16(dt, sig[:, None] * (z + ((np.arange(Mb) % 5 - 2) / 4.0)[:, None]))
    W = f32r(0.05 * rng.standard_normal((N, K)) * 2.0 ** rng.integers(-2, 3, N)[:, None])
    bias = f32r(0.1 * rng.standard_normal(N))
    st = np.full((n_stats, 64, 2), np.nan)
    for j, cols in enumerate(np.array_split(np.arange(K), n_stats)):
        st[j, :Mb, 0] = y16[:, cols].sum(-1)
        st[j, :Mb, 1] = (y16[:, cols] ** 2).sum(-1)
    return {"op": 3, "Mb": Mb, "N": N, "K": K, "wpk": 1, "x": y16, "W": W, "bias": bias, "stats_in": f32r(st), "n_stats": n_stats,
            "wsum": f32r(round16(dt, W).sum(-1)), "out0": sentinel(Mb, N), "kind": "gauss"}


def lna64(dt, o, fault=None):
    """gelu(rstd (y16 w16^T - mean_y wsum) + b),  (mean_y, var) of the whole row of y16,  rstd = 1 / sqrt(var + 1e-5)"""
    y16 = round16(dt, o["x"])
    K = o["K"]
    W16 = weights_seen(dt, o["W"], 1, fault)
    mean = y16.mean(-1)
    ex2 = (y16 * y16).mean(-1)
    if fault == "lna_mean_short":                                # the statistics over n_stats - 1 slots
        st = np.asarray(o["stats_in"], np.float64)[:-1, :o["Mb"]]
        mean, ex2 = st[..., 0].sum(0) / K, st[..., 1].sum(0) / K
    var = np.maximum(ex2 - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + (0.0 if fault == "no_eps" else LN_EPS))
    wsum = np.asarray(o["W"], np.float64).sum(-1) if fault == "wsum_unrounded" else np.asarray(o["wsum"], np.float64)
    acc = y16 @ W16.T
    lin = rstd[:, None] * (acc - mean[:, None] * wsum)
    v = lin + np.asarray(o["bias"], np.float64)
    return {"out": gelu_tanh64(v) if fault == "gelu_tanh" else gelu64(v), "v": v, "lin": lin, "acc": acc, "mean": mean, "var": var,
            "ex2": ex2, "rstd": rstd, "y16": y16}


def lna_unit(ref):
    """u E[y^2] / (var + eps) |v - bias|: what one rounding of s2 / K does to rstd (v - bias) through var = s2 / K - mean^2"""
    return U32 * (ref["ex2"] / (ref["var"] + LN_EPS))[:, None] * np.abs(ref["lin"])


def lna_derived_bound(dt, o, ref):
    """the accumulation, the product mean_y wsum and the sums of the statistics (n_stats + 2 terms each, the slot sums given in f32),
    through rstd; the roundings of the normalisation; then GELU and the 16-bit store"""
    W16 = np.abs(round16(dt, o["W"]))
    n = o["n_stats"] + 2
    mw = np.abs(ref["mean"])[:, None] * np.abs(np.asarray(o["wsum"], np.float64))
    dv = ref["rstd"][:, None] * (2 * o["K"] * U32 * (np.abs(ref["y16"]) @ W16.T) + (n + 2) * U32 * mw + 2 * U32 * np.abs(ref["acc"]))
    dv = dv + 4 * U32 * np.abs(ref["lin"]) + U32 * np.abs(ref["v"])
    return dv


def lna_bound(dt, o, ref, yardstick=None):
    """of the value in front of the 16-bit store (the bound assert_act16 takes)"""
    yardstick = LNA_YARDSTICK if yardstick is None else yardstick
    dv = lna_derived_bound(dt, o, ref) + yardstick * (o["n_stats"] + 2) * lna_unit(ref)
    return gelu_bound(ref["v"], dv)


# ---- launcher selection (coverage only) ----------------------------------------------------------------------------------------------
def launcher_branches(o, *, gemv_loop=1, comb_rowgroups=1, mt_variant=-1, comb_nt2=0):
    """A restatement of the selection in csrc/gemm.hip (cw_launch_gemv -> launch_gemv_epi -> launch_gemv2 / launch_gemv2_shape /
    launch_gemv_large / launch_gemv_mt) for the 16-bit engines: the set of branch names one call reaches.  Used by the coverage
    assertion of tests/test_decode_gemv_refs.py only -- never to compute an expected value."""
    op = o["op"]
    Mb, K = o["Mb"], o["K"]
    tags = set()
    if op == 1:
        tags.add("prep<combine>")
        if o.get("pstats") is not None:
            tags.add("prep.cvec_out")
        return tags
    N = o["N"]
    if op == 2:
        steps = K // 128
        return {"mt.OWN", f"mt.OWN.NSLOT{1 if steps <= 4 else 2 if steps <= 8 else 3}", f"mt.OWN.rowtiles{(Mb + 15) // 16}"}
    if op == 3:
        steps = K // 128
        return {"mt.LNA", f"mt.LNA.NSLOT{1 if steps <= 4 else 2 if steps <= 8 else 3}"}
    epi, wpk = o["epi"], o["wpk"]
    ln, comb = o.get("ln") is not None, o.get("part_o") is not None
    inplace = epi == 2 and o["inplace"]
    if Mb > 16 and wpk:
        if o.get("frag_in"):
            tags.add("mt.producer(x=null)")
        else:
            tags.add("prep<combine>" if comb else "prep<plain>")
            if ln:
                tags.add("prep.ln_" + o["ln"])
        ksplit = 1
        if inplace:
            tiles, steps = (N + 15) // 16, K // 128
            while tiles * ksplit < 256 and steps % (ksplit * 2) == 0 and steps // (ksplit * 2) >= 4:
                ksplit *= 2
        while K // ksplit > 1280:
            ksplit *= 2
        MT = (Mb + 15) // 16
        steps = (K // ksplit) // 128
        ns = 1 if steps <= 4 else 2 if steps <= 8 else 3
        variant = mt_variant if mt_variant >= 0 else (2 if N % 32 == 0 and (N // 32) * ksplit * 2 >= 160 else 1)
        tags |= {f"mt.MT{MT}", f"mt.NSLOT{ns}", f"mt.epi{epi}"}
        if epi == 2 and ksplit > 1:
            tags.add("mt.ATOMIC")
        if MT >= 3 and variant >= 1 and (variant == 1 or N % 32 == 0):
            tags.add(f"mt.variant{variant}")
        else:
            tags.add("mt.variant0")
        return tags
    for m_base in range(0, Mb, 16):
        rows = min(16, Mb - m_base)
        rpw = 2 if rows <= 8 else 4
        t = {f"gemv2.RPW{rpw}", f"gemv2.epi{epi}", "gemv2.wpk" if wpk else "gemv2.rowmajor"}
        if m_base > 0:
            t |= {"gemv2.m_base>0", f"gemv2.m_base>0.epi{epi}"}
        if ln:
            t.add("gemv2.ln_" + o["ln"])
        ksplit = 1
        if inplace and not ln:
            tiles, steps = (N + 15) // 16, K // 128
            while tiles * ksplit < 256 and steps % (ksplit * 2) == 0 and steps // (ksplit * 2) >= 4:
                ksplit *= 2
        while K // ksplit > 1280:
            ksplit *= 2
        if inplace and not ln and not comb and K > 1280 and N % 32 == 0:
            ks = ksplit + 1
            while (N // 32) * ks <= 256:
                if K % (ks * 128) == 0:
                    ksplit = ks
                ks += 1
        if comb_nt2 and comb and inplace and K % 256 == 0 and K >= 512 and N % 32 == 0:
            tags |= t | {"gemv2.COMBINE.NT2(CW_COMB_NT2)"}
            continue
        Kb = K // ksplit
        if comb and ksplit > 1 and rows > 1 and N % 32 == 0 and 256 < Kb <= 768 and comb_rowgroups:
            G = max(1, min(rows, 256 // ((N // 32) * ksplit)))
            if rpw == 4 and rows > 12 and -(-rows // G) <= 8:
                tags |= t | {"gemv2.COMBINE.rowgroups.RPW2", f"gemv2.COMBINE.G{G}"}
                rpb = -(-rows // G)
                if rows % rpb:
                    tags.add("gemv2.COMBINE.short_or_empty_group")
                if rpb * (G - 1) >= rows:
                    tags.add("gemv2.COMBINE.empty_group")
                continue
            while G > 1 and -(-rows // G) > 4:
                G += 1
            if -(-rows // G) <= 4:
                rpb = -(-rows // G)
                tags |= t | {"gemv2.COMBINE.rowgroups.RPW1", f"gemv2.COMBINE.G{G}"}
                if rows % rpb:
                    tags.add("gemv2.COMBINE.short_or_empty_group")
                if rpb * (G - 1) >= rows:
                    tags.add("gemv2.COMBINE.empty_group")
                continue
        shape = "NSLOT1" if Kb <= 256 else "NSLOT2" if Kb <= 768 else "NSLOT3"
        t.add("gemv2." + shape)
        gx = (N + 15) // 16
        if comb:
            t.add("gemv2.COMBINE.(N/16,ksplit)" if ksplit > 1 else "gemv2.COMBINE.single")
        elif epi == 2 and ksplit > 1:
            t.add("gemv2.ATOMIC")
            if N % 32 == 0 and gx * ksplit > 256 and gx * ksplit // 2 >= 128:
                t.add("gemv2.ATOMIC.NT2")
            if o.get("x16"):
                t.add("gemv2.X16")
        elif epi == 5 and ln and ksplit == 1 and gx >= 1024 and wpk and K <= 1280 and gemv_loop and m_base == 0:
            t.add("gemv_loop")
        elif ln and ksplit == 1 and gx >= 1024:
            t.add("gemv2.LN.NT3")
            if gx % 3:
                t.add("gemv2.LN.NT3.tail")
        elif ln and ksplit == 1 and gx > 256 and gx // 2 >= 128:
            t.add("gemv2.LN.NT2")
        if N % 16:
            t.add("gemv2.clamped_columns")
        tags |= t
    return tags


# every branch of the launchers that decode_step reaches (the issue's list); the case table of the GPU module must cover them all
REQUIRED_BRANCHES = {
    "gemv2.wpk", "gemv2.rowmajor", "gemv2.RPW2", "gemv2.RPW4", "gemv2.ATOMIC", "gemv2.ATOMIC.NT2", "gemv2.X16", "gemv2.NSLOT1",
    "gemv2.NSLOT2", "gemv2.NSLOT3", "gemv2.epi1", "gemv2.epi2", "gemv2.epi5", "gemv2.epi6", "gemv2.epi7", "gemv2.LN.NT2", "gemv2.LN.NT3",
    "gemv2.LN.NT3.tail", "gemv2.ln_affine", "gemv2.ln_folded", "gemv2.clamped_columns", "gemv_loop",
    "gemv2.COMBINE.(N/16,ksplit)", "gemv2.COMBINE.rowgroups.RPW1", "gemv2.COMBINE.rowgroups.RPW2", "gemv2.COMBINE.short_or_empty_group",
    "gemv2.COMBINE.empty_group", "gemv2.COMBINE.NT2(CW_COMB_NT2)",
    "prep<plain>", "prep<combine>", "prep.ln_affine", "prep.ln_folded", "prep.cvec_out", "mt.producer(x=null)",
    "mt.MT2", "mt.MT3", "mt.MT4", "mt.NSLOT1", "mt.NSLOT2", "mt.NSLOT3", "mt.ATOMIC", "mt.epi2", "mt.epi5", "mt.epi6", "mt.epi8",
    "mt.variant0", "mt.variant1", "mt.variant2",
    "gemv2.m_base>0", "gemv2.m_base>0.epi2", "gemv2.m_base>0.epi6", "gemv2.m_base>0.epi7",
    "mt.OWN", "mt.OWN.NSLOT1", "mt.OWN.NSLOT3", "mt.LNA", "mt.LNA.NSLOT1", "mt.LNA.NSLOT3",
}

ROWS16 = [1, 5, 8, 9, 16]
ROWS64 = [17, 32, 33, 48, 49, 64]


def case_table():
    """Every (description, call keywords, switches) the GPU module launches: the skeleton operand dicts (no arrays) that
    launcher_branches reads.  slices: the K slices of the reference and of the bound -- "K/128" the cap, an int where the launcher's
    documented rule fixes the count (fc2: K = 5120, N = 1280 -> grid (40, 5))."""
    T = []

    def add(name, sw=None, **kw):
        kw.setdefault("op", 0)
        kw.setdefault("wpk", 1)
        kw.setdefault("inplace", False)
        T.append((name, kw, sw or {}))
    for wpk in (0, 1):
        for Mb in ROWS16:
            add("ksplit N=16", epi=2, Mb=Mb, N=16, K=1024, wpk=wpk, inplace=True)
            add("ksplit NT2", epi=2, Mb=Mb, N=2080, K=1024, wpk=wpk, inplace=True)
            add("fc2", epi=2, Mb=Mb, N=1280, K=5120, wpk=wpk, inplace=True)
            add("fc2 x16", epi=2, Mb=Mb, N=1280, K=5120, wpk=wpk, inplace=True, x16=True)
            add("x16 N=48", epi=2, Mb=Mb, N=48, K=2560, wpk=wpk, inplace=True, x16=True)
            add("ksplit clamped", epi=2, Mb=Mb, N=43, K=1024, wpk=wpk, inplace=True)
    for ln in ("affine", "folded"):
        for Mb in (1, 8, 13):
            add("LN NT2", epi=5, Mb=Mb, N=4112, K=256, ln=ln)
            for N in (16400, 16411):
                add("LN NT3 row-major", epi=5, Mb=Mb, N=N, K=128, ln=ln, wpk=0)
                add("LN NT3 packed", {"gemv_loop": 0}, epi=5, Mb=Mb, N=N, K=128, ln=ln)
                for K in (128, 1280):
                    add("LN loop", {"gemv_loop": 1}, epi=5, Mb=Mb, N=N, K=K, ln=ln)
    for Mb in (5, 13):
        for H in (2, 20):
            add("qkv cache", epi=6, Mb=Mb, N=3 * H * 64, K=H * 64, ln="folded", H=H)
            add("qkv cache", epi=6, Mb=Mb, N=3 * H * 64, K=H * 64, ln="affine", H=H, wpk=0)
            add("qkv cache exact", epi=6, Mb=Mb, N=3 * H * 64, K=H * 64, H=H)
        for epi in (1, 5, 7):
            add("epilogue", epi=epi, Mb=Mb, N=272, K=640, ln="folded")
        add("separate resid", epi=2, Mb=Mb, N=272, K=640)
    for Mb in (2, 8, 12, 13, 16):
        add("combine rowgroups", {"comb_rowgroups": 1}, epi=2, Mb=Mb, N=1280, K=1280, inplace=True, part_o=True)
        add("combine plain grid", {"comb_rowgroups": 0}, epi=2, Mb=Mb, N=1280, K=1280, inplace=True, part_o=True)
    for Mb in (13, 16):
        add("combine G=6", {"comb_rowgroups": 1}, epi=2, Mb=Mb, N=640, K=1280, inplace=True, part_o=True)
    for Mb in (3, 8):
        add("combine one row per group", {"comb_rowgroups": 1}, epi=2, Mb=Mb, N=64, K=1024, inplace=True, part_o=True)
    add("combine NT2", {"comb_nt2": 1}, epi=2, Mb=8, N=1280, K=1280, inplace=True, part_o=True)
    for Mb in ROWS64:
        for K in (512, 1024, 1280):
            add("mt store", epi=5, Mb=Mb, N=272, K=K, ln="folded")
        add("mt ksplit N=16", epi=2, Mb=Mb, N=16, K=1024, inplace=True)
        add("mt fc2", epi=2, Mb=Mb, N=1280, K=5120, inplace=True)
        add("mt fc2 frag_in", epi=2, Mb=Mb, N=1280, K=5120, inplace=True, frag_in=True)
        add("mt qkv", epi=6, Mb=Mb, N=384, K=128, ln="affine", H=2)
        add("mt gelu frag", epi=8, Mb=Mb, N=512, K=128, ln="folded")
        add("mt combine", epi=2, Mb=Mb, N=1280, K=1280, inplace=True, part_o=True)
        for var in (-1, 0, 1, 2):
            add("mt variants", {"mt_variant": var}, epi=5, Mb=Mb, N=288, K=256, ln="affine")
    for Mb in (17, 40, 64):
        add("row-major groups ksplit", epi=2, Mb=Mb, N=16, K=1024, wpk=0, inplace=True)
        add("row-major groups qkv", epi=6, Mb=Mb, N=384, K=128, ln="folded", H=2, wpk=0)
        add("row-major groups gelu", epi=7, Mb=Mb, N=272, K=640, ln="folded", wpk=0)
    for n_pstats in (1, 40, 80):
        add("rows_combine cvec", op=1, Mb=40, N=1280, K=1280, part_o=True, pstats=True, n_pstats=n_pstats)
    for Mb in (17, 33, 64):
        for D in (128, 1280):
            add("own", op=2, Mb=Mb, N=D, K=D)
    for Mb in (33, 48, 64):
        add("lna", op=3, Mb=Mb, N=64, K=128, n_stats=8)
        add("lna", op=3, Mb=Mb, N=5120, K=1280, n_stats=80)
        add("lna limit", op=3, Mb=Mb, N=64, K=1280, n_stats=96)
    return T


def table_branches():
    got = set()
    for _, kw, sw in case_table():
        o = dict(kw)
        if o.get("part_o") is None:
            o.pop("part_o", None)
        got |= launcher_branches(o, gemv_loop=sw.get("gemv_loop", 1), comb_rowgroups=sw.get("comb_rowgroups", 1),
                                 mt_variant=sw.get("mt_variant", -1), comb_nt2=sw.get("comb_nt2", 0))
    return got


# ---- exactness of the exact operands -------------------------------------------------------------------------------------------------
def f32_gemv_restatement(dt, o, order, slices=1):
    """the exact launch (no LayerNorm, no combine) evaluated in float32 in one of two summation orders"""
    f = np.float32
    a = round16(dt, o["x"]).astype(f)
    W = round16(dt, o["W"]).astype(f)
    K = o["K"]

    def dot(a_, w_):
        k = a_.shape[1]
        acc = np.zeros((a_.shape[0], w_.shape[0]), f)
        rng_ = range(0, k, 32) if order == 0 else range(k - 32, -1, -32)
        for k0 in rng_:
            sl = slice(k0, k0 + 32)
            acc = (acc + (a_[:, sl] @ w_[:, sl].T if order == 0 else a_[:, sl][:, ::-1] @ w_[:, sl][:, ::-1].T)).astype(f)
        return acc
    bias = np.zeros(o["N"], f) if o.get("bias") is None else np.asarray(o["bias"], f)
    if o["epi"] == 2:
        edges = np.linspace(0, K, slices + 1).astype(int)
        out = np.asarray(o["out0"] if o["inplace"] else o["resid"], f)[:, :o["N"]].copy()
        idx = range(slices) if order == 0 else range(slices - 1, -1, -1)
        for s in idx:
            p = dot(a[:, edges[s]:edges[s + 1]], W[:, edges[s]:edges[s + 1]])
            if s == 0:
                p = (p + bias).astype(f)
            out = (out + (np.rint(p * f(4096)) * f(1 / 4096)).astype(f)).astype(f)
        return out.astype(np.float64)
    return (dot(a, W) + bias).astype(f).astype(np.float64)
