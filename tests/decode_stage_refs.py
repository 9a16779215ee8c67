"""Float64 / numpy references, input builders and comparators of the decode-stage kernel tests (tests/test_gpu_decode_stages.py):
the load-time folds (fold_layernorm / fold_product / fold_rowvec / wfrag_pack), the stacked GEMV of the fused out-projection stage
(csrc/decfuse.hip: gemv_stack_kernel) and the query the cross-attention kernels finish from its (sum, sum of squares) planes.  Kept
apart from the GPU module so that tests/test_decode_stage_refs.py can show on a CPU-only machine that every comparator rejects a
subtly wrong kernel output (the `fault` arguments plant one) and that the exact-operand builders are exact.

The references restate the documented operation -- the header comments of the kernels -- not their instruction order."""
import math

import numpy as np

from tests.encoder_refs import SENTINEL, ordinal16, round16   # noqa: F401  (re-exported to the two test modules)

U32 = 2.0 ** -24            # unit roundoff of f32
SIG = {"bf16": 8, "f16": 11}   # significand bits


def ulp16(dt, x):
    """spacing of the engine's 16-bit type at |x| (float64)"""
    sig, emin = (8, -125) if dt == "bf16" else (11, -13)
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.maximum(e, emin) - sig)


def bits16_to_f64(dt, bits):
    """raw 16-bit patterns of the engine's type -> their values"""
    bits = np.asarray(bits, np.uint16)
    if dt == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float16).astype(np.float64)


# ---- load-time folds -----------------------------------------------------------------------------------------------------------------
FOLD_LN_SHAPES = [(5, 128), (66, 1280), (3, 132)]                 # (N, K): one wave per row, 4 rows per block; K % 256 != 0
FOLD_LN_SCALES = [1.0, 0.125]
FOLD_PRODUCT_SHAPES = [(64, 16, 64), (128, 384, 192), (1280, 1280, 64)]   # (N, J, K): one 64 x 64 tile; 2 x 3 tiles; the engine's J
FOLD_ROWVEC_N = [1, 4, 5, 1283]
FOLD_ROWVEC_J = [64, 100, 1280]
PACK_SHAPES = [(16, 32), (10, 64), (51866 % 4096 + 16, 128), (3840, 1280)]


def dyadic(rng, shape, lo=-4, hi=4, den=16.0):
    """ints / den: exact in bf16, f16 and f32, and so is every product and short sum of them"""
    return rng.integers(lo, hi + 1, shape) / den


def fold_ln_inputs(kind, N, K, seed=0):
    """W [N][K], gamma, beta [K], bias0 [N] (non-zero: the kernel accumulates into it).  "dyadic": W ints / 16 in [-4, 4], gamma a
    power of two in 1/2 .. 2, beta ints / 4 -- scale W gamma is a 16-bit number and the bias sum exact in f32.  "gauss": N(0, 1)
    weights, gamma = 1 + 0.1 N(0, 1), beta = 0.1 N(0, 1)."""
    rng = np.random.default_rng([31, N, K, seed])
    if kind == "dyadic":
        return (dyadic(rng, (N, K)), 2.0 ** rng.integers(-1, 2, K), rng.integers(-8, 9, K) / 4.0, rng.integers(-64, 65, N) / 8.0)
    f = np.float32
    return (rng.standard_normal((N, K)).astype(f).astype(np.float64), (1 + 0.1 * rng.standard_normal(K)).astype(f).astype(np.float64),
            (0.1 * rng.standard_normal(K)).astype(f).astype(np.float64), rng.standard_normal(N).astype(f).astype(np.float64))


def fold_layernorm64(W, g, beta, scale, bias0, fault=None):
    """W' = scale W diag(gamma) (one rounding to 16 bits is the comparator's),  bias = bias0 + scale W beta"""
    W, g, beta = (np.asarray(t, np.float64) for t in (W, g, beta))
    s = 1.0 if fault == "no_scale" else scale
    return s * W * g, np.asarray(bias0, np.float64) + s * (W @ beta)


def fold_ln_bias_bound(W, beta, scale, ref_bias):
    """f32 dot-product bound 2 K 2^-24 sum |w beta| (K / 64 products per lane, a six-level butterfly, one product with scale) and the
    rounding of the accumulated sum"""
    W, beta = np.asarray(W, np.float64), np.asarray(beta, np.float64)
    return 2 * W.shape[1] * U32 * abs(scale) * (np.abs(W) @ np.abs(beta)) + 2 * U32 * np.abs(ref_bias)


def fold_product_inputs(kind, N, J, K, with_s, seed=0):
    """A [N][J], s [J] or None, B [J][K], scale = 1/8.  "dyadic": four non-zeros +-1/2, +-1 per row of A at random columns, s a power
    of two in 1/2 .. 2, B in {-1, 0, 1}: every term is a multiple of 2^-5 of at most 1/4, so C is a multiple of 2^-5 with |C| <= 1 --
    six bits, a number of both 16-bit types, and exact in f32 in any order.  "gauss": entries 1 + 0.25 N(0, 1) -- a sum without
    cancellation, so that the f32 accumulation error stays a small share of a 16-bit spacing (fold_ulp_cap)."""
    rng = np.random.default_rng([37, N, J, K, int(with_s), seed])
    if kind == "dyadic":
        A = np.zeros((N, J))
        for n in range(N):
            A[n, rng.choice(J, min(4, J), replace=False)] = rng.choice([-2.0, -1.0, 1.0, 2.0], min(4, J)) / 2.0
        B = rng.choice([-1.0, 0.0, 1.0], (J, K))
        s = 2.0 ** rng.integers(-1, 2, J) if with_s else None
        return A, s, B, 0.125
    f = np.float32
    A = (1 + 0.25 * rng.standard_normal((N, J))).astype(f).astype(np.float64)
    B = (1 + 0.25 * rng.standard_normal((J, K))).astype(f).astype(np.float64)
    s = (1 + 0.1 * rng.standard_normal(J)).astype(f).astype(np.float64) if with_s else None
    return A, s, B, 0.125


def fold_product64(A, s, scale, B, fault=None):
    """C = (A diag(s) scale) B"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    a = A * (1.0 if s is None else np.asarray(s, np.float64)) * (1.0 if fault == "no_scale" else scale)
    return a @ B


def fold_rowvec64(A, s, scale, v, fault=None):
    """c = (A diag(s) scale) v"""
    a = np.asarray(A, np.float64) * (1.0 if s is None else np.asarray(s, np.float64)) * (1.0 if fault == "no_scale" else scale)
    return a @ np.asarray(v, np.float64)


def rowsum64(dt, W):
    """w = W16 1: row sums of the weights as the MFMAs see them"""
    return round16(dt, W).sum(-1)


def fold_ulp_cap(dt, n_roundings):
    """Largest share of 16-bit results that the f32 arithmetic in front of the one 16-bit rounding may move to the neighbouring
    16-bit number: a value changes sides only when it lies within the f32 error e = n_roundings 2^-24 |x| of a rounding boundary, and
    boundaries are at least 2^-sig |x| apart (sig significand bits): 2 e / (2^-sig |x|).  fold_layernorm: the two products scale w
    gamma, n = 2.  fold_product: the J-term f32 sum grows like a random walk over partial sums that grow linearly -- about
    sqrt(J) / 3 roundings of the result -- plus the two products of A s scale; n = sqrt(J) + 2 is three times that estimate."""
    return 2.0 * n_roundings * U32 * 2.0 ** SIG[dt]


def fold16_counts(dt, got, ref64):
    d = np.abs(ordinal16(dt, got) - ordinal16(dt, round16(dt, ref64)))
    return int((d == 1).sum()), int((d > 1).sum())


def assert_fold16(dt, got, ref64, cap, what=""):
    """every 16-bit value within one position of round16(float64), and at most a share `cap` (+ 2 elements: small matrices) off by one"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), (what, "not finite")
    one, more = fold16_counts(dt, got, ref64)
    assert more == 0, (what, dt, f"{more} of {got.size} elements more than one position from the rounded float64 value")
    assert one <= math.ceil(cap * got.size) + 2, (what, dt, f"{one} of {got.size} elements one position off (cap {cap:.2e})")


def assert_equal(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(bad) == 0, (what, f"{len(bad)} of {got.size} elements differ; first at {bad[:4].tolist()}: "
                                 f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def assert_within(got, ref, bound, what=""):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    err = np.abs(got - ref)
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, (what, f"{len(bad)} of {got.size} elements beyond the bound; first at {bad[:4].tolist()}: err "
                                 f"{err[tuple(bad[0])]:.3e} > {np.broadcast_to(bound, err.shape)[tuple(bad[0])]:.3e}")


# ---- fragment-major image ------------------------------------------------------------------------------------------------------------
def frag_index(n, k, K):
    """element (n, k) of a [N][K] matrix in the packed image (csrc/common.h: frag_index)"""
    return (((n >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (n & 15)) * 8 + (k & 7)


def pack_source_bits(N, K):
    """16-bit patterns that are finite, normal numbers in bf16 and in f16 and differ between neighbours in n and in k"""
    n, k = np.meshgrid(np.arange(N, dtype=np.int64), np.arange(K, dtype=np.int64), indexing="ij")
    return (0x0400 + (n * 1283 + k * 17 + (n >> 4) * 7919) % 0x7000).astype(np.uint16)


def wfrag_image(src, N, K, fault=None):
    """the image of [ceil(N / 16) * 16][K] elements: pad rows repeat the last row"""
    src = np.asarray(src)
    Np = (N + 15) & ~15
    n, k = np.meshgrid(np.arange(Np, dtype=np.int64), np.arange(K, dtype=np.int64), indexing="ij")
    img = np.zeros(Np * K, src.dtype)
    val = src[np.minimum(n, N - 1), k]
    if fault == "pad_row_zero":
        val = np.where(n < N, val, 0).astype(src.dtype)
    img[frag_index(n, k, K)] = val
    return img


# ---- the stacked GEMV ----------------------------------------------------------------------------------------------------------------
def stack_blocks(nt, n_tiles, seg_nt):
    """the launcher's choice (csrc/decfuse.hip: cw_launch_gemv_stack): nt = 0 -> the smallest of 1 .. 3 that keeps the launch within
    256 blocks; a segment asks for fewer tiles per block through its own nt.  -> (launch nt, per-segment nt, per-segment blocks)"""
    def per_seg(t):
        return [s if 0 < s < t else t for s in seg_nt]
    if nt <= 0:
        nt = 1
        while True:
            if sum(-(-n // s) for n, s in zip(n_tiles, per_seg(nt))) <= 256 or nt == 3:
                break
            nt += 1
    snt = per_seg(nt)
    return nt, snt, [-(-n // s) for n, s in zip(n_tiles, snt)]


def row_mean_switch(x):
    """mu [rows]: the float64 row mean where 2 mu^2 >= E[x^2] (|mean| >= std), else 0"""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1)
    return np.where(2 * mu * mu >= (x * x).mean(-1), mu, 0.0)


def switch_ratio(x):
    x = np.asarray(x, np.float64)
    return 2 * x.mean(-1) ** 2 / np.maximum((x * x).mean(-1), 1e-300)


def grid12(v, fault=None):
    """the 2^-12 residual grid: rint(v 4096) / 4096, ties to even"""
    t = np.asarray(v, np.float64) * 4096.0
    if fault == "grid_half_away":
        return np.copysign(np.floor(np.abs(t) + 0.5), t) / 4096.0
    return np.rint(t) / 4096.0


def planes_of(v, cols):
    """[groups][blocks][16][2]: (sum, sum of squares) of every row of v [Mb][n] over blocks of `cols` columns; rows beyond Mb: 0"""
    v = np.asarray(v, np.float64)
    Mb, n = v.shape
    idx = np.arange(0, n, cols)
    groups = (Mb + 15) // 16
    ps = np.zeros((groups * 16, len(idx), 2))
    ps[:Mb, :, 0] = np.add.reduceat(v, idx, axis=1)
    ps[:Mb, :, 1] = np.add.reduceat(v * v, idx, axis=1)
    return ps.reshape(groups, 16, len(idx), 2).transpose(0, 2, 1, 3).copy()


def stack_ref(dt, W, segs, Mb, nt=0, fault=None, round_x=True):
    """Reference of one launch.  W [sum n_tiles * 16][K]; segs: dicts with x [>= Mb][K], n_tiles, epi, optional bias, wsum, resid,
    nt, out0 (initial contents of an accumulating buffer; segments that share one list the same key `acc`).  Per segment
        epi 0 / 2   v = round16(x - mu) round16(W)^T + bias + mu wsum       (mu = row_mean_switch(x) with wsum, else 0)
        epi 1       v = resid + grid12(round16(x) round16(W)^T + bias);  pstats[group][block][row][0 / 1] = sum / sum of squares of
                    v over the block's columns, rows beyond Mb: 0
    round_x = False keeps x - mu of the centred rows (mu != 0) unrounded: the Gaussian comparison, whose bound carries that rounding.
    -> per segment a dict with out (epi 2: out0 plus every segment of the same `acc` key), pstats (epi 1), blocks, nt"""
    W16 = round16(dt, W)
    n_tiles = [s["n_tiles"] for s in segs]
    _, snt, blocks = stack_blocks(nt, n_tiles, [s.get("nt", 0) for s in segs])
    groups = (Mb + 15) // 16
    res, accs, t0 = [], {}, 0
    for si, s in enumerate(segs):
        n = s["n_tiles"] * 16
        Ws = W16[t0 * 16:t0 * 16 + n]
        t0 += s["n_tiles"]
        x = np.asarray(s["x"], np.float64)[:Mb]
        bias = np.zeros(n) if s.get("bias") is None else np.asarray(s["bias"], np.float64)
        mu = np.zeros(Mb)
        if s.get("wsum") is not None and fault != "no_centring":
            mu = row_mean_switch(x)
        xc = x - mu[:, None]
        acc = np.where((mu != 0)[:, None] & (not round_x), xc, round16(dt, xc)) @ Ws.T
        r = {"blocks": blocks[si], "nt": snt[si]}
        if s["epi"] == 1:
            v = np.asarray(s["resid"], np.float64)[:Mb] + grid12(acc + bias, fault)
            ps = planes_of(v, snt[si] * 16)
            if fault == "tail_clamped" and s["n_tiles"] % snt[si]:
                # the tail block also stores the tile it clamped its loads to (the segment's last): at the columns behind the row,
                # which are the head of the next row, and into its own partial sums
                v = v.copy()
                last = v[:, n - 16:].copy()
                spill = (blocks[si] * snt[si] - s["n_tiles"]) * 16
                for m in range(Mb - 1):
                    v[m + 1, :min(spill, 16)] = last[m, :min(spill, 16)]
                for m in range(Mb):
                    ps[m >> 4, -1, m & 15] += (last[m].sum(), (last[m] ** 2).sum())
            if fault == "pstats_group_stride_16" and groups > 1:
                flat = np.full(groups * blocks[si] * 32, np.nan)      # what no block wrote keeps what it held
                for gi in range(groups):
                    for j in range(blocks[si]):
                        o = (gi + j) * 32
                        flat[o:o + 32] = ps[gi, j].reshape(-1)
                ps = flat.reshape(ps.shape)
            r["out"], r["pstats"] = v, ps
        else:
            ws = np.zeros(n) if s.get("wsum") is None else np.asarray(s["wsum"], np.float64)
            if fault == "wsum_neighbour_tile":
                ws = np.roll(ws, -16)
            v = acc + bias + mu[:, None] * ws
            if s["epi"] == 2:
                key = s.get("acc", si)
                if key not in accs:
                    accs[key] = np.asarray(s["out0"], np.float64)[:Mb].copy()
                accs[key] += v
                r["out"] = accs[key]
            else:
                r["out"] = v
        res.append(r)
    return res


def stack_elem_bound(dt, W, seg, Mb, ref_out):
    """Derived bound of one segment's Gaussian comparison: the f32 accumulation 2 K 2^-24 sum |x16 w16| over the operand the kernel
    rounds (x, or x - mu); for centred rows the 16-bit rounding of the unrounded reference operand, 1/2 sum |w16| ulp16(x - mu) (the
    f32 mean may differ from the float64 one by 2^-20 |mu|, which can lift an element into the next binade); the product mu wsum and
    the f32 value of wsum, 2^-22 |mu wsum|; the final additions, 2^-23 |result|; epi 1: half a grid step, 2^-13."""
    W16 = np.abs(round16(dt, W))
    x = np.asarray(seg["x"], np.float64)[:Mb]
    K = x.shape[1]
    mu = row_mean_switch(x) if seg.get("wsum") is not None else np.zeros(Mb)
    xc = x - mu[:, None]
    b = 2 * K * U32 * (np.abs(round16(dt, xc)) @ W16.T) + 2 * U32 * np.abs(ref_out)
    cen = mu != 0
    if cen.any():
        b[cen] += 0.5 * (ulp16(dt, np.abs(xc[cen]) + 2.0 ** -20 * np.abs(mu[cen])[:, None]) @ W16.T)
        b[cen] += 4 * U32 * np.abs(mu[cen])[:, None] * np.abs(np.asarray(seg["wsum"], np.float64))
    if seg["epi"] == 1:
        b = b + 2.0 ** -13
    return b


# exact operands ------------------------------------------------------------------------------------------------------------------------
CENTRE_OFFSET = 5000.0      # not a neighbour of 5000 +- 4 in bf16 (spacing 32) or f16 (spacing 4)
STACK_K = {128: (8, 5, 7), 384: (24, 25, 10), 1280: (80, 80, 80)}   # K -> tiles of the three segments (a tail tile at nt = 2 or 3 in each K)
STACK_MB = [1, 7, 8, 9, 16, 17, 33, 64]
STACK_NT = [1, 2, 3, 0]
STACK_X2_TILES = {128: (32, 32, 8), 1280: (320, 320, 80)}           # [W'1 ; W'1 Wo_c ; Wo_c]: ffn_dim = 4 d_model; nt = 0 chooses 3 at 1280


def centred_rows(Mb):
    """rows that carry the offset: every third one, so that centred and plain rows share a wave (2 or 4 rows per wave) and a launch"""
    return np.arange(Mb) % 3 == 1


def stack_exact_case(K, tiles, layout, seed=0, rows=64):
    """Operands of an exact launch in the engine's X1 layout (epilogues 0, 0, 1: qa = W'q x + bias with centring, qb = (W'q Wo) a, x1
    = x + grid(Wo a + bo) with planes) or X2 layout (2, 2, 1: the two halves of u1 accumulate into one buffer that holds small numbers,
    x2 with a second copy, and a buffer to clear).
      x rows: ints in [-4, 4]; centred rows: CENTRE_OFFSET + zero-sum ints in [-4, 4]
      W: ints in [-2, 2] over 16; bias: ints / 16; epi 1 bias: ints / 16 +- 2^-13, which puts (acc + bias) 4096 on a tie whose even
      neighbour is the multiple of 256 -- up for -, down for + -- so the result stays on the 1 / 16 grid and the sums of squares exact
      wsum: the row sums of W (exact: multiples of 1 / 16), resid: ints / 16
    -> W [sum tiles * 16][K], segs (x for `rows` rows), extras dict"""
    rng = np.random.default_rng([41, K, sum(tiles), 0 if layout == "x1" else 1, seed])
    W = rng.integers(-2, 3, (sum(tiles) * 16, K)) / 16.0
    xa = rng.integers(-4, 5, (rows, K)).astype(np.float64)
    d = rng.integers(-4, 5, (rows, K)).astype(np.float64)
    d[:, 0] = 0
    tot = d.sum(-1)                                              # spread -tot over the row in steps of +-1 where that keeps |d| <= 4
    for m in range(rows):
        k, step = 1, -np.sign(tot[m])
        while tot[m] != 0:
            if abs(d[m, k] + step) <= 4:
                d[m, k] += step
                tot[m] += step
            k = k + 1 if k + 1 < K else 1
    cen = centred_rows(rows)
    x0 = np.where(cen[:, None], CENTRE_OFFSET + d, xa)
    xb = rng.integers(-4, 5, (rows, K)).astype(np.float64)       # the attention output rows
    n0, n1, n2 = (t * 16 for t in tiles)
    wsum0 = W[:n0].sum(-1)
    tie = rng.choice([-1.0, 0.0, 0.0, 1.0], n2) * 2.0 ** -13
    bias2 = rng.integers(-32, 33, n2) / 16.0 + tie
    resid = rng.integers(-64, 65, (rows, n2)) / 16.0
    seg0 = {"x": x0, "bias": rng.integers(-32, 33, n0) / 16.0, "wsum": wsum0, "n_tiles": tiles[0]}
    seg1 = {"x": xb, "bias": None, "n_tiles": tiles[1]}
    seg2 = {"x": xb, "bias": bias2, "resid": resid, "n_tiles": tiles[2], "epi": 1}
    if layout == "x1":
        seg0["epi"] = seg1["epi"] = 0
    else:
        assert tiles[0] == tiles[1]
        out0 = rng.integers(-64, 65, (rows, n0)) / 16.0
        seg0.update(epi=2, acc="u1", out0=out0)
        seg1.update(epi=2, acc="u1", out0=out0)
    return W, [seg0, seg1, seg2], {"tie_columns": tie != 0}


def stack_exactness_margins(dt, W, segs, Mb):
    """Sufficient conditions for every f32 partial sum of the exact launch to be exact in ANY order: all terms of a sum are multiples
    of one granule g and sum |terms| / g < 2^24.  -> the largest sum |terms| / g over products (g = 2^-4), back-added means (2^-4),
    residual results (2^-4; ties resolve onto that grid), plane sums (2^-4) and plane sums of squares (2^-8), each to stay below 2^24"""
    res = stack_ref(dt, W, segs, Mb, nt=1)
    worst, t0 = 0.0, 0
    for s, r in zip(segs, res):
        n = s["n_tiles"] * 16
        Ws = np.abs(W[t0 * 16:t0 * 16 + n])
        t0 += s["n_tiles"]
        x = np.asarray(s["x"], np.float64)[:Mb]
        mu = row_mean_switch(x) if s.get("wsum") is not None else np.zeros(Mb)
        bias = np.zeros(n) if s.get("bias") is None else np.abs(s["bias"])
        back = np.abs(mu[:, None] * (np.zeros(n) if s.get("wsum") is None else np.asarray(s["wsum"])))
        total = np.abs(x - mu[:, None]) @ Ws.T + bias + back        # every term of the products, the bias and the mean added back
        worst = max(worst, float(np.abs(x).sum(-1).max()))           # the integer row sum the mean is taken of
        if s["epi"] == 1:
            v = r["out"]
            assert np.array_equal(v * 16, np.rint(v * 16)), "epi 1 results leave the 1 / 16 grid"
            vt = v.reshape(Mb, -1, 16)                               # a block sums at most three 16-column tiles
            worst = max(worst, float(total.max()) * 2 ** 13,         # acc + bias carries the 2^-13 tie offsets
                        3 * float(np.abs(vt).sum(-1).max()) * 16, 3 * float((vt * vt).sum(-1).max()) * 256)
        else:
            if s["epi"] == 2:                                        # two such segments and the buffer's contents add up
                total = 2 * total + np.abs(s["out0"][:Mb])
            worst = max(worst, float(total.max()) * 16)
    return worst


def stack_f32_restatement(dt, W, segs, Mb, nt, order):
    """The exact launch evaluated in float32 in one of two summation orders (0: left to right, 1: right to left, K in two halves
    added at the end); used with exact operands only, where it has to agree with the float64 reference bit for bit"""
    f = np.float32
    _, snt, blocks = stack_blocks(nt, [s["n_tiles"] for s in segs], [s.get("nt", 0) for s in segs])
    W16 = round16(dt, W).astype(f)
    outs, t0, accs = [], 0, {}

    def dot(a, b):
        K = a.shape[1]
        if order == 0:
            acc = np.zeros((a.shape[0], b.shape[0]), f)
            for k0 in range(0, K, 64):
                acc = (acc + a[:, k0:k0 + 64] @ b[:, k0:k0 + 64].T).astype(f)
            return acc
        h = K // 2
        lo = np.zeros((a.shape[0], b.shape[0]), f)
        hi = np.zeros_like(lo)
        for k0 in range(h - 64, -1, -64):
            lo = (lo + a[:, k0:k0 + 64][:, ::-1] @ b[:, k0:k0 + 64][:, ::-1].T).astype(f)
        for k0 in range(K - 64, h - 1, -64):
            hi = (hi + a[:, k0:k0 + 64][:, ::-1] @ b[:, k0:k0 + 64][:, ::-1].T).astype(f)
        return (hi + lo).astype(f)

    for si, s in enumerate(segs):
        n = s["n_tiles"] * 16
        Ws = W16[t0 * 16:t0 * 16 + n]
        t0 += s["n_tiles"]
        x = np.asarray(s["x"], f)[:Mb]
        K = x.shape[1]
        mu = np.zeros(Mb, f)
        if s.get("wsum") is not None:
            xs = x if order == 0 else x[:, ::-1]
            m1 = (np.cumsum(xs, -1, dtype=f)[:, -1] / f(K)).astype(f)
            m2 = (np.cumsum(xs * xs, -1, dtype=f)[:, -1] / f(K)).astype(f)
            mu = np.where(f(2) * m1 * m1 < m2, f(0), m1).astype(f)
        xr = round16(dt, (x - mu[:, None]).astype(f)).astype(f)
        acc = dot(xr, Ws)
        bias = np.zeros(n, f) if s.get("bias") is None else np.asarray(s["bias"], f)
        r = {}
        if s["epi"] == 1:
            v = (np.asarray(s["resid"], f)[:Mb] + (np.rint((acc + bias).astype(f) * f(4096)) * f(1 / 4096)).astype(f)).astype(f)
            groups = (Mb + 15) // 16
            ps = np.zeros((groups, blocks[si], 16, 2), f)
            cols = snt[si] * 16
            for j in range(blocks[si]):
                blk = v[:, j * cols:min((j + 1) * cols, n)]
                if order == 1:
                    blk = blk[:, ::-1]
                s1 = np.cumsum(blk, -1, dtype=f)[:, -1]
                s2 = np.cumsum((blk * blk).astype(f), -1, dtype=f)[:, -1]
                for m in range(Mb):
                    ps[m >> 4, j, m & 15] = (s1[m], s2[m])
            r["out"], r["pstats"] = v, ps
        else:
            ws = np.zeros(n, f) if s.get("wsum") is None else np.asarray(s["wsum"], f)
            back = (mu[:, None] * ws).astype(f)
            v = ((acc + bias).astype(f) + back).astype(f) if order == 0 else (acc + (bias + back).astype(f)).astype(f)
            if s["epi"] == 2:
                key = s.get("acc", si)
                if key not in accs:
                    accs[key] = np.asarray(s["out0"], f)[:Mb].copy()
                accs[key] = (accs[key] + v).astype(f)
                r["out"] = accs[key]
            else:
                r["out"] = v
        outs.append(r)
    for si, s in enumerate(segs):                                # an accumulating buffer: its final contents
        if s["epi"] == 2:
            outs[si]["out"] = accs[s.get("acc", si)]
    return outs


# Gaussian operands ----------------------------------------------------------------------------------------------------------------------
STACK_GAUSS_MB = [5, 40]
GAUSS_OFFSET, GAUSS_SPREAD = 100.0, 0.5     # centred rows: offset 200 spreads (test_decode_stage_refs.py: without centring 90 % of them fail)


def stack_gauss_case(dt, Mb, seed=0):
    """X1 layout at K = 1280, 80 tiles per segment: W ~ 0.05 N(0, 1), x rows N(0, 1), every third row GAUSS_OFFSET + GAUSS_SPREAD
    N(0, 1); wsum = the float32 row sums of the rounded weights; the attention rows N(0, 1); resid on the 2^-12 grid."""
    rng = np.random.default_rng([43, Mb, seed])
    K, t = 1280, 80
    f = np.float32
    W = (0.05 * rng.standard_normal((3 * t * 16, K))).astype(f).astype(np.float64)
    x = rng.standard_normal((Mb, K))
    cen = centred_rows(Mb)
    x[cen] = GAUSS_OFFSET + GAUSS_SPREAD * x[cen]
    x = x.astype(f).astype(np.float64)
    xb = rng.standard_normal((Mb, K)).astype(f).astype(np.float64)
    n = t * 16
    wsum = rowsum64(dt, W[:n]).astype(f).astype(np.float64)
    resid = np.rint(rng.standard_normal((Mb, n)) * 4096) / 4096
    segs = [{"x": x, "bias": (0.1 * rng.standard_normal(n)).astype(f).astype(np.float64), "wsum": wsum, "n_tiles": t, "epi": 0},
            {"x": xb, "bias": None, "n_tiles": t, "epi": 0},
            {"x": xb, "bias": (0.1 * rng.standard_normal(n)).astype(f).astype(np.float64), "resid": resid, "n_tiles": t, "epi": 1}]
    return W, segs


def pstats_bound(out_ref, out_bound, snt, blocks, Mb):
    """planes of the Gaussian launch: the sums are taken of the kernel's own f32 results, each within out_bound of the reference; f32
    summation of <= 48 terms adds 48 2^-24 sum |.|"""
    groups = (Mb + 15) // 16
    b = np.zeros((groups, blocks, 16, 2))
    cols = snt * 16
    n = out_ref.shape[1]
    for j in range(blocks):
        sl = slice(j * cols, min((j + 1) * cols, n))
        a, e = np.abs(out_ref[:, sl]), out_bound[:, sl]
        for m in range(Mb):
            b[m >> 4, j, m & 15] = (e[m].sum() + 48 * U32 * a[m].sum(),
                                    (2 * a[m] * e[m] + e[m] ** 2).sum() + 49 * U32 * ((a[m] + e[m]) ** 2).sum())
    return b


# ---- the query the cross-attention kernels finish ---------------------------------------------------------------------------------------
XQ_S = 384                                  # 6 splits of 64 keys: key k of every head is the unit vector e_(k mod 64)
XQ_SPLIT_H = [2, 6, 20]
XQ_SPLIT_B = [1, 8, 16, 17, 64]
XQ_SPLIT_NP = [1, 27, 40, 64, 65, 80, 128]
XQ_BEAM_DIV = [2, 5, 16]
XQ_BEAM_NP = [1, 33, 65, 80, 96]
XQ_QMAX = 4.0


def onehot_cache(Bk, H):
    """K = V [Bk][H][XQ_S][64]: row k is e_(k mod 64) -- exact in every type, e4m3 included (scale 1 / 448)"""
    kv = np.zeros((Bk, H, XQ_S, 64), np.float32)
    kv[:, :, np.arange(XQ_S), np.arange(XQ_S) % 64] = 1.0
    return kv


def readout_query(part_o, part_ml):
    """q[b][h][split][j] = m + log(part_o[split][b][h * 64 + j]): with the one-hot caches every split holds exp(q_j - m) and its max"""
    NS, B, D = part_o.shape
    H = D // 64
    po = np.asarray(part_o, np.float64).reshape(NS, B, H, 64).transpose(1, 2, 0, 3)
    m = np.asarray(part_ml, np.float64)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return m[..., None] + np.log(po)


def finish_query64(qa, qb, qw, qbias, pstats, n_pstats, cut=None):
    """q = rstd (qa + qb - mean qw) + qbias with mean = sum ps1 / D, var = max(sum ps2 / D - mean^2, 0), rstd = 1 / sqrt(var + 1e-5),
    the sums over the n_pstats plane slots of the row's group.  cut: a consumer that stops at that many slots.
    -> q [B][D], (mean, var, ex2) [B]"""
    qa, qb, qw, qbias = (np.asarray(t, np.float64) for t in (qa, qb, qw, qbias))
    ps = np.asarray(pstats, np.float64).reshape(-1, n_pstats, 16, 2)
    B, D = qa.shape
    n = n_pstats if cut is None else min(n_pstats, cut)
    b = np.arange(B)
    s = ps[b >> 4, :n, b & 15].sum(1)                            # [B][2]
    mean = s[:, 0] / D
    ex2 = s[:, 1] / D
    var = np.maximum(ex2 - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    return rstd[:, None] * (qa + qb - mean[:, None] * qw) + qbias, (mean, var, ex2)


def fused_query_case(B, H, n_pstats, seed=0):
    """Inputs whose float64-finished query is a given target with |q| <= XQ_QMAX.  Per row a LayerNorm-like mean and standard
    deviation (|mean| << std; row B // 2: mean = 30 std), planes of n_pstats slots that add up to D mean and D (var + mean^2) -- slot
    sums of tiles of such a row -- qw in [-1/16, 1/16] (30 std |qw| stays next to the query, so that the f32 subtraction of mean qw
    costs no more than the rounding of the query itself), qb = a quarter to a half of the un-normalised query, qa the rest.  Rows
    beyond B of the last group's planes hold NaN.  -> qa, qb, qw, qbias (float32), pstats [groups][n_pstats][16][2] (float32)"""
    rng = np.random.default_rng([47, B, H, n_pstats, seed])
    D = H * 64
    f = np.float32
    std = rng.uniform(0.5, 2.0, B)
    mean = rng.uniform(-0.05, 0.05, B) * std
    mean[B // 2] = 30.0 * std[B // 2]
    groups = (B + 15) // 16
    ps = np.full((groups, n_pstats, 16, 2), np.nan)
    cols = D / n_pstats                                          # columns per slot (need not be whole: only the sums matter)
    for b in range(B):
        s1 = cols * mean[b] + math.sqrt(cols) * std[b] * rng.standard_normal(n_pstats)
        s1 += (D * mean[b] - s1.sum()) / n_pstats
        s2 = cols * (std[b] ** 2 + mean[b] ** 2) * rng.uniform(0.8, 1.2, n_pstats)
        s2 *= D * (std[b] ** 2 + mean[b] ** 2) / s2.sum()
        if b == B // 2:
            # the offset row: E[x^2] / var = 901 magnifies every rounding of the two sums, and the tolerance's variance term pays for
            # the roundings of sum / D and mean^2 only -- so this row's slots lie on a grid on which any f32 summation order is exact
            for s in (s1, s2):
                s[:] = np.rint(np.ldexp(s, 23 - math.frexp(np.abs(s).sum())[1])) * 2.0 ** (math.frexp(np.abs(s).sum())[1] - 23)
        ps[b >> 4, :, b & 15, 0], ps[b >> 4, :, b & 15, 1] = s1, s2
    ps = ps.astype(f)
    qw = rng.uniform(-1 / 16, 1 / 16, D).astype(f)
    qbias = rng.uniform(-0.5, 0.5, D).astype(f)
    target = rng.uniform(-(XQ_QMAX - 0.6), XQ_QMAX - 0.6, (B, D))
    # the statistics the consumer will see: those of the float32 planes
    _, (m64, v64, _) = finish_query64(np.zeros((B, D)), np.zeros((B, D)), qw, qbias, ps, n_pstats)
    u = (target - qbias) * np.sqrt(v64 + 1e-5)[:, None] + m64[:, None] * qw
    qb = (u * rng.uniform(0.25, 0.5, (B, D))).astype(f)
    qa = (u - qb).astype(f)
    return qa, qb, qw, qbias, ps


def fused_query_tol(yardstick, q_ref, qbias, var, ex2):
    """4 x the readback error of a finished query through the same kernel family (the factor leaves room for the f32 evaluation of the
    finishing formula on top of the same exponentials) + 2^-23 E[x^2] / (2 var) |q - qbias|: var = E[x^2] - mean^2 is taken in f32,
    and a relative error of var is half that of rstd"""
    return 4 * yardstick + 2.0 ** -23 * (ex2 / (2 * np.maximum(var, 1e-30)))[:, None] * np.abs(q_ref - np.asarray(qbias, np.float64))


def assert_query(readout, q_ref, tol, what=""):
    """readout [B][H][6][64] against q_ref [B][H * 64], tol [B][H * 64]: every split of every (row, head) carries the whole query"""
    B, H, NS, _ = readout.shape
    assert np.isfinite(readout).all(), (what, "non-finite readout", np.argwhere(~np.isfinite(readout))[:4].tolist())
    err = np.abs(readout - q_ref.reshape(B, H, 1, 64))
    bad = np.argwhere(err > tol.reshape(B, H, 1, 64))
    assert len(bad) == 0, (what, f"{len(bad)} of {err.size} query elements beyond the tolerance; first (row, head, split, column) "
                                 f"{bad[:4].tolist()}: err {err[tuple(bad[0])]:.3e} > {np.broadcast_to(tol.reshape(B, H, 1, 64), err.shape)[tuple(bad[0])]:.3e}")
