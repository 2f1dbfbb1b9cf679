"""The fused BRDF MLP (nmf_amd/csrc/brdf_mlp.hip) without a GPU: the inputs, the float64 references, the fp32 restatement of the
kernels' arithmetic and the margins that the GPU tests (tests/test_hip_brdf_mlp.py) hold nmf_brdf_mlp_fwd / nmf_brdf_mlp_bwd_segments to --
and the tests that show that the inputs enter the tile loops they are named for and that the margins are not blind.

Ray counts and grids (CASES; a wave owns a 32-ray tile, 4 waves per workgroup, a wave walks tiles wave, wave + 4 grid, ...):
    R = 1, 31, 32, 33   max_workgroups 0   waves with no tile; a full / a ragged single tile; clamped lanes rc = R - 1
    R = 421             max_workgroups 1   14 tiles: waves 0-1 take 4, waves 2-3 take 3, the last tile has 5 rays
    R = 513             max_workgroups 2   17 tiles on 8 waves (3, 2, 2, ...), the last tile has one ray
    R = 997             max_workgroups 1   32 tiles, 8 per wave (the depth of a training step), the last tile has 5 rays
    R = 2049            max_workgroups 0   65 tiles: forward 17 workgroups, backward cdiv(65, 8) = 9: waves with 2 tiles and with 1
test_tiles_per_wave_are_what_the_cases_are_named_for restates the grid formulas and holds them to that table.

Rows: src_idx is non-decreasing in runs of 1, 31, 32, 33, 70, 1, ... rays (runs start, end and straddle at tile edges and span tiles
of different waves); feature rows 1 and M - 1 are gathered by no ray.  rough is exactly 0.01 on the first gathered row, 1.0 on the
second, uniform between on the others.  The src_idx = None form gets the gathered rows, one per ray: the same numbers per ray.

Weight sets: "golden" (tests/golden/shading_parts.npz: |W| <= 0.31, biases <= 0.027) and "wide" (W ~ N(0, 0.5^2), b ~ N(0, 1): the
b0 column COL_BIAS, b2 and b4 weigh in every metric).  W4 / b4 have four rows, the kernels read three: the float64 autograd gives
zeros for the fourth, so gW4[3] / gb4[3] keep what was in them.

Conditioning is constructed: a ray's half and diff vectors are redrawn until each of its 128 float64 pre-activations is CLEAR[set]
[layer] from zero; CLEAR is a power of two between 32 x and 128 x the largest pre-activation error of the forward restatement
(test_clear_is_32_to_128_restatement_errors; errors 1.5e-6 / 8.6e-7 golden, 3.7e-6 / 1.1e-5 wide).  The GPU tests then compare the
forward's masks bit for bit on every ray and every gradient element.  Share of rays redrawn on the first pass, all cases of a set
together (test_redraw_share; cap 5 %): golden 0.69 %, wide 1.23 %.

References (float64 on the fp32 inputs): oracle.brdf_mlp and its autograd; forward64() -- the same network on the kernels' 80-column
input image, which also gives the pre-activations and the masks in the kernels' [R, 4] layout -- and backward64_given(), which takes
the masks as given the way the kernel defines it (H1 = m1 ? a1 : 0, dW4 from relu(H1 W2^T + b2) by sign, dH2 = m2 ? g W4 : 0,
dH1 = m1 ? dH2 W2 : 0).  test_references_agree: the three agree where they overlap.

Restatement (numpy float32): split() = bf16 round-to-nearest-even planes; product() = the kernels' `product`: per K block of 16 the
six (forward, three planes) or three (backward, two planes) plane products smallest first, each added to an fp32 accumulator (the
16-term dot product of an instruction carried exactly); the VALU output layer per lane half in unit order and the sigmoid with a
correctly rounded exp; backward32(): per tile what k_brdf_mlp_bwd does, the weight-gradient accumulators of a wave carried in
fp32 over its tiles, waves of a workgroup added in order, workgroups in the order of k_brdf_mlp_reduce, then one add per gradient
element into what was there (gW4, gb2: the two lane halves one after the other; gb4: the 32 ray lanes in order).

Margins (margins() of tests/test_shading_rows_cpu.py): per metric and case 8 x the restatement's largest error against float64, at
least 2^-23 x the largest |reference|.  Metrics: out, d_feat, gW0, gb0, gW2, gb2, gW4, gb4; the gradients are compared as
PATTERN + gradient (the buffers are accumulated into).  No margin is looser than tests/test_hip_parity.py's tolerance for the same
quantity: where 8 x the error exceeds it the tolerance is the margin (13 of 472, none of them a given-mask case: `out` of the wide
set from 31 rays on, where the restatement's error reaches 0.24 of the tolerance, d_feat of the golden set at 33 rays;
test_margins_are_not_looser_than_the_fp32_test, which also holds the restatement itself to a quarter of its own margin and to half
of a capped one).  Two margins leave little room and are deterministic: the restatement at 0.24 of the capped `out` margin (wide,
2049 rays) and the kernel at 0.91 of the `out` margin of the wide set at 33 rays, where the restatement's largest error over 99
elements is a tenth of what it is at 31 and 32 rays.

Given masks (R = 421, wide weights): all ones, all zeros, alternating, and sixteen single-unit cases, one per 4-bit group of a
layer's mask bits, margins per metric and case like the others.  A single-unit case leaves ONE element of gW2, gb2 and gb0, a sum
over the rays of terms of both signs.  single_units() takes, of the 4 x 4 positions inside the two groups, the pair whose lone sums
cancel least (condition numbers 7 to 19 in float64).  The restatement's error on one element is the luck of one rounding sequence,
not a largest error, so for these three metrics alone the sixteen cases share a margin: 8 x their largest RELATIVE error times the
case's scale, capped like every other -- it stays below 1 % of the scale, a unit on the wrong bit is an error of 100 %, and the
restatement with swapped bit groups misses it (test_given_masks).

The margins are not blind (test_broken_restatements_miss_their_margins; error / margin of the restatement broken on purpose, wide
weights, R = 421 on one workgroup unless named):
    1 forward on two bf16 terms (three products)          out 7.9 (golden weights: 4.3)
    2 the next tile's inputs used for the current tile    out 9.4e+04
    3 clamped lanes counted in the weight gradients       gW0 8.4e+03  gb0 8.9e+03  gW2 1.1e+04  gb2 1.7e+04  gW4 1.3e+04  gb4 5.4e+04
    4 a wave's accumulators keep only its last tile       gW0 1.7e+04  gb0 1.8e+04  gW2 1.4e+04  gb2 2.6e+04  gW4 2.0e+04  gb4 9.8e+04
    5 the two 4-bit lane-half groups of a mask byte       d_feat 2.8e+04  gW0 2.0e+04  gb0 2.9e+04  gW2 2.8e+04  gb2 4.5e+04  gW4 2.1e+04
      swapped (backward)                                  (gb4 0.12: it does not read the masks)
    6 the b0 column dropped                               out 9.4e+04
    7 input columns 61-65 of gW0 left at zero             gW0 1.0e+04
    8 set 1's tiles read set 0's d_out (421 + 37 rays)    d_feat1 2.5e+04  gW0 5.3e+03  gb0 4.6e+03  gW2 6.1e+03  gb2 9.4e+03  gW4 6.2e+03
                                                          gb4 2.7e+04  (d_feat0 0.12: set 0 is untouched)
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import Golden
from oracle import nmf_oracle as O
from test_shading_rows_cpu import FLOOR, _big, _ro, errors_over, margins

F32, F64 = np.float32, np.float64
RT, WAVES, GRID_CAP = 32, 4, 256                  # brdf_mlp.hip: rays per wave tile, waves per workgroup, one workgroup per CU
BWD_TILES_PER_WAVE = 2                            # bwd_grid_tiles: short launches give every wave at least two tiles
CASES = ((1, 0), (31, 0), (32, 0), (33, 0), (421, 1), (513, 2), (997, 1), (2049, 0))        # (R, max_workgroups)
WEIGHTS = ("golden", "wide")
FORMS = ("rows", "rays")                          # src_idx given / None (one feature row per ray)
RUNS = (1, 31, 32, 33, 70)
PAIRS = ((421, 37), (33, 997), (1, 1))            # two ray sets in one launch, max_workgroups = 1
OUT_BIAS = float(F32(0.37))
MIN_ROUGH = F32(0.01)
ORDER = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias")
GRADS = ("gW0", "gb0", "gW2", "gb2", "gW4", "gb4")
METRICS = ("out", "d_feat") + GRADS
# the distance every pre-activation keeps from zero in float64: (layer 1, layer 2) per weight set
CLEAR = {"golden": (2.0 ** -14, 2.0 ** -14), "wide": (2.0 ** -12, 2.0 ** -10)}
REDRAW_CAP = 0.05
# input columns of the LDS image (brdf_mlp.hip): 0-20 half vector (18 ISH + xyz) | 21-44 features | 45 = 1.0 (b0) | 46-47 zero |
# 48-68 diff vector (18 ISH + xyz) | 69-79 zero
NCOL, COL_FEAT, COL_BIAS, COL_DIFF = 80, 21, 45, 48
TERMS = {2: ((1, 0), (0, 1), (0, 0)), 3: ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))}      # (A plane, B plane), smallest first
FAULTS = ("two_terms", "cur_nxt", "clamped", "last_tile", "nibbles", "no_b0", "no_tail", "d_out_of_set0")


def col_orig(c):
    """image column -> column of W0 / gW0, -1 = the bias column, -2 = padding"""
    if c < COL_FEAT:
        return 24 + c
    if c < COL_BIAS:
        return c - COL_FEAT
    if c == COL_BIAS:
        return -1
    return c - 3 if COL_DIFF <= c < COL_DIFF + 21 else -2


COL_ORIG = np.array([col_orig(c) for c in range(NCOL)])


def cdiv(a, b):
    return -(-a // b)


# ---- grids ------------------------------------------------------------------------------------------------------------------------------
def fwd_grid(R, max_workgroups):
    cap = max_workgroups if 0 < max_workgroups < GRID_CAP else GRID_CAP
    return min(cdiv(cdiv(R, RT), WAVES), cap)


def bwd_grid(tiles, max_workgroups):
    cap = max_workgroups if 0 < max_workgroups < GRID_CAP else GRID_CAP
    return min(cdiv(tiles, WAVES * BWD_TILES_PER_WAVE), cap)


def tiles_per_wave(tiles, grid):
    return [len(range(wave, tiles, grid * WAVES)) for wave in range(grid * WAVES)]


# ---- weights and inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(name):
    """(W0 [64, 66], b0, W2 [64, 64], b2, W4 [4, 64], b4) float32, read-only"""
    if name == "golden":
        g = Golden("shading_parts")
        ws = [g.np("brdf_param/mlp." + k).astype(F32) for k in ORDER]
    else:
        rng = np.random.default_rng(41)
        ws = [(s * rng.standard_normal(shape)).astype(F32)
              for s, shape in ((0.5, (64, 66)), (1.0, (64,)), (0.5, (64, 64)), (1.0, (64,)), (0.5, (4, 64)), (1.0, (4,)))]
    for a in ws:
        a.setflags(write=False)
    return tuple(ws)


def w0_image(w):
    """W0 | b0 in the column order of the LDS image [64, 80]"""
    img = np.zeros((64, NCOL), dtype=F32)
    for c, co in enumerate(COL_ORIG):
        if co >= 0:
            img[:, c] = w[0][:, co]
        elif co == -1:
            img[:, c] = w[1]
    return img


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _ish64(d, kappa):
    return O.ish_basis((0, 1, 2, 4), torch.from_numpy(d.astype(F64)), torch.from_numpy(kappa)).numpy()


def _ish32(d, kappa):
    """ish18 of the kernel in float32, operation by operation (exp correctly rounded)"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    k = kappa + F32(1e-8)
    with np.errstate(all="ignore"):
        a1 = np.exp((F32(-1) / k).astype(F64)).astype(F32)
        a2 = np.exp((F32(-3) / k).astype(F64)).astype(F32)
    xx, yy, zz = x * x, y * y, z * z
    c1, c2 = F32(0.488603), F32(1.092548)
    o = [np.full_like(x, F32(0.28209479177387814)), -a1 * c1 * x, a1 * c1 * z, -a1 * c1 * y,
         a2 * c2 * y * x, -a2 * c2 * y * z, a2 * F32(0.315392) * (F32(3) * zz - F32(1)), -a2 * c2 * x * y,
         a2 * F32(0.546274) * (xx - yy),
         F32(2.50334) * x * y * (xx - yy), F32(-1.77013) * y * z * (F32(-3) * xx + yy),
         F32(0.946175) * x * y * (F32(7) * zz - F32(1)), F32(0.669047) * y * z * (F32(7) * zz - F32(3)),
         F32(3.70251) * (zz * zz) - F32(3.17358) * zz + F32(0.317358), F32(0.669047) * x * z * (F32(7) * zz - F32(3)),
         (F32(0.473087) * xx - F32(0.473087) * yy) * (F32(7) * zz - F32(1)), F32(1.77013) * x * z * (xx - F32(3) * yy),
         F32(0.625836) * (xx * xx) - F32(3.755016) * xx * yy + F32(0.625836) * (yy * yy)]
    return np.stack(o, 1).astype(F32)


def image(hv, dv, feat_rays, rough_rays, dtype):
    """the kernels' input image [R, 80] of a ray set: float64 through oracle.ish_basis, float32 as build_x computes it"""
    R = len(hv)
    X = np.zeros((R, NCOL), dtype=dtype)
    if dtype == F64:
        kappa = 1.0 / (rough_rays.astype(F64) + 1e-3)
        ish = _ish64
    else:
        kappa = (F32(1) / (rough_rays + F32(1e-3))).astype(F32)
        ish = _ish32
    X[:, 0:18], X[:, 18:21] = ish(hv, kappa), hv
    X[:, COL_FEAT:COL_BIAS] = feat_rays
    X[:, COL_BIAS] = 1
    X[:, COL_DIFF:COL_DIFF + 18], X[:, COL_DIFF + 18:COL_DIFF + 21] = ish(dv, kappa), dv
    return X


def forward64(w, X):
    """the network in float64 on an image -> out [R, 3], pre-activations a1, a2 [R, 64]"""
    W0, W2, b2, W4, b4 = w0_image(w).astype(F64), w[2].astype(F64), w[3].astype(F64), w[4].astype(F64), w[5].astype(F64)
    a1 = X @ W0.T
    a2 = np.maximum(a1, 0) @ W2.T + b2
    o = np.maximum(a2, 0) @ W4[:3].T + b4[:3] + OUT_BIAS
    return 1.0 / (1.0 + np.exp(-o)), a1, a2


def pack_masks(m1, m2):
    """two [R, 64] bool arrays -> [R, 4] uint32: {layer 1 units 0-31, 32-63, layer 2 units 0-31, 32-63}, unit u on bit u % 32"""
    bit = np.uint64(1) << np.arange(32, dtype=np.uint64)
    words = [(m[:, 32 * k:32 * k + 32].astype(np.uint64) * bit).sum(-1) for m in (m1, m2) for k in (0, 1)]
    return np.stack(words, 1).astype(np.uint32)


def unpack_masks(bits):
    b = np.asarray(bits).view(np.uint32).astype(np.uint64)
    m = ((b[:, :, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return m[:, :2].reshape(-1, 64), m[:, 2:].reshape(-1, 64)


@functools.lru_cache(maxsize=None)
def inputs(R, ws, salt=0):
    """a ray set: hv, dv [R, 3], feat [M, 24], rough [M], src_idx [R] (int32, runs of RUNS), d_out [R, 3], the gathered rows
    feat_rays / rough_rays of the src_idx = None form, and how many rays the first conditioning pass redrew; float32, read-only"""
    rng = np.random.default_rng([43, R, salt])
    lens = []
    while sum(lens) < R:
        lens.append(RUNS[(len(lens) + salt) % len(RUNS)])
    M = len(lens) + 2                                              # rows 1 and M - 1 are gathered by no ray
    src = np.repeat([k if k == 0 else k + 1 for k in range(len(lens))], lens)[:R].astype(np.int32)
    feat = rng.standard_normal((M, 24)).astype(F32)
    rough = rng.uniform(0.01, 1.0, M).astype(F32)
    rough[0] = MIN_ROUGH
    rough[min(2, M - 1)] = F32(1.0)
    hv, dv = _unit(rng.standard_normal((R, 3))), _unit(rng.standard_normal((R, 3)))
    w = weights(ws)
    first = None
    while True:
        _, a1, a2 = forward64(w, image(hv, dv, feat[src], rough[src], F64))
        bad = (np.abs(a1).min(1) < CLEAR[ws][0]) | (np.abs(a2).min(1) < CLEAR[ws][1])
        first = int(bad.sum()) if first is None else first
        if not bad.any():
            break
        n = int(bad.sum())
        hv[bad], dv[bad] = _unit(rng.standard_normal((n, 3))), _unit(rng.standard_normal((n, 3)))
    return _ro(SimpleNamespace(R=R, M=M, hv=hv, dv=dv, feat=feat, rough=rough, src_idx=src, feat_rays=feat[src], rough_rays=rough[src],
                               d_out=rng.standard_normal((R, 3)).astype(F32), redrawn=first, gathered=np.unique(src)))


def pattern():
    """what the gradient buffers hold before a launch: six arrays shaped like the weights, every entry non-zero and exact in fp32"""
    out = []
    for k, a in enumerate(weights("wide")):
        n = np.arange(a.size) + 5 * k
        out.append((((n * 7) % 17 - 8.5) / 128).astype(F32).reshape(a.shape))
    return out


def zeros():
    return [np.zeros_like(a) for a in weights("wide")]


# ---- float64 references -----------------------------------------------------------------------------------------------------------------
def _rows_of(d_rays, src, M):
    out = np.zeros((M, 24), dtype=F64)
    np.add.at(out, src, d_rays)
    return out


@functools.lru_cache(maxsize=None)
def reference64(R, ws, salt=0):
    """oracle.brdf_mlp on doubles and its autograd -> out, masks [R, 4] uint32, pre-activations, d_feat per ray and per row, the six
    weight gradients (gradient alone: no pattern)"""
    i, w = inputs(R, ws, salt), weights(ws)
    t = lambda a: torch.from_numpy(np.array(a, dtype=F64))      # noqa: E731
    sd = {"model.brdf.mlp." + k: t(a).requires_grad_(True) for k, a in zip(ORDER, w)}
    fr = t(i.feat_rays).requires_grad_(True)
    out = O.brdf_mlp(sd, O.Cfg(brdf_bias=OUT_BIAS), t(i.hv), t(i.dv), fr, t(i.rough_rays))
    g = torch.autograd.grad((out * t(i.d_out)).sum(), [fr] + [sd["model.brdf.mlp." + k] for k in ORDER])
    X = image(i.hv, i.dv, i.feat_rays, i.rough_rays, F64)
    out_img, a1, a2 = forward64(w, X)
    ref = {"out": out.detach().numpy(), "d_feat_rays": g[0].numpy(), "d_feat_rows": _rows_of(g[0].numpy(), i.src_idx, i.M)}
    ref.update({k: v.numpy() for k, v in zip(GRADS, g[1:])})
    return SimpleNamespace(X=X, a1=a1, a2=a2, out_img=out_img, m1=a1 > 0, m2=a2 > 0, masks=pack_masks(a1 > 0, a2 > 0), **ref)


def backward64_given(w, X, m1, m2, s, d_out):
    """the backward as the kernel defines it on GIVEN masks and forward output s, float64 -> d_feat_rays and the six gradients"""
    W0, W2, b2, W4 = w0_image(w).astype(F64), w[2].astype(F64), w[3].astype(F64), w[4].astype(F64)
    g = d_out.astype(F64) * s * (1 - s)
    H1 = np.where(m1, X @ W0.T, 0.0)
    v = np.maximum(H1 @ W2.T + b2, 0.0)
    dH2 = np.where(m2, g @ W4[:3], 0.0)
    dH1 = np.where(m1, dH2 @ W2, 0.0)
    dW0i = dH1.T @ X
    gW0 = np.zeros((64, 66))
    for c, co in enumerate(COL_ORIG):
        if co >= 0:
            gW0[:, co] = dW0i[:, c]
    gW4, gb4 = np.zeros((4, 64)), np.zeros(4)
    gW4[:3], gb4[:3] = g.T @ v, g.sum(0)
    return {"d_feat_rays": (dH1 @ W0)[:, COL_FEAT:COL_BIAS], "gW0": gW0, "gb0": dW0i[:, COL_BIAS], "gW2": dH2.T @ H1, "gb2": dH2.sum(0),
            "gW4": gW4, "gb4": gb4}


# ---- the fp32 restatement ---------------------------------------------------------------------------------------------------------------
def bf16(v):
    """round to nearest even to bfloat16, as float32"""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(F32)


def split(v, n):
    """v as n bf16 planes, each the rounding of what the ones before left over -> [n, ...]"""
    v = np.array(v, dtype=F32)
    planes = []
    for _ in range(n):
        p = bf16(v)
        planes.append(p)
        v = v - p
    return np.stack(planes)


def product(rays, units, rays_are_b, acc=None):
    """`product` of the kernel: acc[r, u] += sum_k rays[.][r, k] units[.][u, k], per K block of 16 the plane products of TERMS in
    order, each one fp32 accumulation.  rays_are_b: the ray-side operand is the MFMA's B (the `swapped` layer products)"""
    n, K = len(rays), rays.shape[-1]
    acc = np.zeros((rays.shape[1], units.shape[1]), dtype=F32) if acc is None else acc.astype(F32)
    for k0 in range(0, K, 16):
        for ia, ib in TERMS[n]:
            ir, iu = (ib, ia) if rays_are_b else (ia, ib)
            acc = (acc.astype(F64) + rays[ir][:, k0:k0 + 16].astype(F64) @ units[iu][:, k0:k0 + 16].astype(F64).T).astype(F32)
    return acc


def _exp32(x):
    with np.errstate(over="ignore"):
        return np.exp(x.astype(F64)).astype(F32)


def forward32(w, X, planes=3, fault=None, stride_rays=0):
    """k_brdf_mlp_fwd on an fp32 image -> out [R, 3], a1, a2 [R, 64] (float32).  fault: "two_terms" (planes = 2), "no_b0" (the bias
    column left out), "cur_nxt" (a tile computed from the inputs of the wave's next tile, stride_rays behind)"""
    assert fault is None or fault in FAULTS
    X = np.array(X, dtype=F32)
    if fault == "no_b0":
        X[:, COL_BIAS] = 0
    if fault == "cur_nxt":
        X = X[np.minimum(np.arange(len(X)) + stride_rays, len(X) - 1)]
    planes = 2 if fault == "two_terms" else planes
    a1 = product(split(X, planes), split(w0_image(w), planes), True)
    a2 = product(split(np.maximum(a1, F32(0)), planes), split(w[2], planes), True, np.broadcast_to(w[3], a1.shape))
    r2 = np.maximum(a2, F32(0))
    o = np.zeros((2, len(X), 3), dtype=F32)
    for h in (0, 1):
        for ub in (0, 1):
            for q in range(4):
                for i in range(4):
                    u = 32 * ub + 8 * q + 4 * h + i
                    o[h] = o[h] + r2[:, u:u + 1] * w[4][:3, u]
    z = ((o[0] + o[1]) + w[5][:3]) + F32(OUT_BIAS)
    return (F32(1) / (F32(1) + _exp32(-z))).astype(F32), a1, a2


def acc_row(q, h):
    return (q & 3) + 8 * (q >> 2) + 4 * h


def _swap_nibbles(m):
    return m[:, np.arange(64) ^ 4]


def _per_ray32(w, seg, fault):
    """what the backward computes per ray with no arithmetic across rays: input planes, g, H1 planes, relu(layer 2), the planes of
    dH2 and dH1, dX[:, features]"""
    m1, m2 = (_swap_nibbles(seg.m1), _swap_nibbles(seg.m2)) if fault == "nibbles" else (seg.m1, seg.m2)
    xp = split(seg.X, 2)
    g = ((seg.d_out * seg.s) * (F32(1) - seg.s)).astype(F32)
    a1 = product(xp, split(w0_image(w), 2), True)
    H1p = split(np.where(m1, a1, F32(0)), 2)
    v = np.maximum(product(H1p, split(w[2], 2), False) + w[3], F32(0))
    W4 = w[4]
    dH2 = np.where(m2, (g[:, 0:1] * W4[0] + g[:, 1:2] * W4[1]) + g[:, 2:3] * W4[2], F32(0)).astype(F32)
    d2p = split(dH2, 2)
    d1p = split(np.where(m1, product(d2p, split(np.ascontiguousarray(w[2].T), 2), True), F32(0)), 2)
    dx = product(d1p, split(np.ascontiguousarray(w[0][:, :24].T), 2), True)
    return SimpleNamespace(xp=xp, g=g, H1p=H1p, v=v, d2p=d2p, d1p=d1p, dx=dx)


def _new_acc():
    return {"W2": np.zeros((64, 64), F32), "W0": np.zeros((64, 64), F32), "tail": np.zeros((64, 8), F32),
            "W4": np.zeros((3, 64, 2), F32), "b2": np.zeros((64, 2), F32), "b4": np.zeros((3, 32), F32)}


def _mm(acc, a, b):
    return (acc.astype(F64) + a.astype(F64).T @ b.astype(F64)).astype(F32)


def reduce_workgroups(parts):
    """k_brdf_mlp_reduce: eight lane groups take partials wl, wl + 64, ... in batches of eight (stride 8) summed as a tree, then the
    groups as a tree"""
    n, z = len(parts), np.zeros_like(parts[0])
    tree = lambda a: ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))      # noqa: E731
    groups = []
    for wl in range(8):
        v = z.copy()
        for wb in range(wl, n, 64):
            v = v + tree([parts[wb + 8 * k] if wb + 8 * k < n else z for k in range(8)])
        groups.append(v)
    return tree(groups)


def backward32(w, segs, max_workgroups, fault=None):
    """k_brdf_mlp_bwd + k_brdf_mlp_reduce over one or two ray sets.  A set: namespace of X [R, 80] (fp32 image), m1, m2 [R, 64] bool,
    s (forward output) and d_out [R, 3], rows [R] (feature row of each ray) and M (rows) -> (reduced accumulators, [d_feat per set]).
    fault: "clamped", "last_tile", "nibbles", "d_out_of_set0" (see the module docstring)"""
    assert fault is None or fault in FAULTS
    if fault == "d_out_of_set0":
        s0, s1 = segs
        take = np.minimum(np.arange(len(s1.X)), len(s0.X) - 1)
        segs = [s0, SimpleNamespace(**dict(vars(s1), d_out=s0.d_out[take]))]
    per = [_per_ray32(w, s, fault) for s in segs]
    tiles = [(k, t) for k, s in enumerate(segs) for t in range(cdiv(len(s.X), RT))]
    grid = bwd_grid(len(tiles), max_workgroups)
    d_feat = [np.zeros((s.M, 24), dtype=F32) for s in segs]
    parts = []
    for wg in range(grid):
        waves = []
        for wave in range(WAVES):
            acc = _new_acc()
            for tl in range(wg * WAVES + wave, len(tiles), grid * WAVES):
                if fault == "last_tile":
                    acc = _new_acc()
                k, t = tiles[tl]
                _tile32(acc, d_feat[k], segs[k], per[k], t, fault)
            waves.append(acc)
        parts.append({key: ((waves[0][key] + waves[1][key]) + waves[2][key]) + waves[3][key] for key in waves[0]})
    return {key: reduce_workgroups([p[key] for p in parts]) for key in parts[0]}, d_feat


def _tile32(acc, d_feat, seg, p, t, fault):
    R = len(seg.X)
    lanes = t * RT + np.arange(RT)
    valid = lanes < R
    idx = np.minimum(lanes, R - 1)
    live = np.ones(RT, dtype=bool) if fault == "clamped" else valid
    g = np.where(live[:, None], p.g[idx], F32(0))
    xp, H1p, v = p.xp[:, idx], p.H1p[:, idx], p.v[idx]
    d2p, d1p = np.where(live[None, :, None], p.d2p[:, idx], F32(0)), np.where(live[None, :, None], p.d1p[:, idx], F32(0))
    dx = np.where(live[:, None], p.dx[idx], F32(0))
    acc["b4"] = acc["b4"] + g.T
    for h in (0, 1):
        for q in range(16):
            r = acc_row(q, h)
            acc["W4"][:, :, h] = acc["W4"][:, :, h] + g[r][:, None] * v[r][None, :]
        s8 = lambda a: functools.reduce(lambda x, y: x + y, [a[i] for i in range(8)])      # noqa: E731
        k0, k1 = slice(8 * h, 8 * h + 8), slice(16 + 8 * h, 16 + 8 * h + 8)
        acc["b2"][:, h] = acc["b2"][:, h] + ((s8(d2p[0][k0]) + s8(d2p[1][k0])) + (s8(d2p[0][k1]) + s8(d2p[1][k1])))
    tt = np.zeros((16, 64), dtype=F32)
    for kp in (slice(0, 16), slice(16, 32)):
        for ia, ib in TERMS[2]:
            acc["W2"] = _mm(acc["W2"], d2p[ia][kp], H1p[ib][kp])
            acc["W0"] = _mm(acc["W0"], d1p[ia][kp], xp[ib][kp][:, :64])
            tt = _mm(tt, xp[ia][kp][:, 64:], d1p[ib][kp])
    acc["tail"] = acc["tail"] + tt[:8].T
    # the feature rows: per run of equal row indices and half tile one masked sum in ray order, one add to the row
    rows = seg.rows[idx]
    starts = [0] + [r for r in range(1, RT) if rows[r] != rows[r - 1]] + [RT]
    for s, e in zip(starts[:-1], starts[1:]):
        for part in (0, 1):
            lo, hi = max(s, 16 * part), min(e, 16 * part + 16)
            if lo < hi:
                a = np.zeros(24, dtype=F32)
                for r in range(lo, hi):
                    a = a + dx[r]
                d_feat[rows[s]] = d_feat[rows[s]] + a


def emit(acc, init, fault=None):
    """mlp_grad_emit: the reduced accumulators added to what the six gradient buffers hold -> dict over GRADS (float32)"""
    gW0, gb0, gW2, gb2, gW4, gb4 = (np.array(a, dtype=F32) for a in init)
    for c in range(64):
        if COL_ORIG[c] >= 0:
            gW0[:, COL_ORIG[c]] = gW0[:, COL_ORIG[c]] + acc["W0"][:, c]
        elif COL_ORIG[c] == -1:
            gb0 = gb0 + acc["W0"][:, c]
    for c in range(64, 72):
        if COL_ORIG[c] >= 0 and fault != "no_tail":
            gW0[:, COL_ORIG[c]] = gW0[:, COL_ORIG[c]] + acc["tail"][:, c - 64]
    gW2 = gW2 + acc["W2"]
    gW4[:3] = (gW4[:3] + acc["W4"][:, :, 0]) + acc["W4"][:, :, 1]
    gb2 = (gb2 + acc["b2"][:, 0]) + acc["b2"][:, 1]
    for lane in range(RT):
        gb4[:3] = gb4[:3] + acc["b4"][:, lane]
    return dict(zip(GRADS, (gW0, gb0, gW2, gb2, gW4, gb4)))


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_forward(R, ws, salt=0):
    i = inputs(R, ws, salt)
    X = image(i.hv, i.dv, i.feat_rays, i.rough_rays, F32)
    X.setflags(write=False)
    out, a1, a2 = forward32(weights(ws), X)
    return SimpleNamespace(X=X, out=out, a1=a1, a2=a2)


def segment(R, ws, form, salt=0, masks=None):
    """the restatement's view of a ray set: its own forward output, the float64 masks (or the given ones)"""
    i, ref, own = inputs(R, ws, salt), reference64(R, ws, salt), own_forward(R, ws, salt)
    m1, m2 = (ref.m1, ref.m2) if masks is None else masks
    rows, M = (i.src_idx, i.M) if form == "rows" else (np.arange(R), R)
    return SimpleNamespace(X=own.X, m1=m1, m2=m2, s=own.out, d_out=i.d_out, rows=rows, M=M)


def _with(init, grads):
    return {k: np.asarray(a, dtype=F64) + grads[k] for k, a in zip(GRADS, init)}


def _case(want, own, metrics=METRICS, capped=True):
    """errors of the restatement and the margins: 8 x the error, at least 2^-23 x the scale -- and, for the quantities that
    tests/test_hip_parity.py also compares, never more than it allows them (`capped`)"""
    err = errors_over(own, want, metrics)
    mg = margins(err, want, metrics)
    if capped:
        mg = {m: min(v, parity_tolerance(m, _big(want[m]))) if _big(want[m]) > 0 else v for m, v in mg.items()}
    return SimpleNamespace(want=want, own=own, err=err, mg=mg, metrics=metrics)


@functools.lru_cache(maxsize=None)
def case(R, max_workgroups, ws, form="rows", filled=True):
    """(float64 reference `want`, restatement `own`, its errors `err`, margins `mg`) over METRICS of a forward + backward; the
    gradients as PATTERN + gradient when `filled`, alone otherwise"""
    ref = reference64(R, ws)
    init = pattern() if filled else zeros()
    acc, d_feat = backward32(weights(ws), [segment(R, ws, form)], max_workgroups)
    own = dict(emit(acc, init), out=own_forward(R, ws).out, d_feat=d_feat[0])
    want = dict(_with(init, vars(ref)), out=ref.out, d_feat=ref.d_feat_rows if form == "rows" else ref.d_feat_rays)
    return _case(want, own)


MASK_R, MASK_WS = 421, "wide"
MASK_NAMES = ("ones", "zeros", "alternating") + tuple(range(16))
N_GROUPS = 16                                     # 4-bit groups of a layer's 64 mask bits: (word, byte, lane half)


LONE = ("gW2", "gb2", "gb0")                      # the metrics of which a single-unit case leaves ONE element


@functools.lru_cache(maxsize=None)
def single_units(k):
    """(u1, u2) of single-unit case k: a unit of bit group k in layer 1 and one of group (k + 5) % 16 in layer 2.  Their lone
    elements gW2[u2, u1], gb2[u2], gb0[u1] are sums over the 421 rays of terms of both signs (d_out is), and a sum that cancels has
    no scale to hold an error against: of the 4 x 4 positions inside the two groups the pair is taken whose worst condition number
    sum |term| / |sum term| of the three, in float64, is smallest (7 to 19; the first positions drawn ran up to 385)"""
    i, ref, w = inputs(MASK_R, MASK_WS), reference64(MASK_R, MASK_WS), weights(MASK_WS)
    a1 = ref.X @ w0_image(w).astype(F64).T
    dH2 = (i.d_out.astype(F64) * ref.out * (1 - ref.out)) @ w[4].astype(F64)[:3]
    cond = lambda t: np.abs(t).sum() / abs(t.sum())      # noqa: E731
    pairs = [(4 * k + p, 4 * ((k + 5) % N_GROUPS) + q) for p in range(4) for q in range(4)]
    worst = [max(cond(dH2[:, u2] * a1[:, u1]), cond(dH2[:, u2]), cond(dH2[:, u2] * F64(w[2][u2, u1]))) for u1, u2 in pairs]
    return pairs[int(np.argmin(worst))] + (float(min(worst)),)


def given_masks(name):
    """m1, m2 [421, 64] bool: "ones", "zeros", "alternating" (units 0, 2, ... of layer 1 and 1, 3, ... of layer 2), or an integer k:
    the units single_units(k) alone"""
    R = MASK_R
    if name == "ones":
        m1 = m2 = np.ones((R, 64), dtype=bool)
    elif name == "zeros":
        m1 = m2 = np.zeros((R, 64), dtype=bool)
    elif name == "alternating":
        m1 = np.broadcast_to(np.arange(64) % 2 == 0, (R, 64))
        m2 = ~m1
    else:
        u1, u2, _ = single_units(int(name))
        m1, m2 = np.zeros((R, 64), dtype=bool), np.zeros((R, 64), dtype=bool)
        m1[:, u1], m2[:, u2] = True, True
    return m1, m2


@functools.lru_cache(maxsize=None)
def _mask_case(name):
    i, ref, w = inputs(MASK_R, MASK_WS), reference64(MASK_R, MASK_WS), weights(MASK_WS)
    m1, m2 = given_masks(name)
    acc, d_feat = backward32(w, [segment(MASK_R, MASK_WS, "rows", masks=(m1, m2))], 1)
    init = pattern()
    own = dict(emit(acc, init), out=own_forward(MASK_R, MASK_WS).out, d_feat=d_feat[0])
    g = backward64_given(w, ref.X, m1, m2, ref.out, i.d_out)
    c = _case(dict(_with(init, g), out=ref.out, d_feat=_rows_of(g["d_feat_rays"], i.src_idx, i.M)), own, capped=False)
    c.masks = pack_masks(m1, m2)
    return c


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """the backward at R = 421 on one workgroup with GIVEN masks, against backward64_given -> case() fields plus `masks` [R, 4];
    margins per metric and case, capped like case()'s.  A single-unit case leaves ONE element of gW2, gb2 and gb0 (LONE): the
    restatement's error on it is the luck of one rounding sequence and gives a maximum nothing to average over (the kernel sums in
    another order).  For these three metrics alone the sixteen single-unit cases share their margin: 8 x the largest restatement
    error of the sixteen RELATIVE to each case's scale, times this case's scale"""
    c = _mask_case(name)
    c = SimpleNamespace(**vars(c))
    mg = dict(c.mg)
    if isinstance(name, int):
        for m in LONE:
            rel = max(o.err[m] / _big(o.want[m]) for o in map(_mask_case, range(N_GROUPS)))
            mg[m] = max(8 * rel, FLOOR) * _big(c.want[m])
    c.mg = {m: min(v, parity_tolerance(m, _big(c.want[m]))) for m, v in mg.items()}
    return c


@functools.lru_cache(maxsize=None)
def pair_case(R0, R1, ws, fault=None):
    """two ray sets in one launch on one workgroup: set 0 = inputs(R0) with its src_idx, set 1 = inputs(R1, salt 1) with one feature
    row per ray; the weight gradients against the float64 sum of both -> case() fields with the metrics
    d_feat0, d_feat1 and the six gradients"""
    refs = (reference64(R0, ws), reference64(R1, ws, 1))
    init = pattern()
    acc, d_feat = backward32(weights(ws), [segment(R0, ws, "rows"), segment(R1, ws, "rays", 1)], 1, fault)
    own = dict(emit(acc, init), d_feat0=d_feat[0], d_feat1=d_feat[1])
    want = _with(init, {k: getattr(refs[0], k) + getattr(refs[1], k) for k in GRADS})
    want.update(d_feat0=refs[0].d_feat_rows, d_feat1=refs[1].d_feat_rays)
    return _case(want, own, ("d_feat0", "d_feat1") + GRADS)


# what tests/test_hip_parity.py allows the same quantities (atol + rtol x the metric's scale): no margin here may be looser
def parity_tolerance(metric, scale):
    if metric == "out":
        return 1e-6 + 1e-5 * scale
    if metric.startswith("d_feat"):
        return 1e-5 * (scale + 1) + 1e-4 * scale
    return 2e-5 * (scale + 1e-3) + 2e-4 * scale


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
def test_tiles_per_wave_are_what_the_cases_are_named_for():
    table = {  # (R, max_workgroups): (tiles, rays of the last tile, forward tiles per wave, backward tiles per wave)
        (1, 0): (1, 1, [1, 0, 0, 0], [1, 0, 0, 0]),
        (31, 0): (1, 31, [1, 0, 0, 0], [1, 0, 0, 0]),
        (32, 0): (1, 32, [1, 0, 0, 0], [1, 0, 0, 0]),
        (33, 0): (2, 1, [1, 1, 0, 0], [1, 1, 0, 0]),
        (421, 1): (14, 5, [4, 4, 3, 3], [4, 4, 3, 3]),
        (513, 2): (17, 1, [3] + [2] * 7, [3] + [2] * 7),
        (997, 1): (32, 5, [8] * 4, [8] * 4),
        (2049, 0): (65, 1, [1] * 65 + [0] * 3, [2] * 29 + [1] * 7),
    }
    assert set(table) == set(CASES)
    for (R, mw), (tiles, last, fwd, bwd) in table.items():
        assert cdiv(R, RT) == tiles and R - (tiles - 1) * RT == last
        assert tiles_per_wave(tiles, fwd_grid(R, mw)) == fwd, (R, mw)
        assert tiles_per_wave(tiles, bwd_grid(tiles, mw)) == bwd, (R, mw)
    # the forward's loop takes a second iteration, the backward reaches the step's 8 tiles per wave, the default grids stay default
    assert fwd_grid(2049, 0) == 17 and bwd_grid(65, 0) == 9 and fwd_grid(10 ** 6, 0) == 256 and bwd_grid(10 ** 5, 300) == 256
    # through autograd (no max_workgroups): 8 workgroups forward, 4 backward at R = 997
    assert fwd_grid(997, 0) == 8 and bwd_grid(32, 0) == 4
    for R0, R1 in PAIRS:
        assert bwd_grid(cdiv(R0, RT) + cdiv(R1, RT), 1) == 1


@pytest.mark.parametrize("ws", WEIGHTS)
def test_rows_and_roughness(ws):
    for R, _ in CASES:
        for salt in (0, 1):
            i = inputs(R, ws, salt)
            src = i.src_idx
            assert src.dtype == np.int32 and len(src) == R and (np.diff(src) >= 0).all() and src[0] == 0
            lens = np.diff(np.flatnonzero(np.concatenate([[True], np.diff(src) > 0, [True]])))
            assert all(n == RUNS[(k + salt) % 5] for k, n in enumerate(lens[:-1])) and lens[-1] <= RUNS[(len(lens) - 1 + salt) % 5]
            unused = np.setdiff1d(np.arange(i.M), i.gathered)
            assert len(unused) >= 1 and i.M - 1 in unused
            assert i.rough_rays.min() >= MIN_ROUGH and i.rough_rays.max() <= 1 and i.rough_rays[0] == MIN_ROUGH
            if len(lens) > 1:
                assert (i.rough_rays == F32(1.0)).any() and 1 in unused
            assert np.array_equal(i.feat_rays, i.feat[src]) and np.array_equal(i.rough_rays, i.rough[src])
    # runs straddle tile edges and tiles of different waves at R = 421: a run covering rays of two tiles, a tile with three runs
    src = inputs(421, ws).src_idx
    assert any(src[32 * t - 1] == src[32 * t] for t in range(1, 14)) and any(len(np.unique(src[32 * t:32 * t + 32])) >= 3 for t in range(13))
    w = weights(ws)
    assert [a.shape for a in w] == [(64, 66), (64,), (64, 64), (64,), (4, 64), (4,)]
    assert len({float(w[k][0]) for k in (1, 3, 5)}) == 3
    assert all(np.all(a != 0) for a in pattern())


@pytest.mark.parametrize("ws", WEIGHTS)
def test_redraw_share(ws):
    redrawn = sum(inputs(R, ws, s).redrawn for R, _ in CASES for s in (0, 1))
    total = 2 * sum(R for R, _ in CASES)
    print(f"{ws}: {redrawn} of {total} rays redrawn on the first pass = {100 * redrawn / total:.2f} %")
    assert redrawn <= REDRAW_CAP * total
    for R, _ in CASES:
        ref = reference64(R, ws)
        assert np.abs(ref.a1).min() >= CLEAR[ws][0] and np.abs(ref.a2).min() >= CLEAR[ws][1]


@pytest.mark.parametrize("ws", WEIGHTS)
def test_clear_is_32_to_128_restatement_errors(ws):
    """CLEAR[ws][layer] >= 32 x the largest error of the restatement's pre-activations of that layer; and its masks are the float64 ones"""
    e1 = max(_big(own_forward(R, ws, s).a1 - reference64(R, ws, s).a1) for R, _ in CASES for s in (0, 1))
    e2 = max(_big(own_forward(R, ws, s).a2 - reference64(R, ws, s).a2) for R, _ in CASES for s in (0, 1))
    print(f"{ws}: pre-activation errors {e1:.3e} {e2:.3e}, x 32 = {32 * e1:.3e} {32 * e2:.3e}, CLEAR {CLEAR[ws]}")
    assert 32 * e1 <= CLEAR[ws][0] <= 128 * e1 and 32 * e2 <= CLEAR[ws][1] <= 128 * e2
    for R, _ in CASES:
        own, ref = own_forward(R, ws), reference64(R, ws)
        assert np.array_equal(pack_masks(own.a1 > 0, own.a2 > 0), ref.masks)


@pytest.mark.parametrize("ws", WEIGHTS)
def test_references_agree(ws):
    """forward64 on the image is oracle.brdf_mlp; backward64_given on the forward's masks is its autograd; W4's fourth row gets zeros"""
    for R in (33, 421):
        i, ref, w = inputs(R, ws), reference64(R, ws), weights(ws)
        assert _big(ref.out_img - ref.out) <= 1e-14
        g = backward64_given(w, ref.X, ref.m1, ref.m2, ref.out, i.d_out)
        for k in GRADS + ("d_feat_rays",):
            assert _big(g[k] - getattr(ref, k)) <= 1e-12 * max(_big(getattr(ref, k)), 1.0), k
        assert not ref.gW4[3].any() and ref.gb4[3] == 0 and _big(ref.gW4[:3]) > 0
        m1, m2 = unpack_masks(ref.masks.view(np.int32))
        assert np.array_equal(m1, ref.m1) and np.array_equal(m2, ref.m2)
        assert not ref.d_feat_rows[1].any() and not ref.d_feat_rows[i.M - 1].any()
    # bit layout: unit u of layer l on bit u % 32 of word 2 l + u // 32
    m = np.zeros((1, 64), dtype=bool)
    m[0, 37] = True
    assert pack_masks(m, ~m).tolist() == [[0, 1 << 5, 0xFFFFFFFF, 0xFFFFFFFF ^ (1 << 5)]]


def test_split_and_products():
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-3, 3, 4096)).astype(F32)
    # ties go to the even mantissa: 1 + 2^-8 -> 1, 1 + 2^-7 + 2^-8 -> 1 + 2^-6
    assert bf16(np.array([1.0, 1.00390625, 1.01171875, -1.00390625], dtype=F32)).tolist() == [1.0, 1.0, 1.015625, -1.0]
    assert all((p.view(np.uint32) & 0xFFFF == 0).all() for p in split(v, 3))
    for n, bits in ((2, 16), (3, 24)):
        assert _big((split(v, n).astype(F64).sum(0) - v) / v) <= 2.0 ** -bits
    a, b = rng.standard_normal((32, 80)).astype(F32), rng.standard_normal((64, 80)).astype(F32)
    exact = a.astype(F64) @ b.astype(F64).T
    e3, e2 = (_big(product(split(a, n), split(b, n), True) - exact) for n in (3, 2))
    assert e3 < 2e-5 and 4 * e3 < e2 < 1e-3, (e3, e2)


def test_margins_are_not_looser_than_the_fp32_test():
    """... and the cap binds on few of them: the margins are the restatement's, not the older test's"""
    n, bound = 0, []
    cases = [((ws, R, mw, form), case(R, mw, ws, form)) for ws in WEIGHTS for R, mw in CASES for form in FORMS]
    cases += [((ws, R0, R1), pair_case(R0, R1, ws)) for ws in WEIGHTS for R0, R1 in PAIRS]
    cases += [((ws, 997, 0, "autograd"), case(997, 0, ws, "rows", False)) for ws in WEIGHTS]
    cases += [(("masks", name), mask_case(name)) for name in MASK_NAMES]
    for what, c in cases:
        for m in c.metrics:
            tol = parity_tolerance(m, _big(c.want[m]))
            n += 1
            assert c.mg[m] <= tol, (what, m, c.mg[m], tol)
            # the restatement itself is well inside: a quarter of its own margin, half of a margin that the cap has cut
            assert c.err[m] <= (c.mg[m] / 4 if c.mg[m] < tol else tol / 2), (what, m, c.err[m], c.mg[m])
            if c.mg[m] == tol:
                bound.append((what, m, round(c.err[m] / tol, 2)))
    print(f"the parity tolerance is the margin on {len(bound)} of {n}: {bound}")
    assert len(bound) <= n // 10


def test_restatement_table():
    """prints the restatement's errors against float64 and the margins of every case"""
    for ws in WEIGHTS:
        for R, mw in CASES:
            c = case(R, mw, ws)
            print(f"{ws:6s} R {R:4d} wg {mw}: " + "  ".join(f"{m} {c.err[m]:.1e}/{_big(c.want[m]):.1e}" for m in METRICS))
            assert all(np.isfinite(c.mg[m]) and c.mg[m] > 0 for m in METRICS)


@pytest.mark.parametrize("name", MASK_NAMES)
def test_given_masks(name):
    """with all-zero masks gW4 / gb4 are still gradients (relu(b2) as the layer's values) and everything upstream is exactly zero;
    a single unit per layer leaves exactly its row / column of the hidden gradients"""
    c, init = mask_case(name), dict(zip(GRADS, pattern()))
    grad = {k: c.want[k] - init[k] for k in GRADS}
    assert _big(grad["gW4"][:3]) > 0 and _big(grad["gb4"][:3]) > 0
    if name == "zeros":
        for k in ("gW0", "gb0", "gW2", "gb2"):
            assert not grad[k].any() and np.array_equal(c.own[k], init[k]), k
        assert not c.want["d_feat"].any() and not c.own["d_feat"].any()
    if isinstance(name, int):
        m1, m2 = given_masks(name)
        u1, u2 = int(np.flatnonzero(m1[0])[0]), int(np.flatnonzero(m2[0])[0])
        assert u1 // 4 == name and u2 // 4 == (name + 5) % N_GROUPS and (u1, u2) == single_units(name)[:2]
        assert single_units(name)[2] <= 20
        only = np.zeros((64, 64), dtype=bool)
        only[u2, u1] = True
        assert grad["gW2"][u2, u1] != 0 and not grad["gW2"][~only].any() and np.array_equal(c.own["gW2"][~only], init["gW2"][~only])
        assert np.flatnonzero(grad["gb2"]).tolist() == [u2] and np.flatnonzero(grad["gb0"]).tolist() == [u1]
        assert np.flatnonzero(np.abs(grad["gW0"]).sum(1)).tolist() == [u1]
        # the shared margins stay below 1 % of the scale, and the restatement with the lane-half groups swapped (the units land on
        # other bits) misses them
        assert all(c.err[m] <= c.mg[m] <= 0.01 * _big(c.want[m]) for m in METRICS), (c.err, c.mg)
        acc, d_feat = backward32(weights(MASK_WS), [segment(MASK_R, MASK_WS, "rows", masks=(m1, m2))], 1, "nibbles")
        broken = _ratio(c, dict(emit(acc, pattern()), d_feat=d_feat[0]), METRICS[1:])
        assert all(broken[m] > 1 for m in ("d_feat", "gW0", "gb0", "gW2", "gb2")), broken


def _ratio(c, own, metrics):
    return {m: _big(np.asarray(own[m], dtype=F64) - c.want[m]) / c.mg[m] for m in metrics}


def test_broken_restatements_miss_their_margins():
    ws, R, mw = "wide", 421, 1
    w, c, init = weights(ws), case(R, mw, ws), pattern()
    X = own_forward(R, ws).X
    rows = []

    def fwd(fault, **kw):
        return {"out": forward32(w, X, fault=fault, **kw)[0]}

    def bwd(fault):
        acc, d_feat = backward32(w, [segment(R, ws, "rows")], mw, None if fault == "no_tail" else fault)
        return dict(emit(acc, init, fault), d_feat=d_feat[0])

    rows.append(("1 forward on two bf16 terms", _ratio(c, fwd("two_terms"), ("out",)), ("out",)))
    rows.append(("2 the next tile's inputs used for the current tile", _ratio(c, fwd("cur_nxt", stride_rays=RT * WAVES * fwd_grid(R, mw)), ("out",)),
                 ("out",)))
    rows.append(("3 clamped lanes counted in the weight gradients", _ratio(c, bwd("clamped"), GRADS), ("gW0", "gb0", "gW2", "gb2", "gW4", "gb4")))
    rows.append(("4 a wave keeps only its last tile", _ratio(c, bwd("last_tile"), GRADS), GRADS))
    rows.append(("5 lane-half groups of a mask byte swapped", _ratio(c, bwd("nibbles"), METRICS[1:]), ("d_feat", "gW0", "gb0", "gW2", "gb2", "gW4")))
    rows.append(("6 the b0 column dropped", _ratio(c, fwd("no_b0"), ("out",)), ("out",)))
    rows.append(("7 input columns 61-65 of gW0 left at zero", _ratio(c, bwd("no_tail"), ("gW0",)), ("gW0",)))
    p = pair_case(421, 37, ws)
    broken = pair_case(421, 37, ws, "d_out_of_set0").own
    rows.append(("8 set 1 reads set 0's d_out (421 + 37)", _ratio(p, broken, p.metrics), ("d_feat1",) + GRADS))
    for what, ratio, named in rows:
        print(f"    {what:52s}" + "  ".join(f"{m} {ratio[m]:.1e}" for m in ratio))
    for what, ratio, named in rows:
        for m in named:
            assert ratio[m] > 1, (what, m, ratio[m])
    # fault 1 also on the golden weights: the variant the design rejects is outside the margin there too
    g = case(R, mw, "golden")
    two = _ratio(g, {"out": forward32(weights("golden"), own_forward(R, "golden").X, fault="two_terms")[0]}, ("out",))
    print(f"    1 on the golden weights: out {two['out']:.1e}")
    assert two["out"] > 1
    assert _ratio(p, broken, ("d_feat0",))["d_feat0"] <= 1
