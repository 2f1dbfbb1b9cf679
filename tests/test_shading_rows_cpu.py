"""The per-ray and per-row glue of the shading step without a GPU: the inputs, the float64 references, the fp32 restatements of
csrc/shade.hip (ray compose, bounce prep), csrc/rows_bwd.hpp and csrc/heads.hip, and the margins that the GPU tests
(tests/test_hip_shading_rows.py) hold the kernels to -- and the tests that show those margins are neither vacuous nor blind.

Ray batches put ray r at ladder()[r % 34] samples (tests/test_composite_cpu.py), so the two-samples-per-lane-per-pass walk of
k_ray_compose_fwd_wave meets 63 / 64 / 65, 127 / 128 / 129, 191 / 192 / 193 samples under 64 lanes and 7 / 8 / 9, 15 / 16 / 17,
23 / 24 / 25 under 8.  Bounce rows come at 1, 255, 256, 257 and 4099 rows with their adjoints dense and as column slices of
[Mb, 7], [Mb, 4] and [Mb, 6] buffers whose other columns hold 1e30; the heads at 1, 255, 256, 257 and 1024 * 256 + 257 rows (the
first size with a second pass of the capped grid and a partial last block).

Where the inputs leave the ranges first written down for them, and why:
  * weights are u * min(0.02, 1.6 / n) for a ray of n samples, u uniform in [0, 1], not u * 0.02: a 257-sample ray of weights with
    mean 0.01 has acc = 2.6, and 1 - acc < 0 is no state the step ever composes.  Rays up to 80 samples keep [0, 0.02].
  * every seventh ray is `bright` (a bounce row on every sample, reflectance in [1.5, 2]) so that long rays reach rgb_lin > 1 and the
    [0, 1] clip of the tonemap binds on some rays and not on others, and every seventh `dim` (reflectance scaled by 2^-9) so that
    rays of any length stay below the sRGB knee; the other rays have a row on half of their samples.
  * the conditioning (below) is constructed, not drawn: a ray channel whose float64 rgb_lin lands within 2e-3 of a gate is scaled
    by 1/4 (or set to exactly 0 below the clip at 0), a normal whose float64 V.N lies within 2e-3 of 0 is moved 0.1 along the ray,
    a head row within 2e-3 of a roughness gate is moved away from it.  With ~1.2 M samples no seed meets the condition by itself.

Conditioning: every quantity that feeds a gate -- sign(V.N) and ndv < 0, h9 >= min_rough, the sRGB knee, the [0, 1] clip of the
tonemap output, r >= 0.01 of the heads -- is at least 1e-3 from its threshold in float64, or sits exactly on it with exactly
representable values (a zero normal, h9 == min_rough, an rgb_lin of exactly 0, and the one-sample rays `knee` and `knee_up` whose
rgb_lin is the fp32 knee constant and the float above it).  test_every_gate_is_clear_or_exact asserts it; the GPU tests then compare
EVERY element.

Margins (the convention of tests/test_composite_cpu.py): per metric and batch, 8 x the largest error of the restatement against
float64, at least 2^-23 x the metric's scale (the largest |reference|; a reference of zeros therefore demands exact zeros).
test_margins_are_not_looser_than_the_fp32_tests holds each against the tolerance of tests/test_hip_parity.py for the same quantity.

The margins are not blind (test_broken_restatements_miss_their_margins; error / margin of the restatement broken on purpose):
    the k + W sample of the second pass dropped     partial: acc 4.9e+05  rgb_lin 4.4e+05  ori 5.2e+05     narrow: 1.3e+05  1.4e+05  2.1e+05
    row adjoints read with pitch 3 from pitch 7     d_normals, d_heads > 1e+34 (the 1e30 of the unused columns) from 255 rows on
    second grid pass of the weight gradient left    gW 5.6e+03   gb 3.5e+03

Which test enters which of the six paths that no earlier test entered:
  1  second sample and second pass of k_ray_compose_fwd_wave<64>, 8 lanes at long rays
         test_batches_have_the_shapes_they_are_named_for, test_lane_walk_restatement_*, GPU: test_ray_compose_against_float64,
         test_ray_compose_one_hot_weights, test_same_rays_under_both_lane_widths
  2  the forms levels >= 1 call (no normals / ori / tonemap, per-ray background), refl absent, noclip
         FLAGS (all 32 combinations), GPU: test_ray_compose_against_float64, test_ray_compose_without_bounce_rows
  3  strided row adjoints: strided_adjoints(), test_pitch_*; GPU: test_bounce_prep_bwd_dense_and_strided, test_fused_prep_heads_bwd_*
  4  k_heads_bwd beyond one pass of the grid: HEAD_ROWS[-1]; GPU: test_heads_against_float64, test_heads_one_hot_rows
  5  gates and saturation of the heads: heads_inputs(), test_heads_inputs_*; GPU: test_heads_saturated_and_clipped_rows
  6  float64 on the reference side: every *_reference64 below
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nmf_oracle as O
from test_composite_cpu import batch, ladder

F32, F64 = np.float32, np.float64
FLOOR = 2.0 ** -23
WPR_MAX_RAYS = 16384                     # csrc/shade.hip: up to this many rays 64 lanes walk a ray, above it 8
KNEE32 = F32(0.0031308)                  # SRGB_LIMIT of csrc/shade.hip: the threshold the kernel compares fp32 values with
CLEAR = 1e-3                             # the distance every gate keeps in float64
RAY_BATCHES = {"partial": 4 * len(ladder()) + 3, "last64": 16384, "narrow": 16384 + 37}
SMALL_RAY_BATCHES = ("one", "empty5", "knee", "knee_up")
# (tonemap, noclip, bg_per_ray, want_ori, with_refl)
FLAGS = list(itertools.product((False, True), repeat=5))
LEVEL1 = (False, False, True, False, True)          # what the levels >= 1 of the step call
ROW_COUNTS = (1, 255, 256, 257, 4099)
HEAD_ROWS = (1, 255, 256, 257, 1024 * 256 + 257)
MIN_ROUGH, ANOISE = 0.25, 0.25                       # exactly representable: the kernels get them as floats
HP = (1.5, -0.625, 0.125, -0.25, -1.0)               # diffuse_mul, diffuse_bias, tint_bias, f0_bias, rough_bias (all exact in fp32)
RAY_METRICS = ("rgb_lin", "acc", "ori", "rgb_map", "d_weight", "d_refl", "d_normals", "bg_adjoint")
ROW_METRICS = ("N", "r1", "f0", "diffuse", "feat", "d_normals", "d_heads", "d_app")
HEAD_METRICS = ("out", "d_feat", "gW", "gb")


def _ro(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def _big(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def flag_id(f):
    return "".join(c if on else "-" for c, on in zip("TNBOR", f))


# ---- inputs: rays ---------------------------------------------------------------------------------------------------------------------
def tonemap64(x, noclip, limit=float(KNEE32)):
    """oracle.srgb_tonemap (modules/tonemap.py:38-49) on doubles with the knee at the constant the kernel compares with: the fp32
    value of 0.0031308.  The two agree everywhere but between the two constants (test_tonemap64_is_the_oracle_off_the_knee)."""
    out = torch.where(x > limit, 1.055 * (x.clip(min=limit) ** (1.0 / 2.4)) - 0.055, 12.92 * x)
    return out if noclip else out.clip(0, 1)


def _lin64(weight, refl, inv, ray_id, b):
    rgb = np.where((inv >= 0)[:, None], refl.astype(F64)[np.maximum(inv, 0)], 0.0) if len(refl) else np.zeros((len(weight), 3))
    return np.stack([np.bincount(ray_id, weights=weight.astype(F64) * rgb[:, c], minlength=b) for c in range(3)], axis=1)


def _clear_of_the_plane(normals, dirs):
    """normals whose float64 dot product with the ray direction lies within 2e-3 of zero are moved by 0.1 of it along the direction"""
    dn = (normals.astype(F64) * dirs.astype(F64)).sum(1)
    bad = np.abs(dn) < 2 * CLEAR
    step = np.where(dn >= 0, 0.1, -0.1) / (dirs.astype(F64) ** 2).sum(1)
    normals[bad] = (normals[bad].astype(F64) + step[bad, None] * dirs[bad].astype(F64)).astype(F32)
    return normals


def _ray_ns(off, weight, inv, refl, normals, rays, rng):
    b = len(off) - 1
    ray_id = np.repeat(np.arange(b), np.diff(off)).astype(np.int32)
    return _ro(SimpleNamespace(
        b=b, offsets=off, ray_id=ray_id, weight=weight, inv=inv, refl=refl, normals=normals, rays=rays,
        bg_ray=rng.uniform(0.0, 1.0, (b, 3)).astype(F32), bg_one=np.ones((1, 3), dtype=F32),
        d_rgb=rng.standard_normal((b, 3)).astype(F32), d_acc=rng.standard_normal(b).astype(F32),
        d_ori=rng.standard_normal(b).astype(F32)))


@functools.lru_cache(maxsize=None)
def ray_inputs(name):
    """b, offsets [b+1] int64, ray_id [M] int32, weight [M], inv [M] int32 (bounce row of a sample or -1), refl [Mb,3], normals [M,3],
    rays [b,6], bg_ray [b,3], bg_one [1,3] and the adjoints d_rgb [b,3], d_acc [b], d_ori [b]; float32, read-only, built once"""
    rng = np.random.default_rng([7, sum(map(ord, name))])
    if name in ("one", "knee", "knee_up"):               # one ray, one sample (knee*: weight 1, rgb_lin on / one float above the knee)
        refl = {"one": np.array([[0.9, 0.002, 1.7]], dtype=F32), "knee": np.full((1, 3), KNEE32, dtype=F32),
                "knee_up": np.full((1, 3), np.nextafter(KNEE32, F32(1)), dtype=F32)}[name]
        w = np.array([0.0125 if name == "one" else 1.0], dtype=F32)
        return _ray_ns(np.array([0, 1], dtype=np.int64), w, np.zeros(1, dtype=np.int32), refl,
                       np.array([[0.3, -0.8, 0.5]], dtype=F32), np.array([[0, 0, 0, 0.6, 0.0, -0.8]], dtype=F32), rng)
    if name == "empty5":                                 # five rays, no sample: every per-sample array is empty
        return _ray_ns(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=F32), np.zeros(0, dtype=np.int32), np.zeros((0, 3), dtype=F32),
                       np.zeros((0, 3), dtype=F32), rng.standard_normal((5, 6)).astype(F32), rng)
    b = RAY_BATCHES[name]
    off, _, _ = batch(b, 0)
    counts = np.diff(off)
    M = int(off[-1])
    ray = np.repeat(np.arange(b), counts)
    weight = (rng.uniform(0.0, 1.0, M) * np.minimum(0.02, 1.6 / np.maximum(counts, 1))[ray]).astype(F32)
    bright = (ray % 7) == 3
    has = bright | (rng.uniform(0.0, 1.0, M) < 0.5)
    inv = np.where(has, np.cumsum(has) - 1, -1).astype(np.int32)
    refl = rng.uniform(0.0, 2.0, (int(has.sum()), 3)).astype(F32)
    refl[bright[has]] = rng.uniform(1.5, 2.0, (int(bright[has].sum()), 3)).astype(F32)
    dim = ((ray % 7) == 5)[has]
    refl[dim] *= F32(2.0 ** -9)                           # reflectance in [0, 0.004]: rgb_lin below the knee on rays of any length
    row_ray = ray[has]
    lin = _lin64(weight, refl, inv, ray, b)
    refl[(0 < lin[row_ray]) & (lin[row_ray] < 2 * CLEAR / 12.92)] = 0.0
    near = (np.abs(lin - float(KNEE32)) < 2 * CLEAR) | (np.abs(lin - 1.0) < 6 * CLEAR)
    refl[near[row_ray]] *= F32(0.25)
    rays = rng.standard_normal((b, 6)).astype(F32)
    normals = _clear_of_the_plane(rng.standard_normal((M, 3)).astype(F32), rays[ray, 3:6])
    normals[off[1]] = 0.0                                # the first sample of ray 1: a zero normal, ndv == 0 exactly
    return _ray_ns(off, weight, inv, refl, normals, rays, rng)


def head_of(i, n):
    """the first n rays of a ray batch as a batch of their own (views of the same arrays)"""
    M = int(i.offsets[n])
    Mb = int((i.inv[:M] >= 0).sum())
    return SimpleNamespace(b=n, offsets=i.offsets[:n + 1], ray_id=i.ray_id[:M], weight=i.weight[:M], inv=i.inv[:M], refl=i.refl[:Mb],
                           normals=i.normals[:M], rays=i.rays[:n], bg_ray=i.bg_ray[:n], bg_one=i.bg_one, d_rgb=i.d_rgb[:n],
                           d_acc=i.d_acc[:n], d_ori=i.d_ori[:n])


def one_hot_weight(i, index):
    """the weights of a batch with every sample zeroed but sample `index` of each ray (-1: its last); rays too short keep nothing"""
    counts = np.diff(i.offsets)
    rows = np.nonzero(counts > (index if index >= 0 else 0))[0]
    at = i.offsets[rows] + (index if index >= 0 else counts[rows] - 1)
    w = np.zeros_like(i.weight)
    w[at] = i.weight[at]
    return w, rows, at


def ray_gate_distances(i):
    """float64 distance of everything that feeds a gate of ray compose from its threshold; exact hits are counted, not measured"""
    dn = (i.normals.astype(F64) * i.rays[i.ray_id, 3:6].astype(F64)).sum(1)
    zero_n = ~i.normals.any(axis=1)
    lin = _lin64(i.weight, i.refl, i.inv, i.ray_id, i.b)
    o = tonemap64(torch.from_numpy(lin), True).numpy()
    inf = np.inf
    return SimpleNamespace(ndv=np.abs(dn[~zero_n]).min(initial=inf), zero_normals=int(zero_n.sum()),
                           knee=np.abs(lin - float(KNEE32)).min(initial=inf), clip1=np.abs(o - 1.0).min(initial=inf),
                           clip0=o[lin != 0].min(initial=inf), lin=lin, o=o)


# ---- ray compose: float64 and fp32 ------------------------------------------------------------------------------------------------
def ray_reference64(i, flags, weight=None):
    """modules/tensor_nerf.py:448-452 (acc / rgb sums), :583-587 (orientation term), modules/tonemap.py and the background blend
    :658-659 in float64 on the float32 inputs, adjoints by autograd -> dict of float64 numpy arrays over RAY_METRICS + rgb_map_of"""
    tonemap, noclip, per_ray, want_ori, with_refl = flags
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))      # noqa: E731
    w = t(i.weight if weight is None else weight).requires_grad_(True)
    rf, n, bg = t(i.refl).requires_grad_(True), t(i.normals).requires_grad_(True), t(i.bg_ray if per_ray else i.bg_one).requires_grad_(True)
    rid, inv = torch.from_numpy(i.ray_id.astype(np.int64)), torch.from_numpy(i.inv.astype(np.int64))
    M = len(i.ray_id)
    if with_refl and len(i.refl):
        rgb = torch.where((inv >= 0)[:, None], rf[inv.clamp(min=0)], torch.zeros(M, 3, dtype=torch.float64))
    else:
        rgb = torch.zeros(M, 3, dtype=torch.float64)
    acc = torch.zeros(i.b, dtype=torch.float64).index_add(0, rid, w)
    lin = torch.zeros(i.b, 3, dtype=torch.float64).index_add(0, rid, w[:, None] * rgb)
    ndv = (-t(i.rays)[rid][:, 3:6] * n).sum(-1)
    ori = torch.zeros(i.b, dtype=torch.float64).index_add(0, rid, w * ndv.clamp(max=0) ** 2)
    out = (tonemap64(lin, noclip) if tonemap else lin) + (1 - acc[:, None]) * bg
    loss = (out * t(i.d_rgb)).sum() + (acc * t(i.d_acc)).sum() + ((ori * t(i.d_ori)).sum() if want_ori else 0.0)
    gw, grf, gn, gbg = torch.autograd.grad(loss, [w, rf, n, bg], allow_unused=True)
    z = lambda g, like: (torch.zeros_like(like) if g is None else g).numpy()      # noqa: E731
    bg_adj = ((1 - acc.detach())[:, None] * t(i.d_rgb)).numpy()
    return {"rgb_lin": lin.detach().numpy(), "acc": acc.detach().numpy(), "ori": ori.detach().numpy() if want_ori else None,
            "rgb_map": out.detach().numpy(), "d_weight": z(gw, w), "d_refl": z(grf, rf) if with_refl else None,
            "d_normals": z(gn, n) if want_ori else None, "bg_adjoint": bg_adj, "d_bg": z(gbg, bg)}


def rgb_map_of(i, flags, lin, acc):
    """the float64 tonemap and background blend of GIVEN sums (the kernel's own, or the restatement's): the second of the two steps
    in which rgb_map is compared, which keeps powf apart from the summation"""
    tonemap, noclip, per_ray = flags[:3]
    lin, acc = torch.from_numpy(np.asarray(lin, dtype=F64)), torch.from_numpy(np.asarray(acc, dtype=F64))
    bg = torch.from_numpy((i.bg_ray if per_ray else i.bg_one).astype(F64))
    return ((tonemap64(lin, noclip) if tonemap else lin) + (1 - acc[:, None]) * bg).numpy()


def lane_walk32(terms, offsets, W, fault=None):
    """k_ray_compose_fwd_wave<W> on per-sample fp32 terms [M, Q]: lane l of a ray's group takes samples k = l + 2 W p and k + W in
    pass p, adds them in that order to its own fp32 accumulator, then the W/2 .. 1 shuffle tree -> [b, Q] float32.
    fault="second": the k + W sample of the second pass (p = 1) is not added."""
    counts = np.diff(offsets)
    b, Q = len(counts), terms.shape[1]
    n_pass = -(-int(counts.max(initial=0)) // (2 * W)) if b else 0
    width = max(n_pass, 1) * 2 * W
    padded = np.zeros((b, width, Q), dtype=F32)
    col = np.arange(len(terms)) - np.repeat(offsets[:-1], counts)
    padded[np.repeat(np.arange(b), counts), col] = terms
    padded = padded.reshape(b, -1, 2, W, Q)
    v = np.zeros((b, W, Q), dtype=F32)
    for p in range(n_pass):
        v = v + padded[:, p, 0]
        if not (fault == "second" and p == 1):
            v = v + padded[:, p, 1]
    d = W // 2
    while d > 0:                                           # __shfl_down(v, d, W): lane l adds lane l + d where that is inside the group
        up = np.zeros_like(v)
        up[:, :W - d] = v[:, d:]
        v = v + up
        d //= 2
    return v[:, 0]


def _pow32(x, e):
    return np.power(x.astype(F64), e).astype(F32)          # correctly rounded, whatever the host's powf does


def ray_restatement32(i, flags, weight=None, fault=None):
    """nmf_ray_compose_fwd / _bwd and nmf_bg_adjoint in numpy float32 in the kernels' order of operations (products rounded, then
    added: no fma) -> dict of float32 arrays over RAY_METRICS"""
    tonemap, noclip, per_ray, want_ori, with_refl = flags
    w = np.asarray(i.weight if weight is None else weight, dtype=F32)
    W = 64 if i.b <= WPR_MAX_RAYS else 8
    M = len(w)
    d = i.rays[i.ray_id, 3:6]
    row = i.inv >= 0
    c = np.where(row[:, None], i.refl[np.maximum(i.inv, 0)], F32(0)) if with_refl and len(i.refl) else np.zeros((M, 3), dtype=F32)
    nd = -((d[:, 0] * i.normals[:, 0] + d[:, 1] * i.normals[:, 1]) + d[:, 2] * i.normals[:, 2])
    ndv = np.minimum(nd, F32(0))
    terms = np.concatenate([w[:, None], w[:, None] * c, (w * (ndv * ndv))[:, None]], axis=1).astype(F32)
    sums = lane_walk32(terms, i.offsets, W, fault)
    acc, lin, ori = sums[:, 0], sums[:, 1:4], sums[:, 4]
    bg = np.broadcast_to(i.bg_ray if per_ray else i.bg_one, (i.b, 3))

    def srgb(x):
        o = np.where(x > KNEE32, F32(1.055) * _pow32(np.maximum(x, KNEE32), 1.0 / 2.4) - F32(0.055), F32(12.92) * x).astype(F32)
        return o if noclip else np.minimum(np.maximum(o, F32(0)), F32(1))

    rgb_map = (srgb(lin) if tonemap else lin) + (F32(1) - acc)[:, None] * bg
    # backward: one thread per sample
    g = i.d_rgb
    if tonemap:
        with np.errstate(divide="ignore", invalid="ignore"):
            p = _pow32(lin, 1.0 / 2.4)
            up = lin > KNEE32
            o = np.where(up, F32(1.055) * p - F32(0.055), F32(12.92) * lin).astype(F32)
            sg = np.where(up, F32(1.055) * F32(1.0 / 2.4) * p / lin, F32(12.92)).astype(F32)
        if not noclip:
            sg = np.where((o < 0) | (o > 1), F32(0), sg)
        g = i.d_rgb * sg
    ga = i.d_acc.copy()
    for ch in range(3):
        ga = ga - i.d_rgb[:, ch] * bg[:, ch]
    r = i.ray_id
    dw = ga[r]
    d_refl = None
    if with_refl:
        gr = g[r]
        dw = np.where(row, dw + ((gr[:, 0] * c[:, 0] + gr[:, 1] * c[:, 1]) + gr[:, 2] * c[:, 2]), dw) if len(i.refl) else dw
        d_refl = np.zeros_like(i.refl)
        d_refl[i.inv[row]] = (w[:, None] * gr)[row]
    d_normals = None
    if want_ori:
        go = i.d_ori[r]
        neg = nd < 0
        dw = np.where(neg, dw + go * nd * nd, dw)
        k = go * w * F32(2) * nd
        d_normals = np.where(neg[:, None], -k[:, None] * d, F32(0)).astype(F32)
    return {"rgb_lin": lin, "acc": acc, "ori": ori if want_ori else None, "rgb_map": rgb_map.astype(F32), "d_weight": dw.astype(F32),
            "d_refl": d_refl, "d_normals": d_normals, "bg_adjoint": ((F32(1) - acc)[:, None] * i.d_rgb).astype(F32)}


def ray_errors(got, ref, i, flags):
    """metric -> largest |got - float64| over every element; rgb_map against the float64 tonemap and blend of got's OWN sums"""
    out = {}
    for m in RAY_METRICS:
        if ref[m] is None:
            continue
        want = rgb_map_of(i, flags, got["rgb_lin"], got["acc"]) if m == "rgb_map" else ref[m]
        assert got[m].shape == want.shape, (m, got[m].shape, want.shape)
        out[m] = _big(np.asarray(got[m], dtype=F64) - want)
    return out


def margins(own, ref, metrics):
    """metric -> max(8 x the restatement's error, 2^-23 x the largest |reference|)"""
    return {m: max(8 * own[m], FLOOR * _big(ref[m])) for m in metrics if m in own}


# ---- bounce rows ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_inputs_of(Mb):
    """Mb bounce rows among M ~ 2.5 Mb samples with a sorted ray_id: per-sample normals / app / heads / noise / xyzt, bidx, inv, rays,
    conv and the row adjoints dN, dr1, df0, ddiff, dfeat.  Row 0 has a zero normal and row 1 h9 == MIN_ROUGH where there are two rows."""
    rng = np.random.default_rng([11, Mb])
    M = int(2.5 * Mb) + 1
    B = max(M // 7, 1)
    ray_id = np.sort(rng.integers(0, B, M)).astype(np.int32)
    bidx = np.sort(rng.permutation(M)[:Mb]).astype(np.int32)
    inv = np.full(M, -1, dtype=np.int32)
    inv[bidx] = np.arange(Mb, dtype=np.int32)
    rays = rng.standard_normal((B, 6)).astype(F32)
    normals = _clear_of_the_plane(rng.standard_normal((M, 3)).astype(F32), rays[ray_id, 3:6])
    heads = rng.uniform(0.0, 1.0, (M, 11)).astype(F32)
    close = np.abs(heads[:, 9].astype(F64) - MIN_ROUGH) < 2 * CLEAR
    heads[close, 9] += F32(0.01)
    if Mb >= 2:
        normals[bidx[0]] = 0.0
        heads[bidx[1], 9] = MIN_ROUGH
    g = lambda *s: rng.standard_normal(s).astype(F32)      # noqa: E731
    return _ro(SimpleNamespace(Mb=Mb, M=M, B=B, ray_id=ray_id, bidx=bidx, inv=inv, rays=rays, normals=normals, heads=heads,
                               app=g(M, 24), noise=g(M, 24), xyzt=g(M, 4), conv=g(9, 3), dN=g(Mb, 3), dr1=g(Mb), df0=g(Mb, 3),
                               ddiff=g(Mb, 3), dfeat=g(Mb, 24)))


def strided_adjoints(i, view):
    """the row adjoints as the step slices them: dN = rows[:, 0:3] and dr1 = rows[:, 3] of a [Mb, 7] (view) or [Mb, 4] buffer,
    df0 = rows6[:, 0:3], ddiff = rows6[:, 3:6]; the columns nobody may read hold 1e30 -> (rows, rows6) float32"""
    rows = np.full((i.Mb, 7 if view else 4), 1e30, dtype=F32)
    rows[:, 0:3], rows[:, 3] = i.dN, i.dr1
    return rows, np.concatenate([i.df0, i.ddiff], axis=1)


def rows_reference64(i, detach_n):
    """models/microfacet.py:297,304-316,352-361 in float64 on per-sample inputs, adjoints by autograd.  Forward outputs per bounce
    row, gradients per SAMPLE (zero on samples without a row) -> dict of float64 arrays"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))      # noqa: E731
    n, a, h = (t(x).requires_grad_(True) for x in (i.normals, i.app, i.heads))
    idx = torch.from_numpy(i.bidx.astype(np.int64))
    V = -t(i.rays)[torch.from_numpy(i.ray_id.astype(np.int64))][idx][:, 3:6]
    nr = n[idx]
    nn = nr.detach() if detach_n else nr
    N = nn * (V * nn).sum(-1, keepdim=True).sign()
    r1 = h[idx][:, 9].clip(min=MIN_ROUGH)
    E = (t(i.conv).reshape(1, 9, 3) * O.eval_sh9(nr.detach()).reshape(-1, 9, 1)).sum(1)
    f0, diffuse, feat = h[idx][:, 6:9], h[idx][:, 0:3] * E, a[idx] + t(i.noise)[idx] * ANOISE
    loss = (N * t(i.dN)).sum() + (r1 * t(i.dr1)).sum() + (f0 * t(i.df0)).sum() + (diffuse * t(i.ddiff)).sum() + (feat * t(i.dfeat)).sum()
    gn, ga, gh = torch.autograd.grad(loss, [n, a, h], allow_unused=True)
    gn = torch.zeros_like(n) if gn is None else gn
    return {"V": V.numpy(), "N": N.detach().numpy(), "r1": r1.detach().numpy(), "f0": f0.detach().numpy(),
            "diffuse": diffuse.detach().numpy(), "feat": feat.detach().numpy(), "xyz": i.xyzt[i.bidx][:, :3].astype(F64),
            "d_normals": gn.numpy(), "d_heads": gh.numpy(), "d_app": ga.numpy()}


def _sgn(v):
    return np.sign(v).astype(F32)


def rows_restatement32(i, detach_n, bufs=None, pitch=None):
    """k_bounce_prep_fwd / nmf_rows::prep_bwd_row in numpy float32 per bounce row, the adjoints read the way the kernels address them:
    element c of row t of a flat buffer at t * pitch + c.  bufs = (dN, dr1, df0, ddiff) flat buffers with their first elements where
    the kernel's pointers point, pitch = (sN, sr, sf, sd) -> forward outputs and d_normals / d_heads / d_app per ROW (float32)"""
    if bufs is None:
        bufs, pitch = (i.dN.ravel(), i.dr1.ravel(), i.df0.ravel(), i.ddiff.ravel()), (3, 1, 3, 3)
    t = np.arange(i.Mb)
    rd = lambda q, c: bufs[q][t * pitch[q] + c]            # noqa: E731
    n = i.normals[i.bidx]
    h = i.heads[i.bidx]
    d = i.rays[i.ray_id[i.bidx], 3:6]
    v = -d
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    s = _sgn((v[:, 0] * x + v[:, 1] * y) + v[:, 2] * z)
    Y = [np.full(i.Mb, 0.28209479177387814, dtype=F32), F32(0.4886025119029199) * y, F32(0.4886025119029199) * z,
         F32(0.4886025119029199) * x, F32(1.0925484305920792) * (x * y), F32(1.0925484305920792) * (y * z),
         F32(0.31539156525252005) * (F32(3) * (z * z) - F32(1)), F32(1.0925484305920792) * (x * z),
         F32(0.5462742152960396) * (x * x - y * y)]
    E = np.zeros((i.Mb, 3), dtype=F32)
    for c in range(3):
        for k in range(9):
            E[:, c] = E[:, c] + i.conv[k, c] * Y[k]
    s_b = _sgn(-((d[:, 0] * x + d[:, 1] * y) + d[:, 2] * z))
    gh = np.zeros((i.Mb, 11), dtype=F32)
    gn = np.zeros((i.Mb, 3), dtype=F32)
    for c in range(3):
        gh[:, c] = rd(3, c) * E[:, c]
        gh[:, 6 + c] = rd(2, c)
        if not detach_n:
            gn[:, c] = rd(0, c) * s_b
    gh[:, 9] = np.where(h[:, 9] >= F32(MIN_ROUGH), rd(1, 0), F32(0))
    return {"V": v, "N": n * s[:, None], "r1": np.maximum(h[:, 9], F32(MIN_ROUGH)), "f0": h[:, 6:9], "diffuse": h[:, 0:3] * E,
            "feat": i.app[i.bidx] + i.noise[i.bidx] * F32(ANOISE), "xyz": i.xyzt[i.bidx][:, :3], "d_normals": gn, "d_heads": gh,
            "d_app": i.dfeat.copy()}


def rows_of_reference(ref, i):
    """the per-sample gradients of rows_reference64 taken per bounce row (what row_inputs = 2 returns)"""
    out = dict(ref)
    for k in ("d_normals", "d_heads", "d_app"):
        out[k] = ref[k][i.bidx]
    return out


def errors_over(got, ref, metrics):
    out = {}
    for m in metrics:
        assert got[m].shape == ref[m].shape, (m, got[m].shape, ref[m].shape)
        out[m] = _big(np.asarray(got[m], dtype=F64) - ref[m])
    return out


# ---- material heads ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def heads_inputs(M):
    """feat [M,24] randn, W [11,24] with rows of norm 4 (pre-activations ~ N(0, 4^2): +-12 at three sigma), b [11], d_out [M,11] and a
    second adjoint add [M,24].  rough_bias = -1 leaves ~23 % of the roughness outputs below the clip 0.5 sigmoid = 0.01.  Rows 2 and 3
    (from 255 rows on) drive the first diffuse pre-activation to +-100: 1.5 x 100 is past where expf overflows."""
    rng = np.random.default_rng([13, M])
    W = rng.standard_normal((11, 24))
    W = (4.0 * W / np.linalg.norm(W, axis=1, keepdims=True)).astype(F32)
    b = rng.uniform(-0.5, 0.5, 11).astype(F32)
    feat = rng.standard_normal((M, 24)).astype(F32)
    if M >= 255:
        unit = W[0].astype(F64) / (W[0].astype(F64) ** 2).sum()
        feat[2], feat[3] = (100.0 * unit).astype(F32), (-100.0 * unit).astype(F32)
    # rows whose float64 roughness lies within 2e-3 of the clip are moved by 0.5 in the pre-activation, away from it, inside
    # span(W[9], W[10]) so that the other roughness output of the row keeps its place
    G = W[9:11].astype(F64)
    pinv = G.T @ np.linalg.inv(G @ G.T)
    for _ in range(3):
        a = feat.astype(F64) @ G.T + b[9:11].astype(F64) + HP[4]
        r = 0.5 / (1.0 + np.exp(-a))
        bad = np.abs(r - 0.01) < 2 * CLEAR
        if not bad.any():
            break
        rows = bad.any(axis=1)
        delta = np.where(bad, np.where(r >= 0.01, 0.5, -0.5), 0.0)
        feat[rows] = (feat[rows].astype(F64) + delta[rows] @ pinv.T).astype(F32)
    return _ro(SimpleNamespace(M=M, feat=feat, W=W, b=b, d_out=rng.standard_normal((M, 11)).astype(F32),
                               add=rng.standard_normal((M, 24)).astype(F32)))


def _head_sd(W, b):
    p = "model.diffuse_module."
    sd = {}
    for name, lo, hi in (("diffuse", 0, 3), ("tint", 3, 6), ("f0", 6, 9), ("roughness", 9, 11)):
        sd[p + name + "_mlp.0.weight"], sd[p + name + "_mlp.0.bias"] = W[lo:hi], b[lo:hi]
    return sd


def heads_reference64(feat, W, b, d_out, add=None):
    """oracle.material_heads (modules/render_modules.py:519-574) on doubles, adjoints by autograd -> out [M,11], d_feat (+ add), gW, gb"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))      # noqa: E731
    f, Wt, bt = t(feat).requires_grad_(True), t(W).requires_grad_(True), t(b).requires_grad_(True)
    cfg = O.Cfg(diffuse_mul=HP[0], diffuse_bias=HP[1], tint_bias=HP[2], f0_bias=HP[3], roughness_bias=HP[4])
    albedo, tint, f0, rr = O.material_heads(_head_sd(Wt, bt), cfg, f)
    out = torch.cat([albedo, tint, f0, rr], 1)
    gf, gW, gb = torch.autograd.grad((out * t(d_out)).sum(), [f, Wt, bt])
    if add is not None:
        gf = gf + t(add)
    return {"out": out.detach().numpy(), "d_feat": gf.numpy(), "gW": gW.numpy(), "gb": gb.numpy()}


def _fma32(a, x, y):
    return (a.astype(F64) + x.astype(F64) * y.astype(F64)).astype(F32)      # the product of two floats is exact in a double


def _sigm32(x):
    with np.errstate(over="ignore"):
        e = np.exp(-x.astype(F64)).astype(F32)
        return (F32(1) / (F32(1) + e)).astype(F32)


def heads_restatement32(feat, W, b, d_out, add=None, passes=None):
    """nmf_heads::heads_eval and k_heads_bwd in numpy float32: the dot products accumulated with an fma in k order from the bias, the
    activations with a correctly rounded exp, d_feat summed over the outputs in j order, the weight gradient as partial sums per
    256-row block (the rows of a block added exactly, rounded once) accumulated in fp32 in block order.
    passes=1: the blocks beyond the 1024 of the first pass of the grid are left out of gW / gb."""
    M = len(feat)
    mul, dbias, tbias, fbias, rbias = (F32(v) for v in HP)
    a = np.repeat(b[None, :], M, axis=0).astype(F32)
    for j in range(11):
        for k in range(24):
            a[:, j] = _fma32(a[:, j], np.broadcast_to(W[j, k], (M,)), feat[:, k])
    out = np.empty((M, 11), dtype=F32)
    da = np.empty((M, 11), dtype=F32)
    for j in range(11):
        g = d_out[:, j]
        if j < 3:
            s = _sigm32(_fma32(np.broadcast_to(dbias, (M,)), np.broadcast_to(mul, (M,)), a[:, j]))
            out[:, j] = np.minimum(np.maximum(s, F32(0)), F32(1))
            da[:, j] = g * s * (F32(1) - s) * mul
        elif j < 9:
            s = _sigm32(a[:, j] + (tbias if j < 6 else fbias))
            out[:, j] = s
            da[:, j] = g * s * (F32(1) - s)
        else:
            s = _sigm32(a[:, j] + rbias)
            r = F32(0.5) * s
            out[:, j] = np.minimum(np.maximum(r, F32(0.01)), F32(1))
            da[:, j] = np.where((r >= F32(0.01)) & (r <= F32(1)), g * F32(0.5) * s * (F32(1) - s), F32(0))
    df = np.zeros((M, 24), dtype=F32)
    for j in range(11):
        for k in range(24):
            df[:, k] = _fma32(df[:, k], da[:, j], np.broadcast_to(W[j, k], (M,)))
    if add is not None:
        df = add + df
    n_blk = -(-M // 256)
    if passes is not None:
        n_blk = min(n_blk, 1024 * passes)
    gW, gb = np.zeros((11, 24), dtype=F32), np.zeros(11, dtype=F32)
    da64, f64 = da.astype(F64), feat.astype(F64)
    for blk in range(n_blk):
        rows = slice(256 * blk, min(256 * blk + 256, M))
        gW = gW + (da64[rows].T @ f64[rows]).astype(F32)
        gb = gb + da64[rows].sum(0).astype(F32)
    return {"out": out, "d_feat": df.astype(F32), "gW": gW, "gb": gb, "da": da}


def heads_gate_distance(i):
    a = i.feat.astype(F64) @ i.W[9:11].astype(F64).T + i.b[9:11].astype(F64) + HP[4]
    r = 0.5 / (1.0 + np.exp(-a))
    return r, float(np.abs(r - 0.01).min())


@functools.lru_cache(maxsize=None)
def heads_case(M, with_add):
    """(float64 reference, restatement's errors, margins) of the heads at M rows, computed once"""
    i = heads_inputs(M)
    add = i.add if with_add else None
    ref = heads_reference64(i.feat, i.W, i.b, i.d_out, add)
    own = errors_over(heads_restatement32(i.feat, i.W, i.b, i.d_out, add), ref, HEAD_METRICS)
    return ref, own, margins(own, ref, HEAD_METRICS)


@functools.lru_cache(maxsize=None)
def rows_case(Mb, detach_n):
    """(float64 reference with per-sample gradients, restatement's errors per row, margins) of the bounce rows, computed once"""
    i = row_inputs_of(Mb)
    ref = rows_reference64(i, detach_n)
    own = errors_over(rows_restatement32(i, detach_n), rows_of_reference(ref, i), ROW_METRICS)
    return ref, own, margins(own, rows_of_reference(ref, i), ROW_METRICS)


def ray_case(i, flags, weight=None):
    """(float64 reference, restatement's errors, margins) of ray compose on a batch under a combination of flags"""
    ref = ray_reference64(i, flags, weight)
    own = ray_errors(ray_restatement32(i, flags, weight), ref, i, flags)
    mg = margins(own, ref, RAY_METRICS)
    return ref, own, mg


# what tests/test_hip_parity.py allows the same quantities (atol, rtol): no margin here may be looser
def parity_tolerance(metric, scale):
    if metric in ("rgb_lin", "rgb_map"):
        return 2e-6 + 2e-5 * scale
    if metric in ("acc", "ori"):
        return 1e-6 + 2e-5 * scale
    if metric in ("d_weight", "d_refl", "d_normals", "bg_adjoint"):
        return 1e-5 * max(scale, 1.0) + 1e-4 * scale
    if metric in HEAD_METRICS[1:]:
        return 2e-5 * (scale + 1e-3) + 2e-4 * scale
    return 1e-6 + 1e-5 * scale                              # heads out, bounce prep


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_batches_have_the_shapes_they_are_named_for():
    lad = set(ladder())
    for name, b in RAY_BATCHES.items():
        i = ray_inputs(name)
        counts = np.diff(i.offsets)
        assert i.b == b and set(counts.tolist()) == lad and counts[0] == counts[-1] == counts[b // 2] == counts[b // 2 + 1] == 0
        assert len(i.weight) == len(i.inv) == len(i.normals) == len(i.ray_id) == i.offsets[-1] <= 1_300_000
        assert i.inv.max() == len(i.refl) - 1 and i.ray_id.max() < b and (np.diff(i.inv[i.inv >= 0]) == 1).all()
        assert 0 <= i.weight.min() and i.weight.max() <= 0.02 and 0 <= i.refl.min() and i.refl.max() <= 2
        acc = np.bincount(i.ray_id, weights=i.weight.astype(F64), minlength=b)
        assert acc.max() < 1.0, acc.max()
        share = (i.inv >= 0).mean()
        assert 0.5 < share < 0.65, share
    assert RAY_BATCHES["partial"] % 4 == 3 and RAY_BATCHES["last64"] == WPR_MAX_RAYS and RAY_BATCHES["narrow"] % 32 == 5
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193, 257} <= lad and {7, 8, 9, 15, 16, 17, 23, 24, 25} <= lad
    for name in ("one", "knee", "knee_up"):
        i = ray_inputs(name)
        assert i.b == 1 and len(i.weight) == 1
    e = ray_inputs("empty5")
    assert e.b == 5 and len(e.weight) == 0 and e.offsets.tolist() == [0] * 6
    assert ray_inputs("knee").refl[0, 0] == KNEE32 and ray_inputs("knee").weight[0] == 1.0
    assert ray_inputs("knee_up").refl[0, 0] > KNEE32 and ray_inputs("knee_up").refl[0, 0] - KNEE32 < 3e-10
    for Mb in ROW_COUNTS:
        i = row_inputs_of(Mb)
        assert len(i.bidx) == Mb and (np.diff(i.ray_id) >= 0).all() and (np.diff(i.bidx) > 0).all() and 2.4 * Mb < i.M < 2.6 * Mb + 2
        assert (i.inv[i.bidx] == np.arange(Mb)).all() and int((i.inv >= 0).sum()) == Mb and i.ray_id.max() < i.B
    assert HEAD_ROWS[-1] == 1024 * 256 + 257 and -(-HEAD_ROWS[-1] // 256) == 1024 + 2 and HEAD_ROWS[-1] % 256 == 1


@pytest.mark.parametrize("name", list(RAY_BATCHES))
def test_every_gate_is_clear_or_exact_rays(name):
    """rays: |V.N| (the ndv < 0 gate), the sRGB knee and the clip of the tonemap output keep 1e-3 in float64; the exceptions are one
    zero normal and the ray channels whose rgb_lin is exactly 0 (a ray without a bounce row: both sides compute 12.92 * 0)"""
    g = ray_gate_distances(ray_inputs(name))
    print(name, "ndv", g.ndv, "knee", g.knee, "clip at 1", g.clip1, "clip at 0", g.clip0, "zero normals", g.zero_normals)
    assert g.ndv >= CLEAR and g.knee >= CLEAR and g.clip1 >= CLEAR and g.clip0 >= CLEAR and g.zero_normals == 1
    below, between, above = (g.lin < KNEE32) & (g.lin > 0), (g.lin > KNEE32) & (g.o < 1), g.o > 1
    print(name, "ray channels below the knee", int(below.sum()), "between", int(between.sum()), "clipped at 1", int(above.sum()))
    assert min(below.sum(), between.sum(), above.sum()) >= 0.01 * g.lin.size       # every side of both gates is populated


def test_every_gate_is_clear_or_exact_rows_and_heads():
    for Mb in ROW_COUNTS:
        i = row_inputs_of(Mb)
        n, d = i.normals[i.bidx].astype(F64), i.rays[i.ray_id[i.bidx], 3:6].astype(F64)
        dn, h9 = np.abs((n * d).sum(1)), i.heads[i.bidx, 9].astype(F64)
        zero, on = ~n.any(axis=1), h9 == MIN_ROUGH
        assert int(zero.sum()) == int(on.sum()) == (1 if Mb >= 2 else 0)
        assert dn[~zero].min(initial=np.inf) >= CLEAR and np.abs(h9[~on] - MIN_ROUGH).min(initial=np.inf) >= CLEAR
        if Mb >= 255:
            assert (h9 > MIN_ROUGH).mean() > 0.5 and (h9 < MIN_ROUGH).mean() > 0.1
    for M in HEAD_ROWS + ROW_COUNTS[-1:]:
        i = heads_inputs(M)
        r, dist = heads_gate_distance(i)
        print(M, "roughness gate: distance", dist, "share below", (r < 0.01).mean())
        assert dist >= CLEAR
        if M >= 255:
            assert 0.05 <= (r < 0.01).mean() <= 0.95


def test_heads_inputs_span_the_tails():
    """pre-activations beyond +-12, and the two rows that push expf past its range"""
    i = heads_inputs(HEAD_ROWS[-1])
    a = i.feat.astype(F64) @ i.W.astype(F64).T + i.b.astype(F64)
    assert a[4:].max() > 12 and a[4:].min() < -12 and a[2, 0] > 99 and a[3, 0] < -99
    ref, _, _ = heads_case(HEAD_ROWS[-1], False)
    assert all(np.isfinite(v).all() for v in ref.values())
    own = heads_restatement32(i.feat[:4], i.W, i.b, i.d_out[:4])
    assert all(np.isfinite(v).all() for v in own.values()) and own["da"][2, 0] == 0 and own["da"][3, 0] == 0


def test_tonemap64_is_the_oracle_off_the_knee():
    x = torch.linspace(-0.5, 2.5, 30001, dtype=torch.float64)
    x = x[(x - 0.0031308).abs() > 1e-9]
    for noclip in (False, True):
        assert torch.equal(tonemap64(x, noclip), O.srgb_tonemap(x, noclip=noclip))
    assert abs(float(KNEE32) - 0.0031308) < 2e-10


def test_lane_walk_restatement_is_the_strided_two_per_pass_order():
    """terms 1e8, 1, -1e8 placed where one lane meets them in that order (k, k + W, k + 2 W) lose the 1; placed in lanes of their own
    they do not"""
    for W in (64, 8):
        off = np.array([0, 3 * W + 1], dtype=np.int64)
        t = np.zeros((3 * W + 1, 1), dtype=F32)
        t[[5, 5 + W, 5 + 2 * W], 0] = (1e8, 1.0, -1e8)
        assert lane_walk32(t, off, W)[0, 0] == 0.0
        t[:] = 0
        t[[5, 6, 5 + 2 * W], 0] = (1e8, 1.0, -1e8)
        assert lane_walk32(t, off, W)[0, 0] == 1.0
        t[:] = 0
        t[3 * W - 1] = 1.0                                    # lane W - 1, the k sample of the second pass
        assert lane_walk32(t, off, W)[0, 0] == 1.0 and lane_walk32(t, off, W, fault="second")[0, 0] == 1.0
        t[3 * W] = 2.5                                        # lane 0, the k + W sample of the second pass: the last of 3 W + 1
        assert lane_walk32(t, off, W)[0, 0] == 3.5 and lane_walk32(t, off, W, fault="second")[0, 0] == 1.0


def test_small_ray_batches():
    for name in ("one", "knee", "knee_up"):
        i = ray_inputs(name)
        for flags in FLAGS:
            ref, own, mg = ray_case(i, flags)
            w, c = float(i.weight[0]), i.refl[0].astype(F64)
            assert ref["acc"][0] == w and np.allclose(ref["rgb_lin"][0], w * c * flags[4], rtol=1e-15, atol=0)
            assert all(own[m] <= mg[m] / 2 or own[m] == 0 for m in own)
    # on the knee the kernel's comparison x > limit is false: the linear branch and its slope; one float above, the power branch
    T = (True, False, True, False, True)
    on, up = ray_reference64(ray_inputs("knee"), T), ray_reference64(ray_inputs("knee_up"), T)
    assert np.allclose(on["d_refl"][0], 12.92 * ray_inputs("knee").d_rgb[0].astype(F64), rtol=1e-14)
    slope = up["d_refl"][0] / ray_inputs("knee_up").d_rgb[0].astype(F64)
    assert np.all(np.abs(slope - 12.70) < 0.01), slope
    own = ray_restatement32(ray_inputs("knee"), T)
    assert np.all(own["rgb_map"][0] == F32(12.92) * KNEE32)      # acc == 1: no background
    e = ray_inputs("empty5")
    for flags in FLAGS:
        ref = ray_reference64(e, flags)
        own = ray_restatement32(e, flags)
        assert ref["acc"].tolist() == [0.0] * 5 and own["acc"].tolist() == [0.0] * 5 and own["d_weight"].shape == (0,)
        assert np.array_equal(own["rgb_map"], np.broadcast_to(e.bg_ray if flags[2] else e.bg_one, (5, 3)))


def test_background_adjoint_is_the_autograd_gradient():
    i = ray_inputs("partial")
    per_ray, shared = ray_reference64(i, LEVEL1), ray_reference64(i, (False, False, False, False, True))
    assert np.array_equal(per_ray["d_bg"], per_ray["bg_adjoint"])
    assert np.allclose(shared["d_bg"], shared["bg_adjoint"].sum(0, keepdims=True), rtol=1e-12)


@pytest.mark.parametrize("name", list(RAY_BATCHES))
def test_margins_are_not_looser_than_the_fp32_tests_rays(name):
    """under the flags with the most arithmetic (tonemap with the clip, orientation term, bounce rows), with the per-ray and the
    shared background, and in the form of the levels >= 1"""
    i = ray_inputs(name)
    for flags in ((True, False, True, True, True), (True, True, False, True, True), LEVEL1):
        ref, own, mg = ray_case(i, flags)
        for m in mg:
            print(f"{name} {flag_id(flags)} {m}: restatement {own[m]:.3e} margin {mg[m]:.3e} scale {_big(ref[m]):.3e}")
        for m in mg:
            assert mg[m] <= parity_tolerance(m, _big(ref[m])), (m, mg[m])
            assert own[m] <= mg[m] / 2 or own[m] == 0.0


def test_margins_are_not_looser_than_the_fp32_tests_rows_and_heads():
    for Mb in ROW_COUNTS:
        for detach_n in (False, True):
            ref, own, mg = rows_case(Mb, detach_n)
            rr = rows_of_reference(ref, row_inputs_of(Mb))
            for m in mg:
                assert mg[m] <= parity_tolerance("rows", _big(rr[m])), (Mb, m, mg[m])
            if detach_n:
                assert _big(ref["d_normals"]) == 0.0 and mg["d_normals"] == 0.0
    for M in HEAD_ROWS:
        for with_add in (False, True):
            ref, own, mg = heads_case(M, with_add)
            for m in mg:
                print(f"heads {M} add={with_add} {m}: restatement {own[m]:.3e} margin {mg[m]:.3e} scale {_big(ref[m]):.3e}")
            for m in mg:
                assert mg[m] <= parity_tolerance(m, _big(ref[m])), (M, m, mg[m])


@pytest.mark.parametrize("Mb", ROW_COUNTS)
def test_pitch_of_the_strided_adjoints_is_what_the_restatement_reads(Mb):
    """the restatement on the column slices of the [Mb, 7] / [Mb, 4] / [Mb, 6] buffers with their pitches == on the dense adjoints, bit
    for bit (the reference side of the GPU test of the same name)"""
    i = row_inputs_of(Mb)
    dense = rows_restatement32(i, False)
    for view in (False, True):
        rows, rows6 = strided_adjoints(i, view)
        p = rows.shape[1]
        got = rows_restatement32(i, False, (rows.ravel(), rows.ravel()[3:], rows6.ravel(), rows6.ravel()[3:]), (p, p, 6, 6))
        assert all(np.array_equal(got[m], dense[m]) for m in ROW_METRICS)


def test_broken_restatements_miss_their_margins():
    """the three faults this file is there for, built into the restatement: each misses its margin a thousandfold"""
    flags = (False, False, True, True, True)
    for name in ("partial", "narrow"):
        i = ray_inputs(name)
        ref, own, mg = ray_case(i, flags)
        err = ray_errors(ray_restatement32(i, flags, fault="second"), ref, i, flags)
        for m in ("acc", "rgb_lin", "ori"):
            print(f"second-pass sample dropped, {name} {m}: {err[m]:.3e} = {err[m] / mg[m]:.3g} x margin")
            assert err[m] >= 1000 * mg[m], (name, m)
    for Mb in ROW_COUNTS[1:]:
        i = row_inputs_of(Mb)
        ref, own, mg = rows_case(Mb, False)
        rows, rows6 = strided_adjoints(i, True)
        pad = np.concatenate([rows.ravel(), np.zeros(8, dtype=F32)])
        got = rows_restatement32(i, False, (pad, pad[3:], rows6.ravel(), rows6.ravel()[3:]), (3, 3, 6, 6))
        err = errors_over(got, rows_of_reference(ref, i), ("d_normals", "d_heads"))
        for m in err:
            print(f"pitch 3 on the pitch-7 buffer, {Mb} rows {m}: {err[m]:.3e} = {err[m] / mg[m]:.3g} x margin")
            assert err[m] >= 1000 * mg[m], (Mb, m)
    M = HEAD_ROWS[-1]
    i = heads_inputs(M)
    ref, own, mg = heads_case(M, False)
    err = errors_over(heads_restatement32(i.feat, i.W, i.b, i.d_out, passes=1), ref, ("gW", "gb"))
    for m in err:
        print(f"second grid pass skipped, {m}: {err[m]:.3e} = {err[m] / mg[m]:.3g} x margin")
        assert err[m] >= 1000 * mg[m], m
