"""Compositing without a GPU: the inputs, the float64 reference, the fp32 restatement of csrc/composite.hip and the margins that the
GPU tests (tests/test_hip_composite.py) hold the kernels to, and the tests that show those margins are neither vacuous nor blind.

The inputs are built so that a fault in the chunk loops cannot hide: ray lengths sit around the multiples of the lane-group widths
(8, 16, 64) up to 257 samples, and the opacity is low enough that the last sample of the longest ray still carries a weight above
1e-4 (`medium`), next to regimes with a saturated surface inside the ray (`wall`, `hard`) and with exact zeros (`zeros`)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nmf_oracle as O

SCALE = 25.0                           # distance_scale of every test here
F32, F64 = np.float32, np.float64
FLOOR = 2.0 ** -23                     # no margin below one ulp of 1.0f


def ladder():
    """segment lengths around every multiple of 8, 16 and 64 (the lane-group widths) and around 4 x SLOTS of segment_sum_wide"""
    return (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193,
            200, 255, 256, 257)


# name -> (rays, seed).  partial: 64 lanes per ray, 3 rays in the last workgroup; last64: the largest batch of the 64-lane kernels;
# narrow: 8 (forward) / 16 (backward) lanes per ray, 5 rays in the last workgroup of both.  The seeds are those for which the
# `medium` condition min w64 >= 1e-4 holds (test_medium_leaves_no_sample_out_of_the_relative_metric).
BATCHES = {"partial": (4 * len(ladder()) + 3, 0), "last64": (16384, 0), "narrow": (16384 + 37, 0)}
REGIMES = ("medium", "wall", "hard", "zeros")
METRICS = ("w", "acc", "dsigma", "wrel")
OPAQUE = 100.0                         # sigma from here on is a wall sample (ex <= 0.14)
WPR_MAX_RAYS = 16384                   # csrc/composite.hip: batches up to this size walk a ray with 64 lanes, larger ones with 8 / 16


def regimes():
    return REGIMES


def metrics_of(regime):
    """w, acc and dsigma everywhere; wrel where every sample carries weight; dsigma_dark where rays without a translucent sample exist"""
    return METRICS if regime == "medium" else METRICS[:3] + ("dsigma_dark",) if regime == "wall" else METRICS[:3]


def _offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def _mask(counts):
    """dense [b, N] mask, kept samples first: the compacted order is the row-major order of its True entries"""
    n = max(int(counts.max()), 1) if len(counts) else 1
    return np.arange(n)[None, :] < np.asarray(counts)[:, None]


def batch(b, seed):
    """ray r has ladder()[r % len] samples (ray 0 is empty); the last ray and the neighbours b // 2, b // 2 + 1 are emptied too.
    -> offsets [b + 1] int64, dense mask [b, N], dist [M] float32 in [0.8, 1.2] 1e-3"""
    lad = np.asarray(ladder(), dtype=np.int64)
    counts = lad[np.arange(b) % len(lad)]
    counts[[b - 1, b // 2, b // 2 + 1]] = 0
    off = _offsets(counts)
    dist = np.random.default_rng([seed, b, 0]).uniform(0.8e-3, 1.2e-3, int(off[-1])).astype(F32)
    return off, _mask(counts), dist


def _regime(regime, off, mask, dist, seed):
    """-> sigma, dist [M] float32 of a regime on the rays of a batch"""
    b = len(off) - 1
    counts = np.diff(off)
    # medium: sigma in [0.25, 1], alpha in [0.005, 0.03].  The square of a uniform variate keeps the range and puts the mean at 0.5:
    # T is ~0.04 behind 257 samples and the smallest weight ~1.5e-4.  A uniform sigma (mean 0.625) leaves T ~ 0.018 there, and among
    # the ~480 longest rays of the large batches some late sample always has alpha ~ 0.005: the smallest weight never came out above
    # 9.1e-5 over 400 seeds, short of the 1e-4 that test_medium_leaves_no_sample_out_of_the_relative_metric requires.
    sigma = (0.25 + 0.75 * np.random.default_rng([seed, b, 1]).uniform(0.0, 1.0, len(dist)) ** 2).astype(F32)
    mid = off[:-1] + counts // 2
    inner = counts >= 3                                   # the opaque samples keep a neighbour on either side
    if regime == "wall":                                  # ex = exp(-sigma d) from 0.08 down to ~1e-9: f = 1 - alpha + 1e-10 loses its bits
        at = (mid[inner][:, None] + np.arange(-1, 2)[None, :]).reshape(-1)
        sigma[at] = np.random.default_rng([seed, b, 2]).uniform(100.0, 800.0, len(at)).astype(F32)
    elif regime == "hard":                                # ex == 0, alpha == 1, f == 1e-10: the backward divides by it
        sigma[mid[inner]] = F32(1e6)
    elif regime == "zeros":
        ray, col = np.nonzero(mask)
        sigma[ray % 5 == 0] = 0                           # alpha == 0, f == 1.0f exactly, along the whole ray
        dist = dist.copy()
        dist[col % 7 == 6] = 0                            # (never column 0: every ray keeps a sample with a gradient)
    elif regime != "medium":
        raise KeyError(regime)
    return sigma, dist


def _ns(off, mask, sigma, dist, dw):
    for a in (off, mask, sigma, dist, dw):
        a.setflags(write=False)
    return SimpleNamespace(b=len(off) - 1, offsets=off, mask=mask, sigma=sigma, dist=dist, d_weight=dw, scale=SCALE)


@functools.lru_cache(maxsize=None)
def inputs(name, regime):
    """the arrays of one (batch, regime), built once and read-only: b, offsets, mask, sigma, dist, d_weight, scale"""
    if name == "one":                                     # one ray, one sample
        off, mask = np.array([0, 1], dtype=np.int64), np.ones((1, 1), dtype=bool)
        return _ns(off, mask, np.array([0.7], dtype=F32), np.array([1.1e-3], dtype=F32), np.array([-1.3], dtype=F32))
    if name == "empty5":                                  # five rays, no sample at all
        e = np.zeros(0, dtype=F32)
        return _ns(np.zeros(6, dtype=np.int64), np.zeros((5, 1), dtype=bool), e, e.copy(), e.copy())
    b, seed = BATCHES[name]
    off, mask, dist = batch(b, seed)
    sigma, dist = _regime(regime, off, mask, dist, seed)
    dw = np.random.default_rng([seed, b, 3]).standard_normal(len(dist)).astype(F32)
    return _ns(off, mask, sigma, dist, dw)


def dense(v, mask, fill=0.0):
    out = np.full(mask.shape, fill, dtype=v.dtype)
    out[mask] = v
    return out


# ---- float64: the definition ---------------------------------------------------------------------------------------------------------
def reference64(sigma, dist, offsets, scale, d_weight):
    """the header of csrc/composite.hip in float64 on the float32 inputs:  a_k = 1 - exp(-sigma_k dist_k scale),  f_k = 1 - a_k + 1e-10,
    T_k = prod_{j<k} f_j,  w_k = a_k T_k,  acc = sum_k w_k;  d_sigma = d (sum_k d_weight_k w_k) / d sigma by autograd.
    -> weight [M], acc [b], d_sigma [M] (float64 numpy)"""
    mask = _mask(np.diff(offsets))
    m = torch.from_numpy(mask)
    t = lambda v: torch.from_numpy(dense(np.asarray(v, dtype=F64), mask))      # noqa: E731  (padding: sigma = 0 behind the last sample)
    s = t(sigma).requires_grad_(True)
    alpha = 1.0 - torch.exp(-s * (t(dist) * float(scale)))
    f = torch.cat([torch.ones(mask.shape[0], 1, dtype=torch.float64), 1.0 - alpha + 1e-10], dim=-1)
    w = alpha * torch.cumprod(f, dim=-1)[:, :-1]
    (g,) = torch.autograd.grad((w * t(d_weight)).sum(), s)
    return w.detach()[m].numpy(), w.detach().sum(1).numpy(), g[m].numpy()


def oracle32(sigma, dist, offsets, scale, d_weight):
    """the CPU oracle (raw2alpha + autograd, float32) on the dense, zero-padded form -> weight, acc, d_sigma"""
    mask = _mask(np.diff(offsets))
    m = torch.from_numpy(mask)
    t = lambda v: torch.from_numpy(dense(np.asarray(v, dtype=F32), mask))      # noqa: E731
    s = t(sigma).requires_grad_(True)
    w = O.raw2alpha(s, t(dist) * float(scale))
    (g,) = torch.autograd.grad((w * t(d_weight)).sum(), s)
    return w.detach()[m].numpy(), w.detach().sum(1).numpy(), g[m].numpy()


# ---- fp32: the kernel's arithmetic ---------------------------------------------------------------------------------------------------
def restatement32(sigma, dist, offsets, scale, d_weight, fault=None):
    """csrc/composite.hip in numpy, in the kernel's expression order: fp32 alpha, f and d ex; the transmittance a float64 running
    product rounded to fp32 per element; the suffix sum of d_weight w in float64 with an fp32 quotient; the two terms of d_sigma
    added in fp32; the per-ray opacity summed in fp32 the way the forward's lane group does (every lane its own samples in index
    order, then the shuffle tree).  exp is evaluated in float64 and rounded once (correctly rounded, whatever the host's libm does
    in float32).  -> weight, acc, d_sigma (float32)

    fault (the tests' deliberately broken variants): ("carry", W, c) forgets what the chunks in front of chunk c of a W-lane group
    carried, in the product and (from the back) in the suffix sum; "shift" reads the inclusive product of the own lane where the
    exclusive one belongs."""
    counts = np.diff(offsets)
    mask = _mask(counts)
    one = F32(1)
    d = np.asarray(dist, dtype=F32) * F32(scale)
    ex = np.exp(-(np.asarray(sigma, dtype=F32) * d).astype(F64)).astype(F32)
    alpha = one - ex
    f = (one - alpha) + F32(1e-10)
    incl = np.cumprod(dense(f.astype(F64), mask, 1.0), axis=1)
    T = np.concatenate([np.ones((mask.shape[0], 1)), incl[:, :-1]], axis=1)
    if fault == "shift":
        T = incl
    elif fault is not None:
        _, W, c = fault
        if T.shape[1] > c * W:
            T[:, c * W:] /= T[:, c * W:c * W + 1].copy()
    T = T.astype(F32)[mask]
    w = alpha * T
    W = 64 if len(counts) <= WPR_MAX_RAYS else 8
    lanes = np.zeros((mask.shape[0], -(-mask.shape[1] // W) * W), dtype=F32)
    lanes[:, :mask.shape[1]] = dense(w, mask)
    lanes = np.cumsum(lanes.reshape(len(counts), -1, W), axis=1, dtype=F32)[:, -1]
    while W > 1:
        W //= 2
        lanes = lanes[:, :W] + lanes[:, W:2 * W]
    acc = lanes[:, 0]
    # backward
    v = dense(np.asarray(d_weight, dtype=F64) * w.astype(F64), mask)
    suffix = np.cumsum(v[:, ::-1], axis=1)[:, ::-1] - v
    if fault not in (None, "shift"):
        _, W, c = fault
        rows = np.nonzero(counts > c * W)[0]
        first = counts[rows] - c * W                    # column of the first sample of the last c chunks
        tail = suffix[rows, first - 1]                  # = the sum over those chunks
        cols = np.arange(mask.shape[1])[None, :] < first[:, None]
        suffix[rows] -= np.where(cols, tail[:, None], 0.0)
    dex = d * ex
    ds = (-suffix[mask].astype(F32) / f) * dex + (np.asarray(d_weight, dtype=F32) * T) * dex
    return w, acc, ds


def sequential_sum32(vals, scale, offsets):
    """out[r] = the fp32 sum of scale[k] vals[k] over the segment in index order, acc = fl(acc + fl(sc v)): what
    segment_sum(lanes=1) promises bit for bit.  vals [M, D] float32, scale [M] float32 or None -> [n_seg, D] float32"""
    vals = np.asarray(vals, dtype=F32)
    counts = np.diff(offsets)
    out = np.zeros((len(counts), vals.shape[1]), dtype=F32)
    for col in range(int(counts.max()) if len(counts) else 0):
        rows = np.nonzero(counts > col)[0]
        k = offsets[rows] + col
        term = vals[k] if scale is None else np.asarray(scale, dtype=F32)[k, None] * vals[k]
        out[rows] = out[rows] + term
    return out


# ---- metrics and margins -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, regime):
    """reference64 of a batch (computed once, shared by the CPU and GPU tests, read-only) + the largest |d_sigma| of every ray"""
    i = inputs(name, regime)
    w, acc, ds = reference64(i.sigma, i.dist, i.offsets, i.scale, i.d_weight)
    rowmax = dense(np.abs(ds), i.mask).max(axis=1)
    for a in (w, acc, ds, rowmax):
        a.setflags(write=False)
    # a ray of nothing but wall samples (three samples in `wall`) has no gradient to speak of: its largest |d_sigma| is ~1e-9 down
    # to 1e-13 and hangs on the bits that 1 - alpha loses (right fp32 arithmetic is off by 0.4 of it), so the row-relative metric
    # covers the rays that keep a translucent sample, and the others are compared absolutely (dsigma_dark)
    lit = dense(i.sigma < OPAQUE, i.mask).any(axis=1)
    lit.setflags(write=False)
    return SimpleNamespace(w=w, acc=acc, d_sigma=ds, rowmax=rowmax, lit=lit)


def errors(got, ref, offsets, relative):
    """metric -> the largest error of got = (weight, acc, d_sigma) against a reference() over the kept samples: |dw|, |dacc|,
    |d d_sigma| / the ray's largest |d_sigma64| (dsigma_dark: |d d_sigma| on the rays without a translucent sample), and
    (relative=True) |dw| / w64 over EVERY sample"""
    w, acc, ds = (np.asarray(a, dtype=F64) for a in got)
    ray = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    big = lambda a: float(a.max()) if a.size else 0.0      # noqa: E731
    lit = ref.lit[ray]
    out = {"w": big(np.abs(w - ref.w)), "acc": big(np.abs(acc - ref.acc)),
           "dsigma": big(np.abs(ds - ref.d_sigma)[lit] / ref.rowmax[ray][lit]), "dsigma_dark": big(np.abs(ds - ref.d_sigma)[~lit])}
    if relative:
        out["wrel"] = big(np.abs(w - ref.w) / ref.w)
    return out


@functools.lru_cache(maxsize=None)
def restated(name, regime):
    """errors() of the restatement on a batch"""
    i = inputs(name, regime)
    got = restatement32(i.sigma, i.dist, i.offsets, i.scale, i.d_weight)
    return errors(got, reference(name, regime), i.offsets, regime == "medium")


def margin(metric, regime):
    """the tolerance of the kernels against reference64: 8 x the restatement's largest error over the three batches, at least 2^-23.
    The restatement has the kernel's roundings but a correctly rounded exp; the device's expf is allowed an ulp, which on
    alpha = 1 - ex near ex = 1 is the whole of these errors (the same arithmetic with a float32 libm exp measured 3.0 - 3.6 x the
    restatement's error), and 8 leaves a factor of two over that.  An off-by-one scan is 0.5 - 3 % in `medium`, a dropped carry a
    factor."""
    return max(8 * max(restated(name, regime)[metric] for name in BATCHES), FLOOR)


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
CASES = [(r, n) for r in REGIMES for n in BATCHES]


def test_batches_have_the_shapes_they_are_named_for():
    lad = ladder()
    assert len(lad) == 34 and lad[0] == 0 and max(lad) == 257
    for name, (b, _) in BATCHES.items():
        i = inputs(name, "medium")
        counts = np.diff(i.offsets)
        assert i.b == b and counts[0] == 0 and counts[-1] == 0 and counts[b // 2] == 0 and counts[b // 2 + 1] == 0
        assert set(counts.tolist()) == set(lad) and int(i.mask.sum()) == len(i.sigma) == i.offsets[-1] <= 1_300_000
        assert 0.8e-3 * (1 - 1e-7) <= i.dist.min() and i.dist.max() <= 1.2e-3 * (1 + 1e-7)
    assert BATCHES["partial"][0] % 4 == 3 and BATCHES["last64"][0] == 16384               # 4 rays per workgroup at 64 lanes
    assert BATCHES["narrow"][0] % 32 == 5 and BATCHES["narrow"][0] % 16 == 5             # 32 (forward) and 16 (backward)
    z = inputs("partial", "zeros")
    ray, col = np.nonzero(z.mask)
    assert (z.sigma[ray % 5 == 0] == 0).all() and (z.dist[col % 7 == 6] == 0).all() and (z.dist[col == 0] > 0).all()
    h = inputs("partial", "hard")
    assert int((h.sigma == 1e6).sum()) == int((np.diff(h.offsets) >= 3).sum())
    ex = np.exp(-h.sigma[h.sigma == 1e6] * (h.dist[h.sigma == 1e6] * F32(SCALE)))
    assert (ex == 0).all()
    wl = inputs("partial", "wall")
    assert int((wl.sigma >= 100).sum()) == 3 * int((np.diff(wl.offsets) >= 3).sum()) and wl.sigma.max() <= 800


@pytest.mark.parametrize("regime,name", CASES)
def test_restatement_and_oracle_stay_inside_half_the_margin(regime, name):
    """the tolerance is not vacuous: fp32 arithmetic that is right -- the restatement, and the float32 oracle on the dense form --
    meets it twice over"""
    i = inputs(name, regime)
    ref = reference(name, regime)
    own = restated(name, regime)
    orc = errors(oracle32(i.sigma, i.dist, i.offsets, i.scale, i.d_weight), ref, i.offsets, regime == "medium")
    for m in metrics_of(regime):
        print(f"{regime}/{name} {m}: restatement {own[m]:.3e} oracle {orc[m]:.3e} margin {margin(m, regime):.3e}")
    for m in metrics_of(regime):
        assert own[m] <= margin(m, regime) / 2, (m, own[m])
        assert orc[m] <= margin(m, regime) / 2, (m, orc[m])


@pytest.mark.parametrize("name", list(BATCHES))
def test_medium_leaves_no_sample_out_of_the_relative_metric(name):
    """every sample of every chunk carries weight: a wrong carry into the fifth chunk is as visible as one into the second"""
    w = reference(name, "medium").w
    print(name, "min w64", w.min())
    assert w.min() >= 1e-4


@pytest.mark.parametrize("regime,name", CASES)
def test_reference_is_finite_and_zero_on_empty_rays(regime, name):
    i = inputs(name, regime)
    ref = reference(name, regime)
    empty = np.diff(i.offsets) == 0
    assert empty.sum() >= 4 and (ref.acc[empty] == 0).all()
    assert all(np.isfinite(a).all() for a in (ref.w, ref.acc, ref.d_sigma))
    assert (ref.rowmax[~empty] > 0).all()                  # the row-relative metric divides by it
    dark = ~ref.lit & ~empty
    assert (np.diff(i.offsets)[dark] == 3).all() and bool(dark.any()) == (regime == "wall")
    got = restatement32(i.sigma, i.dist, i.offsets, i.scale, i.d_weight)
    assert all(np.isfinite(a).all() for a in got) and (got[1][empty] == 0).all()


def test_small_batches():
    i = inputs("one", "medium")
    ref = reference("one", "medium")
    a = 1 - np.exp(-float(i.sigma[0]) * float(i.dist[0]) * SCALE)
    assert abs(ref.w[0] - a) < 1e-15 and ref.acc[0] == ref.w[0]
    assert abs(ref.d_sigma[0] - float(i.d_weight[0]) * float(i.dist[0]) * SCALE * (1 - a)) < 1e-15
    e = inputs("empty5", "medium")
    w, acc, ds = restatement32(e.sigma, e.dist, e.offsets, e.scale, e.d_weight)
    assert w.shape == ds.shape == (0,) and (acc == 0).all() and acc.shape == (5,)


@pytest.mark.parametrize("fault", [("carry", 16, 2), "shift"], ids=["carry-dropped-at-chunk-3-of-16", "product-shifted-one-lane"])
def test_broken_variants_exceed_the_margin_a_hundredfold(fault):
    """the metrics cannot hide the faults they are there for: the restatement with the carry forgotten at the third 16-lane chunk, and
    with the inclusive product where the exclusive one belongs, misses every `medium` margin by two orders of magnitude"""
    for name in BATCHES:
        i = inputs(name, "medium")
        got = restatement32(i.sigma, i.dist, i.offsets, i.scale, i.d_weight, fault=fault)
        err = errors(got, reference(name, "medium"), i.offsets, True)
        for m in METRICS:
            print(f"{fault} {name} {m}: {err[m]:.3e} = {err[m] / margin(m, 'medium'):.0f} x margin")
            assert err[m] >= 100 * margin(m, "medium"), (name, m, err[m])


def test_sequential_sum_is_index_order():
    off = np.array([0, 0, 3, 4, 4], dtype=np.int64)
    vals = np.array([[1e8], [1.0], [-1e8], [0.25]], dtype=F32)
    out = sequential_sum32(vals, None, off)
    assert out.tolist() == [[0.0], [0.0], [0.25], [0.0]]                  # (1e8 + 1) - 1e8 in fp32: the 1 is lost
    sc = np.array([1.0, 3.0, 1.0, 0.1], dtype=F32)
    assert sequential_sum32(vals, sc, off)[2, 0] == F32(0.1) * F32(0.25)
