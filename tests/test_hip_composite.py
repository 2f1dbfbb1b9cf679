"""Compositing and segmented sums on the GPU: csrc/composite.hip (nmf_composite_fwd / _bwd, nmf_segment_sum), nmf_segment_sum_wide
(csrc/brdf.hip) and nmf_expand_segments (csrc/select.hip) against the float64 reference of tests/test_composite_cpu.py, on ray lengths
around every multiple of the lane-group widths, at the batch sizes where the kernels change and at opacities from 0 to 1.
Tolerance: test_composite_cpu.margin (8 x the error of the fp32 restatement, at least 2^-23).

Measured on an MI355X: error of the kernels / error of the restatement, both against float64, the largest of the three batches
(the margin sits at 8; the device's expf accounts for what is above 1):
    regime   w     acc   dsigma  wrel / dsigma_dark
    medium   1.12  1.35  1.23    1.08
    wall     1.32  1.08  1.00    1.00
    hard     1.29  1.00  1.25
    zeros    1.12  1.46  1.31
The same 139 rays under 64 and under 8 / 16 lanes per ray: no weight differs in its bits in any regime, no d_sigma either except in
`wall` (3.0e-4 of the samples); acc differs on 8 - 23 % of the rays (the lane groups add a ray's weights in another association).
"""
import numpy as np
import pytest
import torch

from nmf_amd import hip
from nmf_amd.functional import Composite
from test_composite_cpu import (BATCHES, REGIMES, SCALE, errors, inputs, ladder, margin, metrics_of, reference, restated,
                                sequential_sum32)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.tensor(a).to(DEV)                # (a copy: the shared inputs are read-only)


def _run(i):
    """forward and backward through the wrappers -> (weight, acc, d_sigma) as numpy"""
    sigma, dist, off = _dev(i.sigma), _dev(i.dist), _dev(i.offsets)
    w, acc = hip.composite_fwd(sigma, dist, off, i.b, i.scale)
    ds = hip.composite_bwd(sigma, dist, w, off, i.b, i.scale, _dev(i.d_weight))
    return w.cpu().numpy(), acc.cpu().numpy(), ds.cpu().numpy()


def _check(got, ref, i, regime, what, own=None):
    empty = np.diff(i.offsets) == 0
    assert all(np.isfinite(a).all() for a in got), what
    assert (got[1][empty] == 0.0).all(), what
    err = errors(got, ref, i.offsets, regime == "medium")
    for m in metrics_of(regime):
        ratio = f" = {err[m] / own[m]:.2f} x restatement" if own and own[m] > 0 else ""
        print(f"{what} {m}: {err[m]:.3e}{ratio}, margin {margin(m, regime):.3e}")
    for m in metrics_of(regime):
        assert err[m] <= margin(m, regime), (what, m, err[m], margin(m, regime))


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("regime", REGIMES)
def test_composite_against_float64(regime, name):
    """weights, per-ray opacity and d_sigma inside the margin in every metric; acc exactly 0 on empty rays; everything finite"""
    i = inputs(name, regime)
    _check(_run(i), reference(name, regime), i, regime, f"{regime}/{name}", restated(name, regime))


def test_composite_one_ray_one_sample():
    i = inputs("one", "medium")
    _check(_run(i), reference("one", "medium"), i, "medium", "one")


def test_composite_batch_without_samples():
    """M == 0 with b > 0: acc is zero, weight and d_sigma are empty, nothing raises"""
    i = inputs("empty5", "medium")
    w, acc, ds = _run(i)
    assert w.shape == (0,) and ds.shape == (0,) and acc.shape == (5,) and (acc == 0.0).all()
    out = Composite.apply(_dev(i.sigma).requires_grad_(True), _dev(i.dist), _dev(i.offsets), i.b, i.scale)
    assert out.shape == (0,)


@pytest.mark.parametrize("regime", REGIMES)
def test_same_rays_under_both_kernel_families(regime):
    """the first 4 x len(ladder) + 3 rays of the large batch as a batch of their own (64 lanes per ray) and as the head of the large
    batch (8 / 16 lanes per ray): both inside the margin.  The float64 scans differ in association, which shows in the fp32 bits on
    rare ties only -- the share of differing samples is printed, not asserted."""
    big = inputs("narrow", regime)
    ref = reference("narrow", regime)
    n = BATCHES["partial"][0]
    M = int(big.offsets[n])
    head = type(big)(b=n, offsets=big.offsets[:n + 1], mask=big.mask[:n], sigma=big.sigma[:M], dist=big.dist[:M],
                     d_weight=big.d_weight[:M], scale=big.scale)
    head_ref = type(ref)(w=ref.w[:M], acc=ref.acc[:n], d_sigma=ref.d_sigma[:M], rowmax=ref.rowmax[:n], lit=ref.lit[:n])
    wide = _run(head)
    w, acc, ds = _run(big)
    narrow = (w[:M], acc[:n], ds[:M])
    _check(wide, head_ref, head, regime, f"{regime}/head, 64 lanes")
    _check(narrow, head_ref, head, regime, f"{regime}/head, 8 and 16 lanes")
    share = [float((a.view(np.uint32) != b.view(np.uint32)).mean()) for a, b in zip(wide, narrow)]
    print(f"{regime}: share of differing bits between the families: weight {share[0]:.2e}, acc {share[1]:.2e}, d_sigma {share[2]:.2e}")


def test_functional_composite_equals_the_wrappers_bit_for_bit():
    """Composite through autograd with a non-contiguous sigma and a non-contiguous adjoint == the direct wrapper calls"""
    i = inputs("partial", "wall")
    M = len(i.sigma)
    leaf = torch.zeros(M, 2, device=DEV)
    leaf[:, 0] = _dev(i.sigma)
    leaf.requires_grad_(True)
    dw2 = torch.zeros(M, 3, device=DEV)
    dw2[:, 1] = _dev(i.d_weight)
    sigma, dw = leaf[:, 0], dw2[:, 1]
    assert not sigma.is_contiguous() and not dw.is_contiguous()
    dist, off = _dev(i.dist), _dev(i.offsets)
    out = Composite.apply(sigma, dist, off, i.b, SCALE)
    (out * dw).sum().backward()
    w, _ = hip.composite_fwd(sigma.detach().contiguous(), dist, off, i.b, SCALE)
    ds = hip.composite_bwd(sigma.detach().contiguous(), dist, w, off, i.b, SCALE, dw.contiguous())
    assert torch.equal(out.detach(), w) and torch.equal(leaf.grad[:, 0], ds)
    assert float(leaf.grad[:, 1].abs().max()) == 0.0


# ---- segmented sums ------------------------------------------------------------------------------------------------------------------
def _values(name, D, stride=None):
    """vals [M, stride] float32 (columns beyond D hold a large number nobody may add), scale [M] float32, offsets"""
    off = inputs(name, "medium").offsets
    rng = np.random.default_rng([D, len(off)])
    vals = rng.standard_normal((int(off[-1]), stride or D)).astype(np.float32)
    vals[:, D:] = 1e30
    return vals, rng.uniform(0.0, 2.0, int(off[-1])).astype(np.float32), off


@pytest.mark.parametrize("name", ["partial", "narrow"])
def test_segment_sum_index_order_is_the_sequential_fp32_walk(name):
    """lanes=1 is bit exact: acc = fl(acc + fl(scale v)) in index order, D = 1..4, with and without scale"""
    for D in (1, 2, 3, 4):
        vals, scale, off = _values(name, D)
        for sc in (None, scale):
            got = hip.segment_sum(_dev(vals), None if sc is None else _dev(sc), _dev(off), len(off) - 1)
            assert torch.equal(got.cpu(), torch.from_numpy(sequential_sum32(vals, sc, off))), (D, sc is not None)
    vals, _, off = _values(name, 5)
    for lanes in (1, 8):
        with pytest.raises(hip.NmfHipError):
            hip.segment_sum(_dev(vals), None, _dev(off), len(off) - 1, lanes=lanes)


def _within_the_fp32_sum_bound(got, vals, scale, off, what):
    """|got - float64 sum| <= n 2^-24 sum |scale v| per element, n = segment length + 1: the bound of an fp32 sum of products in ANY
    order (one rounding per product, at most length - 1 roundings on the way of a term through the adds); empty segments exactly 0"""
    counts = np.diff(off)
    seg = torch.from_numpy(np.repeat(np.arange(len(counts)), counts))
    x = torch.from_numpy(vals.astype(np.float64) * (1.0 if scale is None else scale.astype(np.float64)[:, None]))
    want = torch.zeros(len(counts), x.shape[1], dtype=torch.float64).index_add_(0, seg, x)
    mag = torch.zeros_like(want).index_add_(0, seg, x.abs())
    bound = torch.from_numpy(counts + 1.0)[:, None] * 2.0 ** -24 * mag
    err = (got.cpu().double() - want).abs()
    assert got.shape == want.shape and bool((err <= bound).all()), (what, float((err - bound).max()))
    assert bool((got.cpu()[torch.from_numpy(counts == 0)] == 0.0).all()), what


def test_segment_sum_eight_lanes_within_the_fp32_sum_bound():
    for D in (1, 2, 3, 4):
        vals, scale, off = _values("partial", D)
        for sc in (None, scale):
            got = hip.segment_sum(_dev(vals), None if sc is None else _dev(sc), _dev(off), len(off) - 1, lanes=8)
            _within_the_fp32_sum_bound(got, vals, sc, off, f"segment_sum, 8 lanes, D = {D}")


@pytest.mark.parametrize("D", [1, 6, 7, 8, 9, 16, 17, 24, 32, 33, 64])
def test_segment_sum_wide_within_the_fp32_sum_bound(D):
    """every template (8, 16, 32, 64 lanes per row) at its first and last width, at row stride D and D + 3"""
    for stride in (D, D + 3):
        vals, _, off = _values("partial", D, stride)
        got = hip.segment_sum_wide(_dev(vals), D, _dev(off), len(off) - 1)
        _within_the_fp32_sum_bound(got, vals[:, :D], None, off, f"segment_sum_wide, D = {D}, stride {stride}")


def test_segment_sum_wide_refuses_widths_outside_1_to_64():
    off = inputs("partial", "medium").offsets
    vals = torch.ones(int(off[-1]), 70, device=DEV)
    for D in (0, 65):
        with pytest.raises(hip.NmfHipError):
            hip.segment_sum_wide(vals, D, _dev(off), len(off) - 1)


def test_expand_segments_is_repeat_interleave_and_the_local_arange():
    off = inputs("partial", "medium").offsets
    n_seg = len(off) - 1
    assert n_seg % 32 != 0 and set(np.diff(off).tolist()) == set(ladder())
    seg, loc = hip.expand_segments(_dev(off), n_seg, int(off[-1]))
    counts = torch.from_numpy(np.diff(off))
    want_seg = torch.repeat_interleave(torch.arange(n_seg), counts)
    want_loc = torch.arange(int(off[-1])) - torch.tensor(off)[want_seg]
    assert seg.dtype == loc.dtype == torch.int32
    assert torch.equal(seg.cpu().long(), want_seg) and torch.equal(loc.cpu().long(), want_loc)
