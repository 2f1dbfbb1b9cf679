"""The fused BRDF MLP on the GPU: nmf_brdf_mlp_fwd, nmf_brdf_mlp_pack and nmf_brdf_mlp_bwd_segments (nmf_amd/csrc/brdf_mlp.hip) through the
wrappers of nmf_amd/hip.py and through nmf_amd.functional.brdf_mlp, against the float64 references of tests/test_brdf_mlp_cpu.py, on
its inputs, within its margins (8 x the error of the fp32 restatement, at least 2^-23 of the metric's scale, never more than
tests/test_hip_parity.py allows the same quantity).  The ray counts and `max_workgroups` put up to 8 tiles on a wave below 1000
rays: the forward's second loop iteration (cur = nxt, the prefetch across build_x, hidden planes over the previous tile's input
planes), the backward's accumulators over 3, 4 and 8 tiles, ragged last tiles, a set change on a wave, gradient buffers that are
not zero.  EVERY element is compared and the forward's masks bit for bit: the CPU module keeps every pre-activation clear of zero.

Every test prints kernel error / restatement error per metric before it asserts.

The weight gradients of a launch on the six tensors and on the packed image are the same bits where an element takes ONE add (gW0,
gb0, gW2); gW4, gb2 and gb4 take two or more float atomics per element in the order they retire, which shows once the buffers do
not start at zero, and are held to the margins in both forms; from zeroed buffers all six are the same bits.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close
from nmf_amd import hip
from test_brdf_mlp_cpu import (CASES, FORMS, GRADS, MASK_R, MASK_WS, METRICS, N_GROUPS, OUT_BIAS, PAIRS, WEIGHTS, case, inputs, mask_case,
                               pair_case, pattern, reference64, weights)
from test_shading_rows_cpu import errors_over

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASE_IDS = [f"R{R}-wg{mw}" for R, mw in CASES]


def _dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)    # (a copy: the shared inputs are read-only)


def _report(what, got, c, metrics):
    """prints the largest error of every metric next to the restatement's, then holds every element to the margin"""
    err = errors_over(got, c.want, metrics)
    for m in metrics:
        ratio = f" = {err[m] / c.err[m]:.2f} x restatement" if c.err[m] > 0 else ""
        print(f"{what} {m}: {err[m]:.3e}{ratio}, margin {c.mg[m]:.3e}")
    for m in metrics:
        assert_close(got[m], c.want[m], rtol=0.0, atol=c.mg[m], what=f"{what} {m}")


@functools.lru_cache(maxsize=None)
def _weights(ws):
    w = [_dev(a) for a in weights(ws)]
    return w, hip.brdf_mlp_pack(w)


@functools.lru_cache(maxsize=None)
def _set(R, ws, form, salt=0):
    """(half_vec, diff_vec, feat_src, rough_src, src_idx) of a ray set on the device, and its d_out"""
    i = inputs(R, ws, salt)
    if form == "rows":
        return (_dev(i.hv), _dev(i.dv), _dev(i.feat), _dev(i.rough), _dev(i.src_idx)), _dev(i.d_out)
    return (_dev(i.hv), _dev(i.dv), _dev(i.feat_rays), _dev(i.rough_rays), None), _dev(i.d_out)


def _filled():
    return [_dev(a) for a in pattern()]


def _grads(grads, d_feat=None, **more):
    out = {k: g.cpu().numpy() for k, g in zip(GRADS, grads)}
    if d_feat is not None:
        out["d_feat"] = d_feat.cpu().numpy()
    out.update({k: v.cpu().numpy() for k, v in more.items()})
    return out


def _fourth_row_untouched(got):
    p = pattern()
    assert np.array_equal(got["gW4"][3], p[4][3]) and got["gb4"][3] == p[5][3]


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", WEIGHTS)
@pytest.mark.parametrize("R,mw", CASES, ids=CASE_IDS)
def test_forward_against_float64(R, mw, ws):
    """out within margin, both masks bit for bit; the packed image, the other grids and the other src_idx form give the same bits"""
    w, img = _weights(ws)
    ref = reference64(R, ws)
    first = None
    for form in FORMS:
        s, _ = _set(R, ws, form)
        out, mask = hip.brdf_mlp_fwd(w, *s, OUT_BIAS, max_workgroups=mw, with_mask=True)
        assert out.shape == (R, 3) and mask.shape == (R, 4) and mask.dtype == torch.int32
        bits = mask.cpu().numpy().view(np.uint32)
        assert np.array_equal(bits, ref.masks), (form, int((bits != ref.masks).any(1).sum()))
        _report(f"{ws} R {R} wg {mw} {form}", {"out": out.cpu().numpy()}, case(R, mw, ws, form), ("out",))
        out_i, mask_i = hip.brdf_mlp_fwd(None, *s, OUT_BIAS, max_workgroups=mw, with_mask=True, image=img)
        assert torch.equal(out_i, out) and torch.equal(mask_i, mask), form
        for other in (0, 1, 2):
            out_o, mask_o = hip.brdf_mlp_fwd(w, *s, OUT_BIAS, max_workgroups=other, with_mask=True)
            assert torch.equal(out_o, out) and torch.equal(mask_o, mask), (form, other)
        assert torch.equal(hip.brdf_mlp_fwd(w, *s, OUT_BIAS, max_workgroups=mw), out)
        first = (out, mask) if first is None else first
        assert torch.equal(out, first[0]) and torch.equal(mask, first[1])


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", WEIGHTS)
@pytest.mark.parametrize("R,mw", CASES, ids=CASE_IDS)
def test_backward_against_float64(R, mw, ws):
    """the forward's own output and masks in, gradient buffers that hold PATTERN: every metric within margin, the result is
    PATTERN + gradient, rows that no ray gathers and the fourth row of gW4 / gb4 untouched; tensors and image agree"""
    w, img = _weights(ws)
    i = inputs(R, ws)
    for form in FORMS:
        s, d_out = _set(R, ws, form)
        c = case(R, mw, ws, form)
        out, mask = hip.brdf_mlp_fwd(w, *s, OUT_BIAS, max_workgroups=mw, with_mask=True)
        grads = _filled()
        d_feat = hip.brdf_mlp_bwd(w, *s, out, mask, d_out, grads, max_workgroups=mw)
        got = _grads(grads, d_feat, out=out)
        assert d_feat.shape == ((i.M, 24) if form == "rows" else (R, 24))
        _report(f"{ws} R {R} wg {mw} {form}", got, c, METRICS)
        _fourth_row_untouched(got)
        if form == "rows":
            unused = np.setdiff1d(np.arange(i.M), i.gathered)
            assert len(unused) and not got["d_feat"][unused].any()
        grads_i = _filled()
        d_feat_i = hip.brdf_mlp_bwd(None, *s, out, mask, d_out, grads_i, max_workgroups=mw, image=img)
        got_i = _grads(grads_i, d_feat_i)
        for k in METRICS[1:]:
            # one add per element and a fixed summation order: the same bits; gW4, gb2, gb4 and d_feat take several float atomics per
            # element, in whatever order they retire, on top of what the buffer held
            if k in ("gW0", "gb0", "gW2"):
                assert np.array_equal(got_i[k], got[k]), k
            assert_close(got_i[k], c.want[k], rtol=0.0, atol=c.mg[k], what=f"{k} (packed weights)")
        # from zeroed buffers, as tests/test_hip_parity.py launches them, all six are the same bits in both forms
        za, zb = [torch.zeros_like(g) for g in grads], [torch.zeros_like(g) for g in grads]
        hip.brdf_mlp_bwd(w, *s, out, mask, d_out, za, max_workgroups=mw)
        hip.brdf_mlp_bwd(None, *s, out, mask, d_out, zb, max_workgroups=mw, image=img)
        for k, x, y in zip(GRADS, za, zb):
            assert torch.equal(x, y), k


@pytest.mark.parametrize("name", ("ones", "zeros", "alternating") + tuple(range(N_GROUPS)))
def test_backward_with_given_masks(name):
    """R = 421 on one workgroup, masks that are not the forward's, against the reference that takes them as given: a wrong unit-to-bit
    map of the backward shows here and not in the forward.  All zeros: gW4 / gb4 are still gradients, everything upstream is exact"""
    w, _ = _weights(MASK_WS)
    s, d_out = _set(MASK_R, MASK_WS, "rows")
    c = mask_case(name)
    out = hip.brdf_mlp_fwd(w, *s, OUT_BIAS, max_workgroups=1)
    grads = _filled()
    d_feat = hip.brdf_mlp_bwd(w, *s, out, _dev(c.masks.view(np.int32)), d_out, grads, max_workgroups=1)
    got = _grads(grads, d_feat, out=out)
    _report(f"masks {name}", got, c, METRICS)
    _fourth_row_untouched(got)
    if name == "zeros":
        for k, p in zip(GRADS[:4], pattern()):
            assert np.array_equal(got[k], p), k
        assert not got["d_feat"].any()
        assert not np.array_equal(got["gW4"][:3], pattern()[4][:3]) and not np.array_equal(got["gb4"][:3], pattern()[5][:3])
    if isinstance(name, int):
        only = c.want["gW2"] != pattern()[2].astype(np.float64)
        assert only.sum() == 1 and np.array_equal(got["gW2"][~only], pattern()[2][~only])


@pytest.mark.parametrize("ws", WEIGHTS)
@pytest.mark.parametrize("R0,R1", PAIRS)
def test_two_ray_sets_in_one_launch(R0, R1, ws):
    """different feature tables, set 0 with src_idx and set 1 without, different d_out, one workgroup: a ragged last tile of set 0 is
    followed by set 1 on the same wave.  Each d_feat against its own reference, the weight gradients against the float64 sum"""
    w, img = _weights(ws)
    c = pair_case(R0, R1, ws)
    sets = []
    for R, form, salt in ((R0, "rows", 0), (R1, "rays", 1)):
        s, d_out = _set(R, ws, form, salt)
        out, mask = hip.brdf_mlp_fwd(w, *s, OUT_BIAS, max_workgroups=1, with_mask=True)
        assert np.array_equal(mask.cpu().numpy().view(np.uint32), reference64(R, ws, salt).masks)
        sets.append(s + (out, mask, d_out))
    for use_img in (False, True):
        grads = _filled()
        d0, d1 = hip.brdf_mlp_bwd_segments(None if use_img else w, sets, grads, max_workgroups=1, image=img if use_img else None)
        got = _grads(grads, d_feat0=d0, d_feat1=d1)
        _report(f"{ws} sets {R0} + {R1}{' image' if use_img else ''}", got, c, c.metrics)
        _fourth_row_untouched(got)


@pytest.mark.parametrize("ws", WEIGHTS)
def test_through_autograd(ws):
    """nmf_amd.functional.brdf_mlp at R = 997 (default grids: one tile per wave forward, two backward): the path the trainer takes"""
    from nmf_amd.functional import brdf_mlp
    R = 997
    i, c = inputs(R, ws), case(R, 0, ws, "rows", False)
    (hv, dv, feat, rough, src), d_out = _set(R, ws, "rows")
    w = [a.clone().requires_grad_(True) for a in _weights(ws)[0]]
    feat = feat.clone().requires_grad_(True)
    off = _dev(np.concatenate([[0], np.cumsum(np.bincount(i.src_idx, minlength=i.M))]).astype(np.int64))
    out = brdf_mlp(hv, dv, feat, rough, src, off, OUT_BIAS, w)
    g = torch.autograd.grad((out * d_out).sum(), [feat] + w)
    _report(f"{ws} autograd R {R}", _grads(g[1:], g[0], out=out.detach()), c, METRICS)
