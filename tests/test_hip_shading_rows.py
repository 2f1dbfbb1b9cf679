"""The per-ray and per-row glue of the shading step on the GPU: nmf_ray_compose_fwd / _bwd, nmf_bg_adjoint, nmf_bounce_prep_fwd / _bwd
(csrc/shade.hip), nmf_bounce_prep_heads_bwd, nmf_heads_fwd / _bwd (csrc/heads.hip, csrc/rows_bwd.hpp) through the wrappers the
training step calls, against the float64 references of tests/test_shading_rows_cpu.py, on its inputs, within its margins (8 x the
error of the fp32 restatement, at least 2^-23 of the metric's scale).  EVERY element is compared: the inputs keep every gate 1e-3
away or exactly on its threshold (see the CPU module, which also maps the tests to the code paths they enter).

The wrappers are called directly: the autograd Functions make the adjoints contiguous, and the step does not.
"""
import numpy as np
import pytest
import torch

from conftest import assert_close
from nmf_amd import hip
from test_shading_rows_cpu import (FLAGS, HEAD_METRICS, HEAD_ROWS, HP, MIN_ROUGH, ANOISE, RAY_BATCHES, ROW_COUNTS, ROW_METRICS, errors_over,
                                   flag_id, head_of, heads_case, heads_inputs, heads_reference64, heads_restatement32, margins,
                                   one_hot_weight, ray_case, ray_inputs, rgb_map_of, RAY_METRICS, row_inputs_of, rows_case,
                                   rows_restatement32, strided_adjoints)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = np.float64


def _dev(a):
    return torch.tensor(a).to(DEV)                # (a copy: the shared inputs are read-only)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _report(what, got, want, own, mg, metrics):
    """prints the largest error of every metric next to the restatement's, then holds every element to the margin"""
    err = errors_over(got, want, metrics)
    for m in err:
        ratio = f" = {err[m] / own[m]:.2f} x restatement" if own.get(m, 0) > 0 else ""
        print(f"{what} {m}: {err[m]:.3e}{ratio}, margin {mg[m]:.3e}")
    for m in err:
        assert_close(got[m], want[m], rtol=0.0, atol=mg[m], what=f"{what} {m}")


# ---- ray compose ----------------------------------------------------------------------------------------------------------------------
def _run_rays(i, flags, weight=None):
    """forward, backward (on the kernel's own rgb_lin, as the step does) and background adjoint -> dict of numpy arrays / None"""
    tonemap, noclip, per_ray, want_ori, with_refl = flags
    w = _dev(i.weight if weight is None else weight)
    refl, inv = (_dev(i.refl), _dev(i.inv)) if with_refl else (None, None)
    normals = _dev(i.normals) if want_ori else None
    rays, bg, d_rgb = _dev(i.rays), _dev(i.bg_ray if per_ray else i.bg_one), _dev(i.d_rgb)
    rgb_map, acc, lin, ori = hip.ray_compose_fwd(w, refl, inv, normals, rays, _dev(i.offsets), i.b, bg, per_ray, tonemap, noclip, want_ori)
    d_w, d_refl, d_n = hip.ray_compose_bwd(w, refl, inv, normals, rays, _dev(i.ray_id), bg, per_ray, tonemap, noclip, lin, d_rgb,
                                           _dev(i.d_acc), _dev(i.d_ori) if want_ori else None, want_ori)
    assert (ori is None) == (not want_ori) and (d_n is None) == (not want_ori) and (d_refl is None) == (not with_refl)
    return {"rgb_lin": _np(lin), "acc": _np(acc), "ori": _np(ori), "rgb_map": _np(rgb_map), "d_weight": _np(d_w), "d_refl": _np(d_refl),
            "d_normals": _np(d_n), "bg_adjoint": _np(hip.bg_adjoint(acc, d_rgb))}


def _report_rays(what, got, ref, i, flags, own, mg):
    """rgb_map is held to the float64 tonemap and blend of the kernel's OWN sums, everything else to the float64 reference"""
    want = dict(ref, rgb_map=rgb_map_of(i, flags, got["rgb_lin"], got["acc"]))
    _report(what, got, want, own, mg, [m for m in RAY_METRICS if ref[m] is not None])


def _check_rays(i, flags, what):
    ref, own, mg = ray_case(i, flags)
    got = _run_rays(i, flags)
    assert all(np.isfinite(v).all() for v in got.values() if v is not None), what
    empty = np.diff(i.offsets) == 0
    assert (got["acc"][empty] == 0).all() and (got["rgb_lin"][empty] == 0).all(), what
    if not flags[4]:
        assert not got["rgb_lin"].any(), what               # no bounce rows: the colour sums are exactly zero
    _report_rays(what, got, ref, i, flags, own, mg)
    return got


@pytest.mark.parametrize("flags", FLAGS, ids=flag_id)
@pytest.mark.parametrize("name", list(RAY_BATCHES))
def test_ray_compose_against_float64(name, flags):
    """every batch under every combination of tonemap (T), noclip (N), per-ray background (B), orientation term (O) and bounce rows
    (R): rgb_lin, acc, ori, rgb_map (against the float64 tonemap of the kernel's own sums), d_weight, d_refl, d_normals and the
    background adjoint, every element inside the margin"""
    _check_rays(ray_inputs(name), flags, f"{name}/{flag_id(flags)}")


@pytest.mark.parametrize("name", ["one", "knee", "knee_up", "empty5"])
def test_ray_compose_small_batches(name):
    """one ray with one sample -- also with rgb_lin exactly on the sRGB knee and one float above it -- and five rays without a sample"""
    i = ray_inputs(name)
    for flags in FLAGS:
        got = _check_rays(i, flags, f"{name}/{flag_id(flags)}")
        if name == "empty5":
            assert got["d_weight"].shape == (0,) and got["acc"].shape == (5,) and got["rgb_map"].shape == (5, 3)
            assert np.array_equal(got["rgb_map"], np.broadcast_to(i.bg_ray if flags[2] else i.bg_one, (5, 3)))
    if name == "knee":                                      # x > limit is false on the limit: the linear branch, exactly
        got = _run_rays(i, (True, False, True, False, True))
        assert np.all(got["rgb_map"][0] == np.float32(12.92) * i.refl[0, 0])


def test_ray_compose_without_bounce_rows():
    """refl_rows / inv absent in the form the levels >= 1 call (no normals, no tonemap, per-ray background): rgb_lin == 0 exactly,
    rgb_map == (1 - acc) bg in its two roundings, d_refl is None"""
    for name in RAY_BATCHES:
        i = ray_inputs(name)
        got = _run_rays(i, (False, False, True, False, False))
        assert got["d_refl"] is None and not got["rgb_lin"].any()
        assert np.array_equal(got["rgb_map"], (np.float32(1) - got["acc"])[:, None] * i.bg_ray)


@pytest.mark.parametrize("name,indices", [("partial", (0, 63, 64, 127, 128, -1)), ("narrow", (7, 8, 15, 16, -1))])
def test_ray_compose_one_hot_weights(name, indices):
    """all weights zero but one sample per ray, at the indices around the lanes' first, second and third sample (-1: the ray's
    last): acc is that weight, a colour sum the single product w c -- the float64 product rounded to fp32, within one ulp -- and the
    orientation term w ndv^2 within the error bound of its three-term dot product.  A sample that is dropped, read twice or given
    to another ray cannot hide behind a sum here."""
    i = ray_inputs(name)
    flags = (False, False, True, True, True)
    d = i.rays[i.ray_id, 3:6].astype(F64)
    terms = d * i.normals.astype(F64)
    for index in indices:
        w, rows, at = one_hot_weight(i, index)
        assert len(rows) > 0
        got = _run_rays(i, flags, weight=w)
        others = np.ones(i.b, dtype=bool)
        others[rows] = False
        assert np.array_equal(got["acc"][rows], w[at]) and not got["acc"][others].any(), (name, index)
        assert not got["rgb_lin"][others].any() and not got["ori"][others].any(), (name, index)
        has = i.inv[at] >= 0
        want = np.where(has[:, None], w[at].astype(F64)[:, None] * i.refl[np.maximum(i.inv[at], 0)].astype(F64), 0.0).astype(np.float32)
        off = np.abs(got["rgb_lin"][rows].astype(F64) - want.astype(F64))
        assert (off <= np.spacing(np.abs(want)).astype(F64)).all(), (name, index, float(off.max()))
        assert not got["rgb_lin"][rows][~has].any(), (name, index)
        ndv = np.minimum(-terms[at].sum(1), 0.0)
        delta = 4 * 2.0 ** -24 * np.abs(terms[at]).sum(1)             # the fp32 dot product of three terms (and its negation)
        bound = w[at].astype(F64) * (2 * np.abs(ndv) * delta + delta ** 2) + 4 * 2.0 ** -24 * w[at].astype(F64) * ndv ** 2 + 1e-45
        off = np.abs(got["ori"][rows].astype(F64) - w[at].astype(F64) * ndv ** 2)
        assert (off <= bound).all(), (name, index, float((off - bound).max()))
        print(f"{name} one-hot at {index}: {len(rows)} rays")


def test_same_rays_under_both_lane_widths():
    """the first 16384 rays of `narrow` as a batch of their own (64 lanes per ray) and as the head of the whole batch (8 lanes per
    ray): each inside its own margin against float64.  Bit equality is not claimed: the two walks add in different orders."""
    big = ray_inputs("narrow")
    n = RAY_BATCHES["last64"]
    head = head_of(big, n)
    flags = (True, False, True, True, True)
    ref, own, mg = ray_case(head, flags)
    wide = _run_rays(head, flags)
    _report_rays("head of narrow, 64 lanes", wide, ref, head, flags, own, mg)
    _, own8, mg8 = ray_case(big, flags)
    M, Mb = len(head.weight), len(head.refl)
    cut = {"d_weight": M, "d_normals": M, "d_refl": Mb}
    got = {k: (v if v is None else v[:cut.get(k, n)]) for k, v in _run_rays(big, flags).items()}
    _report_rays("head of narrow, 8 lanes", got, ref, head, flags, own8, mg8)
    differ = {k: float((wide[k].view(np.uint32) != got[k].view(np.uint32)).mean()) for k in ("acc", "rgb_lin", "ori")}
    print("share of sums whose bits differ between the lane widths:", differ)


# ---- bounce rows ----------------------------------------------------------------------------------------------------------------------
def _row_tensors(i, row_inputs):
    """normals / app / heads / noise per sample or per bounce row, as row_inputs 0, 1, 2 want them"""
    per_row = lambda a, on: _dev(a[i.bidx] if on else a)      # noqa: E731
    return per_row(i.normals, row_inputs == 2), per_row(i.app, row_inputs >= 1), per_row(i.heads, row_inputs >= 1), per_row(i.noise, row_inputs >= 1)


def _common(i):
    return _dev(i.bidx), _dev(i.inv), _dev(i.ray_id), _dev(i.rays), _dev(i.conv)


def _prep_bwd(i, row_inputs, detach_n, adj):
    normals, _, heads, _ = _row_tensors(i, row_inputs)
    bidx, inv, ray_id, rays, conv = _common(i)
    dN, dr1, df0, ddiff = adj
    return hip.bounce_prep_bwd(inv, normals, heads, ray_id, rays, conv, MIN_ROUGH, detach_n, dN, dr1, df0, ddiff, _dev(i.dfeat),
                               bidx=bidx, row_inputs=row_inputs)


def _dense_adjoints(i):
    return _dev(i.dN), _dev(i.dr1), _dev(i.df0), _dev(i.ddiff)


def _sliced_adjoints(i, view):
    rows, rows6 = (_dev(a) for a in strided_adjoints(i, view))
    adj = rows[:, 0:3], rows[:, 3], rows6[:, 0:3], rows6[:, 3:6]
    assert i.Mb == 1 or not any(a.is_contiguous() for a in adj)
    return adj


def _scatter(i, per_sample, row_inputs, key):
    """the float64 per-sample gradient in the layout the kernel returns it under row_inputs"""
    per_row = row_inputs == 2 if key == "d_normals" else row_inputs >= 1
    return per_sample[i.bidx] if per_row else per_sample


@pytest.mark.parametrize("row_inputs", [0, 1, 2])
@pytest.mark.parametrize("Mb", ROW_COUNTS)
def test_bounce_prep_fwd_against_float64(Mb, row_inputs):
    i = row_inputs_of(Mb)
    ref, own, mg = rows_case(Mb, False)
    normals, app, heads, noise = _row_tensors(i, row_inputs)
    bidx, _, ray_id, rays, conv = _common(i)
    outs = hip.bounce_prep_fwd(bidx, normals, app, heads, _dev(i.xyzt), ray_id, rays, conv, noise, ANOISE, MIN_ROUGH, row_inputs)
    got = dict(zip(("V", "N", "r1", "f0", "diffuse", "feat", "xyz"), (_np(o) for o in outs)))
    fwd = ROW_METRICS[:5]
    _report(f"bounce prep fwd {Mb} rows, row_inputs {row_inputs}", got, ref, own, mg, fwd)
    assert np.array_equal(got["V"], ref["V"].astype(np.float32)) and np.array_equal(got["xyz"], ref["xyz"].astype(np.float32))
    if Mb >= 2:
        assert not got["N"][0].any() and got["r1"][1] == MIN_ROUGH           # the zero normal, h9 == min_rough


@pytest.mark.parametrize("row_inputs", [0, 1, 2])
@pytest.mark.parametrize("Mb", ROW_COUNTS)
def test_bounce_prep_bwd_dense_and_strided(Mb, row_inputs):
    """nmf_bounce_prep_bwd with the row adjoints dense, and as the column slices of [Mb, 7], [Mb, 4] and [Mb, 6] buffers that the step
    passes (the columns in between hold 1e30): the dense call inside the float64 margin, the strided calls its bits.  With dN absent
    or detach_n the normal adjoint is exactly zero and nothing else changes."""
    i = row_inputs_of(Mb)
    ref, own, mg = rows_case(Mb, False)
    dense = _prep_bwd(i, row_inputs, False, _dense_adjoints(i))
    keys = ("d_normals", "d_heads", "d_app")
    got = dict(zip(keys, (_np(t) for t in dense)))
    want = {k: _scatter(i, ref[k], row_inputs, k) for k in keys}
    _report(f"bounce prep bwd {Mb} rows, row_inputs {row_inputs}", got, want, own, mg, keys)
    for k in keys:                                          # samples without a bounce row: exact zeros
        if got[k].shape[0] == i.M:
            assert not got[k][i.inv < 0].any(), k
    for view in (False, True):
        strided = _prep_bwd(i, row_inputs, False, _sliced_adjoints(i, view))
        assert all(torch.equal(a, b) for a, b in zip(strided, dense)), (Mb, row_inputs, view)
    adj = _sliced_adjoints(i, True)
    for detach_n, a in ((True, adj), (False, (None,) + adj[1:])):
        off = _prep_bwd(i, row_inputs, detach_n, a)
        assert not bool(off[0].any()) and torch.equal(off[1], dense[1]) and torch.equal(off[2], dense[2]), (Mb, row_inputs, detach_n)


def _fused(i, h, adj, detach_n=False):
    bidx, _, ray_id, rays, conv = _common(i)
    gW, gb = torch.zeros(11, 24, device=DEV), torch.zeros(11, device=DEV)
    d_normals, d_app = hip.HOST_EXT.bounce_prep_heads_bwd(bidx, _dev(i.normals[i.bidx]), _dev(i.heads[i.bidx]), ray_id, rays, conv, MIN_ROUGH,
                                                          detach_n, adj[0], adj[1], adj[2], adj[3], _dev(i.dfeat), _dev(h.feat), _dev(h.W),
                                                          _dev(h.b), list(HP), gW, gb, hip._stream())
    return d_normals, d_app, gW, gb


@pytest.mark.parametrize("Mb", ROW_COUNTS)
def test_fused_prep_heads_bwd_dense_and_strided(Mb):
    """nmf_bounce_prep_heads_bwd (the row adjoint computed inside the heads' backward, nmf_rows::prep_bwd_row) against the float64
    composition of the two references: d_normals, d_app = dfeat + the heads' feature adjoint, gW, gb.  The strided call gives the
    bits of the dense one where no atomic is involved (d_normals, d_app) and holds the margin in gW / gb."""
    i, h = row_inputs_of(Mb), heads_inputs(Mb)
    rref, rown, rmg = rows_case(Mb, False)
    d_heads64 = rref["d_heads"][i.bidx]
    ref = heads_reference64(h.feat, h.W, h.b, d_heads64, add=i.dfeat)
    own = errors_over(heads_restatement32(h.feat, h.W, h.b, rows_restatement32(i, False)["d_heads"], add=i.dfeat), ref, HEAD_METRICS[1:])
    mg = margins(own, ref, HEAD_METRICS[1:])
    ref["d_normals"], own["d_normals"], mg["d_normals"] = rref["d_normals"][i.bidx], rown["d_normals"], rmg["d_normals"]
    keys = ("d_normals", "d_feat", "gW", "gb")
    dense = _fused(i, h, _dense_adjoints(i))
    _report(f"fused prep + heads bwd {Mb} rows, dense", dict(zip(keys, map(_np, dense))), ref, own, mg, keys)
    for view in (False, True):
        strided = _fused(i, h, _sliced_adjoints(i, view))
        assert torch.equal(strided[0], dense[0]) and torch.equal(strided[1], dense[1]), (Mb, view)
        _report(f"fused prep + heads bwd {Mb} rows, pitch {7 if view else 4}", dict(zip(keys, map(_np, strided))), ref, own, mg, keys)
    adj = _sliced_adjoints(i, True)
    for detach_n, a in ((True, adj), (False, (None,) + adj[1:])):
        off = _fused(i, h, a, detach_n)
        assert not bool(off[0].any()) and torch.equal(off[1], dense[1]), (Mb, detach_n)


# ---- material heads -------------------------------------------------------------------------------------------------------------------
def _heads_bwd(i, d_out, add=None):
    gW, gb = torch.zeros(11, 24, device=DEV), torch.zeros(11, device=DEV)
    d_feat = hip.heads_bwd(_dev(i.feat), _dev(i.W), _dev(i.b), HP, d_out, gW, gb, add_into=add)
    return d_feat, gW, gb


@pytest.mark.parametrize("M", HEAD_ROWS)
def test_heads_against_float64(M):
    """forward and backward at one row, around one 256-row block and at 1024 x 256 + 257 rows (a second pass of the capped grid with a
    partial last block): out, d_feat with and without add_into, gW, gb"""
    i = heads_inputs(M)
    out = hip.heads_fwd(_dev(i.feat), _dev(i.W), _dev(i.b), HP)
    for with_add in (False, True):
        ref, own, mg = heads_case(M, with_add)
        add = _dev(i.add) if with_add else None
        d_feat, gW, gb = _heads_bwd(i, _dev(i.d_out), add)
        assert not with_add or d_feat.data_ptr() == add.data_ptr()          # added in place, and returned
        got = {"out": _np(out), "d_feat": _np(d_feat), "gW": _np(gW), "gb": _np(gb)}
        assert all(np.isfinite(v).all() for v in got.values())
        _report(f"heads {M} rows, add_into {with_add}", got, ref, own, mg, HEAD_METRICS)


@pytest.mark.parametrize("M,rows", [(257, (0, 255, 256)), (HEAD_ROWS[-1], (0, 255, 256, 262143, 262144, HEAD_ROWS[-1] - 1))])
def test_heads_one_hot_rows(M, rows):
    """d_out zero except in one row -- the first and last of a block, of the first pass of the grid, of the second: gb is then that
    row's da (inside the margin of a row alone against float64) and gW its outer product with the row's features, da f, within
    2 ulp per entry of the float64 product of the kernel's own da.  Every other row's d_feat is exactly zero."""
    i = heads_inputs(M)
    for row in rows:
        d_out = np.zeros_like(i.d_out)
        d_out[row] = i.d_out[row]
        d_feat, gW, gb = (_np(t) for t in _heads_bwd(i, _dev(d_out)))
        one = slice(row, row + 1)
        ref = heads_reference64(i.feat[one], i.W, i.b, i.d_out[one])
        own = errors_over(heads_restatement32(i.feat[one], i.W, i.b, i.d_out[one]), ref, ("d_feat", "gb"))
        mg = margins(own, ref, ("d_feat", "gb"))
        _report(f"heads {M} rows, one-hot row {row}", {"d_feat": d_feat[one], "gb": gb}, ref, own, mg, ("d_feat", "gb"))
        want = gb.astype(F64)[:, None] * i.feat[row].astype(F64)[None, :]
        off = np.abs(gW.astype(F64) - want)
        assert (off <= 2 * np.spacing(np.abs(want).astype(np.float32)).astype(F64) + 2.0 ** -126).all(), (M, row, float(off.max()))
        assert np.abs(gb).max() > 0
        d_feat[row] = 0
        assert not d_feat.any(), (M, row)


def test_heads_saturated_and_clipped_rows():
    """rows whose diffuse pre-activation is +-150 (expf overflows: the sigmoid is exactly 0 or 1) give finite outputs and an exactly
    zero adjoint; rows whose roughness is clipped at 0.01 give an exactly zero da for that output, the others do not"""
    M = 257
    i = heads_inputs(M)
    out = _np(hip.heads_fwd(_dev(i.feat), _dev(i.W), _dev(i.b), HP))
    assert np.isfinite(out).all() and out[2, 0] == 1.0 and out[3, 0] == 0.0
    ref, _, _ = heads_case(M, False)
    for j in (0, 9, 10):
        d_out = np.zeros_like(i.d_out)
        d_out[:, j] = 1.0
        d_feat, gW, gb = (_np(t) for t in _heads_bwd(i, _dev(d_out)))
        assert np.isfinite(d_feat).all() and np.isfinite(gW).all() and np.isfinite(gb).all()
        zero = ~d_feat.any(axis=1)
        if j == 0:
            assert zero[2] and zero[3]
        else:
            clipped = ref["out"][:, j] <= 0.01                # float64, and at least 1e-3 clear of the gate on either side
            assert 0.05 * M < clipped.sum() < 0.95 * M and np.array_equal(zero[4:], clipped[4:]), j      # (rows 2, 3: saturated)
