"""The environment map on the GPU: nmf_sat_build, nmf_sat_build_bwd, nmf_sat_lookup_fwd, nmf_sat_lookup_bwd (direct float atomics) and
nmf_sat_lookup_bwd_binned (csrc/env.hip) through the wrappers of nmf_amd/hip.py, against the float64 references of
tests/test_env_cpu.py, on its inputs, within its margins: values and d_dirs in table units per footprint class, d_sat per texel,
d_pole, the d_mip total of the whole batch and of one sub-batch per combo and mip clamp (8 x the error of the fp32 restatement, at
least 2^-23 of the metric's scale; d_dirs and d_mip against the restatement of the dual-number role in each path's own order).
EVERY element is compared: the inputs keep every gate 1e-3 away (see the CPU module, which also states which lookups reach which
combo).

The lookups run on the table that the CPU module builds in the kernels' rounding, not on the kernel's own build: the float64
references are then computed once, and the build is tested on its own below.
"""
import numpy as np
import pytest
import torch

from conftest import assert_close
from nmf_amd import hip
from test_env_cpu import (BUILD_MAPS, BUILD_METRICS, BWD_METRICS, D_DIRS, MAPS, MIPBIAS, SCALED, SHAPES, batch, build_bwd_case,
                          build_case, build_metrics, case, class_margins, dirs_margins, dual_case, mip_margin, sat_from_act, scaled,
                          split_clip, sub_batches, table)
from test_shading_rows_cpu import errors_over

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = np.float64
HS = [h for h, _ in MAPS]
PATHS = {"direct": 1 << 62, "binned": 1}


def _dev(a):
    return torch.tensor(a).to(DEV)                # (a copy: the shared inputs are read-only)


def _report(what, got, want, own, mg, metrics):
    """prints the largest error of every metric next to the restatement's, then holds every element to the margin"""
    err = errors_over(got, want, metrics)
    for m in err:
        ratio = f" = {err[m] / own[m]:.2f} x restatement" if own.get(m, 0) > 0 else ""
        print(f"{what} {m}: {err[m]:.3e}{ratio}, margin {mg[m]:.3e}")
    for m in err:
        assert_close(got[m], want[m], rtol=0.0, atol=mg[m], what=f"{what} {m}")


def _rows(b, ld):
    return _dev(b.dirs if ld == 3 else np.concatenate([b.origins, b.dirs], axis=1)).contiguous()


def _tables(m):
    return {"planar": _dev(m.sat), "interleaved": _dev(m.sat4)}


def _sc(mipbias=MIPBIAS, brightness=0.0, mul=1.0):
    return torch.tensor([mipbias, brightness, mul], dtype=torch.float32, device=DEV)


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
def _forward(m, b, what, ref_values, own, mg):
    """both tables, both pitches, the scalars by value and on the device: the same bits, every element inside its class margin,
    the pole rows the given pole entries exactly"""
    pole, sa = _dev(m.pole), _dev(b.sa)
    first = None
    for name, tab in _tables(m).items():
        for ld in (3, 6):
            rows = _rows(b, ld)
            vals = hip.sat_lookup_fwd(tab, rows, sa, MIPBIAS, pole)
            assert torch.equal(vals, hip.sat_lookup_fwd(tab, rows, sa, 77.0, pole, sc=_sc())), (what, name, ld)
            first = vals if first is None else first
            assert torch.equal(vals, first), (what, name, ld)
    got = first.cpu().numpy()
    assert got.shape == (b.R, 3) and np.isfinite(got).all()
    top, bot = b.g.pole & (b.g.cy < 0), b.g.pole & (b.g.cy > 0)
    assert np.array_equal(got[top], np.broadcast_to(m.pole[0], got[top].shape)), what
    assert np.array_equal(got[bot], np.broadcast_to(m.pole[1], got[bot].shape)), what
    keys = [k for k in SCALED if k.startswith("values")]
    _report(what, scaled(b, {"values": got}), scaled(b, {"values": ref_values}), own, mg, keys)


@pytest.mark.parametrize("H", HS)
def test_lookup_fwd_against_float64(H):
    """the full batch and its first 1, 31, 32, 33, 255, 256, 257 lookups"""
    m = table(H)
    ref, _, own, _ = case(H, "full")
    mg = class_margins(H)
    _forward(m, batch(H, "full"), f"H {H} full", ref["values"], own, mg)
    for n in SHAPES:
        _forward(m, batch(H, n), f"H {H} first {n}", ref["values"][:n], own, mg)


def test_lookup_fwd_dense_queue():
    """256 lookups of one workgroup with at least four extra boxes each: 1024 and more entries in the LDS queue"""
    ref, _, own, _ = case(16, "dense")
    _forward(table(16), batch(16, "dense"), "H 16 dense", ref["values"], own, class_margins(16))


@pytest.mark.parametrize("H", HS)
def test_lookup_axes(H, monkeypatch):
    """the six unit axes and (1, -1e-30, 0): +x is the table seam cx = -1, (1, -1e-30, 0) its other side cx = 1, +-z the poles.
    Values against float64; the adjoints only have to be finite"""
    m, b = table(H), batch(H, "axis")
    ref = case(H, "axis")[0]
    _forward(m, b, f"H {H} axes", ref["values"], case(H, "full")[2], class_margins(H))
    for path, thr in PATHS.items():
        monkeypatch.setattr(hip, "ENV_BINNED_MIN_LOOKUPS", thr)
        got = _backward(m, b, 3, "interleaved")
        assert all(np.isfinite(v).all() for v in got.values()), (H, path)


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
def _backward(m, b, ld, tab, idx=slice(None)):
    d_sat = torch.zeros(m.H, m.W, 4, device=DEV)
    d_pole, d_mip = torch.zeros(2, 3, device=DEV), torch.zeros(1, device=DEV)
    rows = _rows(b, ld)[idx].contiguous()
    d_dirs = hip.sat_lookup_bwd(_tables(m)[tab], rows, _dev(b.sa[idx]), MIPBIAS, _dev(b.d_out[idx]), d_sat, d_pole, d_mip)
    assert d_dirs.shape == rows.shape
    return {"d_dirs": d_dirs.cpu().numpy(), "d_sat4": d_sat.cpu().numpy(), "d_pole": d_pole.cpu().numpy(),
            "d_mip": float(d_mip.cpu()[0])}


def _check_backward(H, name, path, ld, tab):
    m, b = table(H), batch(H, name)
    ref, _, own, mg = case(H, name)
    _, own_d, mg_d = dual_case(H, name, path)                # d_dirs and d_mip: the dual-number restatement in this path's order
    own, mg = dict(own, **own_d), dict(mg, **mg_d)
    mg.update(dirs_margins(H, path))
    got = _backward(m, b, ld, tab)
    what = f"H {H} {name} {path} ld {ld} {tab}"
    assert all(np.isfinite(v).all() for v in got.values()), what
    if ld == 6:
        assert not got["d_dirs"][:, :3].any(), what                          # no dependence on the ray origin
    dd = got["d_dirs"][:, -3:]
    assert not dd[~b.d_out.any(axis=1)].any() and not dd[b.g.pole].any(), what          # zero adjoints and pole rows: exact zeros
    assert not got["d_sat4"][..., 3].any(), what
    _report(what, scaled(b, {"values": ref["values"], "d_dirs": dd}), scaled(b, ref), own, mg, D_DIRS)
    sums = {"d_sat": np.moveaxis(got["d_sat4"][..., :3], -1, 0), "d_pole": got["d_pole"]}
    _report(what, sums, ref, own, mg, ("d_sat", "d_pole"))
    err = abs(got["d_mip"] - ref["dm"].sum())
    print(f"{what} d_mip: {got['d_mip']:.6e} against {ref['dm'].sum():.6e}: {err:.3e} = {err / max(own['d_mip'], 1e-300):.2f} x restatement,"
          f" margin {mg['d_mip']:.3e}")
    assert err <= mg["d_mip"], what


@pytest.mark.parametrize("name", ["full", "range"])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("H", HS)
def test_lookup_bwd_against_float64(H, path, name, monkeypatch):
    """d_dirs per element, d_sat per texel, d_pole and the d_mip total, on the direct and on the binned path (H = 16: one partial tile
    with more than 4096 records, H = 48: 2 x 2 partial tiles), under the randn adjoints and under those scaled by 10^U(-6, 0)"""
    monkeypatch.setattr(hip, "ENV_BINNED_MIN_LOOKUPS", PATHS[path])
    _check_backward(H, name, path, 3, "planar")
    _check_backward(H, name, path, 6, "interleaved")


@pytest.mark.parametrize("path", list(PATHS))
def test_lookup_bwd_dense_queue(path, monkeypatch):
    monkeypatch.setattr(hip, "ENV_BINNED_MIN_LOOKUPS", PATHS[path])
    _check_backward(16, "dense", path, 3, "interleaved")


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("H", HS)
def test_mip_adjoint_per_class(H, path, monkeypatch):
    """the d_mip total of one sub-batch per combo, of the lookups clamped at mip 0, at mip 7 and at neither: an error confined to one
    class cannot average out against the others"""
    monkeypatch.setattr(hip, "ENV_BINNED_MIN_LOOKUPS", PATHS[path])
    m, b = table(H), batch(H, "full")
    ref = case(H, "full")[0]
    own = dual_case(H, "full", path)[0]
    for name, idx in sub_batches(H).items():
        got = _backward(m, b, 3, "interleaved", idx)["d_mip"]
        want, mg = ref["dm"][idx].sum(), mip_margin(own["dm"], ref["dm"], idx)
        e_own = abs(own["dm"].astype(F64)[idx].sum() - want)
        print(f"H {H} {path} {name} ({len(idx)} lookups) d_mip: {got:.6e} against {want:.6e}: {abs(got - want):.3e}"
              f" = {abs(got - want) / max(e_own, 1e-300):.2f} x restatement, margin {mg:.3e}")
        assert abs(got - want) <= mg, (H, path, name)


# ---- build ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["plain", "clip"])
@pytest.mark.parametrize("H", [h for h, _ in BUILD_MAPS])
def test_build_against_float64(H, which):
    """act against the float64 exp, sat bit for bit from the kernel's own act, the interleaved copy, the pole rows against the float64
    mean; brightness and mul by value and on the device give the same bits"""
    m = table(H)
    i, ref, own, mg = build_case(H, which)
    bg = _dev(i.bg)
    act, sat, pole, sat4 = hip.sat_build(bg, float(i.brightness), float(i.mul), pole=True, interleaved=True)
    other = hip.sat_build(bg, 7.0, -3.0, sc=_sc(0.0, float(i.brightness), float(i.mul)), pole=True, interleaved=True)
    assert all(torch.equal(a, b) for a, b in zip((act, sat, pole, sat4), other)), (H, which)
    got = {"act": act.cpu().numpy(), "pole": pole.cpu().numpy()}
    _report(f"H {H} build {which}", build_metrics(m, got), build_metrics(m, ref), own, mg, BUILD_METRICS)
    assert np.array_equal(sat.cpu().numpy(), sat_from_act(got["act"])), "prefix sums: float64 carried, rounded to fp32 per element"
    assert torch.equal(sat4[..., :3].permute(2, 0, 1), sat) and not bool(sat4[..., 3].any())
    pole_own = np.stack([got["act"][:, 0].astype(F64).mean(-1), got["act"][:, -1].astype(F64).mean(-1)])
    assert np.array_equal(got["pole"], pole_own.astype(np.float32)), "pole rows: the float64 mean of the kernel's own act"
    if which == "clip":
        flat = got["act"].reshape(-1)
        top = flat[m.at20[0]]                                # expf(20): the clip gives the texels above 20 the same bits
        assert (flat[m.at20] == top).all() and (flat[m.above] == top).all() and (flat[m.below] < top).all()


@pytest.mark.parametrize("which", ["plain", "clip"])
@pytest.mark.parametrize("H,table_of", [(h, "rand") for h, _ in BUILD_MAPS] + [(h, "lookups") for h in HS])
def test_build_bwd_against_float64(H, table_of, which):
    """d_bg of a random adjoint table and of the lookups' table, with d_pole, every texel inside its margin; above x == 20 exactly
    zero, at 20 and below not; brightness and mul by value and on the device give the same bits"""
    m = table(H)
    i, _, _, _ = build_case(H, which)
    d_sat4, d_pole, ref, own, mg = build_bwd_case(H, which, table_of)
    args = (_dev(i.bg), _dev(i.act), _dev(d_pole))
    d_bg = hip.sat_build_bwd(_dev(d_sat4), *args, float(i.brightness), float(i.mul))
    other = hip.sat_build_bwd(_dev(d_sat4), *args, 7.0, -3.0, sc=_sc(0.0, float(i.brightness), float(i.mul)))
    assert torch.equal(d_bg, other), (H, which, table_of)
    got = d_bg.cpu().numpy()
    assert np.isfinite(got).all()
    _report(f"H {H} build bwd {which} {table_of}", split_clip(m, got, "d_bg"), split_clip(m, ref, "d_bg"), own, mg, BWD_METRICS)
    if which == "clip":
        flat = got.reshape(-1)
        assert not flat[m.above].any() and flat[m.at20].all() and flat[m.below].all(), (H, table_of)
