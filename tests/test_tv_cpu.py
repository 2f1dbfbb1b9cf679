"""Total-variation regularisers without a GPU: the CPU path of utils.TVLoss / IntegralEquirect.tv_loss and a numpy restatement of
the kernel's arithmetic (nmf_amd/csrc/tv.hip: fp32 terms and gradient, fp64 sum) against the reference's float64 results in
tests/golden/tv.npz (tests/golden/make_tv_golden.py), the weight schedule of train.py:292-295,684-709, the config keys, the terms
the Trainer still refuses, and the argument validation of the entry points."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tv.npz")
f32 = np.float32


def load():
    return np.load(GOLDEN)


def case_input(z, name):
    """-> fp32 [1,C,H,W] input of a case (int8 storage: multiples of 1 / xscale)"""
    x = z[f"{name}_x"]
    if x.dtype == np.int8:
        return x.astype(np.float32) / f32(z[f"{name}_xscale"])
    return x


def case_grad(z, name, g):
    """the part of a [1,C,H,W] gradient the fixture stores for this case (every row, or the rows <name>_rows)"""
    g = np.asarray(g)
    return g[:, :, z[f"{name}_rows"], :] if f"{name}_rows" in z.files else g


def _sign(d):
    return np.sign(d).astype(np.float32)


def tv_numpy(x, kind, w=1.0, scale=1.0):
    """the kernel's arithmetic: -> (value as the kernel writes it (fp32), fp32 gradient scale * w * dTV/dx), x [1,C,H,W] fp32.
    Terms and gradient in fp32 in the kernel's order of operations, the value as the fp64 sum of the fp32 terms; the kernel differs
    at most in the order in which it adds the fp64 partial sums."""
    x = np.ascontiguousarray(x[0], dtype=np.float32)
    own, lo1, lo2 = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    if kind == "plane":
        a = x[:, :-1, :-1]
        dw, dh = x[:, :-1, 1:] - a, x[:, 1:, :-1] - a
        t = np.sqrt(dw * dw + dh * dh + f32(1e-5))
        gw, gh = dw / t, dh / t
        own[:, :-1, :-1] = f32(0) - gw - gh
        lo1[:, :-1, 1:] = gw                    # term (h, w-1) holds this element as x[h][w+1]
        lo2[:, 1:, :-1] = gh                    # term (h-1, w) holds it as x[h+1][w]
    elif kind == "line":
        d = x[:, 1:, :] - x[:, :-1, :]
        t = np.abs(d)
        own[:, :-1, :] = f32(0) - _sign(d)
        lo1[:, 1:, :] = _sign(d)
    else:
        a = x[:-1, :-1, :]
        da, db = x[1:, :-1, :] - a, x[:-1, 1:, :] - a
        t = np.abs(da) + np.abs(db) + f32(1e-8)
        own[:-1, :-1, :] = f32(0) - _sign(da) - _sign(db)
        lo1[1:, :-1, :] = _sign(da)             # term (c-1, h) holds this element as x[c+1][h]
        lo2[:-1, 1:, :] = _sign(db)             # term (c, h-1) holds it as x[c][h+1]
    assert t.dtype == np.float32 and own.dtype == np.float32
    n = f32(t.size)
    coef = f32(scale) * f32(w) / n
    grad = coef * (own + lo1 + lo2)
    value = f32(np.float64(f32(scale)) * (t.astype(np.float64).sum() * (np.float64(f32(w)) / np.float64(n))))
    return value, grad[None]


def fixture_margins(z=None):
    """What the GPU results may deviate by, derived on the CPU from the fixture alone: 4 x the largest deviation of the fp32
    restatement above from the reference's float64 results over every case -- `value`: relative to the value; `grad`: relative to the
    largest |gradient| of the case."""
    z = z or load()
    value, grad = 0.0, 0.0
    for name in z["names"]:
        name = str(name)
        v, g = tv_numpy(case_input(z, name), str(z[f"{name}_kind"]))
        ref_v, ref_g = float(z[f"{name}_value"]), z[f"{name}_grad"]
        value = max(value, abs(float(v) - ref_v) / abs(ref_v))
        grad = max(grad, float(np.abs(case_grad(z, name, g).astype(np.float64) - ref_g).max() / np.abs(ref_g).max()))
    return dict(value=4 * value, grad=4 * grad)


def field_table(z):
    """the 12 tensors of the fixture's field as (name, kind, factor): fields/tensoRF.py:342-360"""
    tab = []
    for tag in ("d", "a"):
        for i in range(3):
            tab += [(f"{tag}p{i}", "plane", 1e-2), (f"{tag}l{i}", "line", 1e-3)]
    return tab


def test_margins_are_fp32_sized():
    m = fixture_margins()
    print("margins", m)
    assert 0 < m["value"] < 1e-5 and 0 < m["grad"] < 1e-5


@pytest.mark.parametrize("name", [str(n) for n in np.load(GOLDEN)["names"]])
def test_cpu_path_and_restatement_match_the_reference(name):
    """utils.TVLoss / IntegralEquirect.tv_loss on CPU tensors (float64: the reference's numbers to rounding) and the fp32 restatement
    of the kernel (within the margins) on every fixture case"""
    from nmf_amd.modules.integral_equirect import IntegralEquirect
    from nmf_amd.utils import TVLoss
    z = load()
    x, kind = case_input(z, name), str(z[f"{name}_kind"])
    ref_v, ref_g = float(z[f"{name}_value"]), z[f"{name}_grad"]
    xd = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    if kind == "env":
        env = IntegralEquirect.__new__(IntegralEquirect)
        torch.nn.Module.__init__(env)
        env.bg_mat = torch.nn.Parameter(xd.detach().clone())
        v = env.tv_loss()
        (g,) = torch.autograd.grad(v, env.bg_mat)
    else:
        v = TVLoss()(xd)
        (g,) = torch.autograd.grad(v, xd)
    assert abs(float(v.detach()) - ref_v) <= 1e-14 * abs(ref_v)
    assert np.abs(case_grad(z, name, g.numpy()) - ref_g).max() <= 1e-14 * np.abs(ref_g).max()
    m = fixture_margins(z)
    rv, rg = tv_numpy(x, kind)
    dv = abs(float(rv) - ref_v) / abs(ref_v)
    dg = float(np.abs(case_grad(z, name, rg).astype(np.float64) - ref_g).max() / np.abs(ref_g).max())
    print(name, "restatement value dev", dv, "grad dev", dg, "margins", m)
    assert dv <= m["value"] and dg <= m["grad"]


def test_field_factors():
    """TV_loss_density / TV_loss_app with the CPU TVLoss and with the restatement: the 1e-2 / 1e-3 factors of fields/tensoRF.py"""
    from nmf_amd.utils import TVLoss
    z = load()
    reg = TVLoss()
    m = fixture_margins(z)
    rows = z["field_rows"]
    for tag, key in (("d", "field_density_value"), ("a", "field_app_value")):
        total, total32 = 0.0, 0.0
        for i in range(3):
            for kind, fac, k in (("plane", 1e-2, f"{tag}p{i}"), ("line", 1e-3, f"{tag}l{i}")):
                x = z[f"field_{k}"]
                xd = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
                v = reg(xd) * fac
                (g,) = torch.autograd.grad(v, xd)
                ref_g = z[f"field_g_{k}"]
                g = g.numpy()[:, :, rows, :] if kind == "plane" else g.numpy()
                assert np.abs(g - ref_g).max() <= 1e-14 * np.abs(ref_g).max()
                total += float(v)
                rv, rg = tv_numpy(x, kind, w=fac)
                rg = rg[:, :, rows, :] if kind == "plane" else rg
                assert np.abs(rg.astype(np.float64) - ref_g).max() <= (m["grad"] + 2.0 ** -23) * np.abs(ref_g).max()   # (+ the fp32 factor)
                total32 += float(rv)
        assert abs(total - float(z[key])) <= 1e-14 * abs(float(z[key]))
        assert abs(total32 - float(z[key])) <= (m["value"] + 2.0 ** -22) * abs(float(z[key]))


# ---- the weight schedule ---------------------------------------------------------------------------------------------------------
def reference_schedule(params, lr_decay_iters, lr_decay_target_ratio, steps, lbatch):
    """train.py:292-295 and :684-709 in plain Python.  steps: per optimizer step the list of its chunks, True = the chunk reaches the
    loss, False = it kept no sample and was skipped before (train.py:567-568) -> per step (sum of w_density / lbatch, of w_app / lbatch,
    of w_bg / lbatch over its chunks) and the weights after the last step."""
    if lr_decay_iters > 0:
        lr_factor = lr_decay_target_ratio ** (1 / lr_decay_iters)
    else:
        lr_factor = lr_decay_target_ratio ** (1 / params["n_iters"])
    TV_weight_density, TV_weight_app = params["TV_weight_density"], params["TV_weight_app"]
    out = []
    for chunks in steps:
        sd = sa = sb = 0.0
        for reaches in chunks:
            if not reaches:
                continue
            if TV_weight_density > 0:
                TV_weight_density *= lr_factor
                sd += TV_weight_density / lbatch
            if TV_weight_app > 0:
                TV_weight_app *= lr_factor
                sa += TV_weight_app / lbatch
            if params["TV_weight_bg"] > 0:
                sb += params["TV_weight_bg"] / lbatch
        out.append((sd, sa, sb))
    return out, (TV_weight_density, TV_weight_app)


@pytest.mark.parametrize("decay_iters", [-1, 250])
def test_weight_schedule(decay_iters):
    from nmf_amd.trainer import TVSchedule
    params = dict(TV_weight_density=0.1, TV_weight_app=0.01, TV_weight_bg=0.003, n_iters=1000)
    steps = [[True, True], [True, False, True], [False], [True]]
    want, final = reference_schedule(params, decay_iters, 0.1, steps, 4096)
    s = TVSchedule(params, lr_decay_iters=decay_iters, lr_decay_target_ratio=0.1)
    assert s.on
    for chunks, w in zip(steps, want):
        s.begin_step()
        for reaches in chunks:
            if reaches:
                s.chunk(4096)
        assert tuple(s.sums) == w
    assert (s.density, s.app) == final and s.bg == 0.003
    # two ranks: rank r's k-th chunk takes the weight of chunk 2 k + r -- the ranks' sums add up to one process over all chunks
    ranks = [TVSchedule(params, decay_iters, 0.1, world_size=2, rank=r) for r in range(2)]
    one = TVSchedule(params, decay_iters, 0.1)
    for s in ranks + [one]:
        s.begin_step()
    for k in range(2):
        for s in ranks:
            s.chunk(8192)
        one.chunk(8192); one.chunk(8192)
    for i in range(3):
        assert abs(ranks[0].sums[i] + ranks[1].sums[i] - one.sums[i]) <= 1e-15 * one.sums[i]
    assert ranks[0].density == ranks[1].density == one.density
    off = TVSchedule(dict(TV_weight_density=0.0, TV_weight_app=0.0, TV_weight_bg=0, n_iters=10))
    assert not off.on


def test_config_keys_parse_from_overrides():
    from nmf_amd.train import compose_run
    ns = argparse.Namespace(datadir=None, near_far=None, downsample=1.0, grid=None, bg=None, seed=None, views=None, test_views=None,
                            res=None, config_dir=None)
    cfg = compose_run(ns, ["model.params.TV_weight_density=0.1", "params.TV_weight_app=0.01", "params.TV_weight_bg=1e-2"])
    p = cfg["model"]["params"]
    assert (p["TV_weight_density"], p["TV_weight_app"], p["TV_weight_bg"]) == (0.1, 0.01, 0.01)
    assert "params" not in cfg
    assert cfg["lr_decay_iters"] == -1 and cfg["lr_decay_target_ratio"] == 0.1
    p0 = compose_run(ns, [])["model"]["params"]
    assert not p0["TV_weight_density"] and not p0["TV_weight_app"] and not p0["TV_weight_bg"]


def test_trainer_accepts_tv_weights_and_still_refuses_the_rest():
    from nmf_amd.config import resolved_config
    from nmf_amd.trainer import Trainer
    params = dict(resolved_config()["params"])
    Trainer.check_loss_terms(dict(params, TV_weight_density=0.1, TV_weight_app=0.01, TV_weight_bg=0.01))
    with pytest.raises(NotImplementedError) as e:
        Trainer.check_loss_terms(dict(params, TV_weight_density=0.1, distortion_lambda=1e-3))
    assert "distortion_lambda" in str(e.value) and "TV" not in str(e.value)
    for k in Trainer.NOT_ASSEMBLED:
        with pytest.raises(NotImplementedError):
            Trainer.check_loss_terms(dict(params, **{k: 1e-3}))


# ---- the entry points refuse bad arguments on the host ---------------------------------------------------------------------------
def test_entry_points_refuse_bad_tables_without_a_gpu():
    from nmf_amd import hip
    lib = hip._lib
    one = C.c_void_p(256)                   # (never dereferenced: the calls fail on their arguments)
    ptrs = (C.c_void_p * 1)(256)

    def call(shape, kind, xs=None, g=False, value=True, ws_bytes=1 << 20):
        sh, kd = (C.c_int32 * 3)(*shape), (C.c_int32 * 1)(kind)
        c, h, w = shape
        st = (C.c_int64 * 3)(*(xs or (h * w, w, 1)))
        wt = (C.c_float * 1)(1.0)
        return lib.nmf_tv_fwd_bwd(ptrs, ptrs if g else None, sh, st, st if g else None, kd, wt, 1, one, one if value else None,
                                  one if value else None, ws_bytes, None), int(lib.nmf_tv_workspace_bytes(sh, kd, 1))

    assert call((16, 1, 8), 0) == (-2, -2) and call((16, 8, 1), 0) == (-2, -2)       # a plane with H == 1 / W == 1: NMF_ERANGE
    assert call((16, 1, 1), 1) == (-2, -2)                                           # a line with G == 1
    assert call((3, 1, 8), 2) == (-2, -2)                                            # an env map with one row
    assert call((16, 8, 2), 1)[0] == -1 and call((4, 8, 8), 2)[0] == -1 and call((4, 8, 8), 7)[0] == -1
    assert call((4, 8, 8), 0, xs=(64, 8, 2))[0] == -1                                # strides that leave the tensor
    assert call((4, 8, 8), 0, value=False)[0] == -1                                  # neither value nor gradient
    assert call((4, 8, 8), 0, ws_bytes=16)[0] == -1                                  # workspace too small
    assert b"workspace" in lib.nmf_last_error_string()
    # 16 bytes of ticket + one fp64 partial sum per workgroup of 1024 elements
    assert call((16, 65, 64), 0, ws_bytes=0)[1] == 16 + 8 * -(-16 * 65 * 64 // 1024)
    sh, kd = (C.c_int32 * 51)(*([4, 8, 8] * 17)), (C.c_int32 * 17)()
    assert int(lib.nmf_tv_workspace_bytes(sh, kd, 17)) == -2 and int(lib.nmf_tv_workspace_bytes(sh, kd, 0)) == -1
    with pytest.raises(hip.NmfHipError):
        hip.tv_value([torch.zeros(1, 4, 8, 8)], ["plane"], [1.0], 1.0)               # a CPU tensor: refused, not computed on the host
