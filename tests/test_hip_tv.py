"""Total-variation regularisers on the GPU: nmf_tv_fwd_bwd through hip.tv_value_grad against the reference's float64 results
(tests/golden/tv.npz) within the margins tests/test_tv_cpu.py derives on the CPU, its modes and determinism, the autograd route
(utils.TVLoss, IntegralEquirect.tv_loss, TensorVMSplit.TV_loss_*), and the Trainer: gradients, value, weight schedule, launch
counts, two data-parallel ranks."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_tv_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = [str(n) for n in np.load(cpu.GOLDEN)["names"]]
_CACHE = {}


def fixture():
    if "z" not in _CACHE:
        z = cpu.load()
        _CACHE["z"], _CACHE["m"] = z, cpu.fixture_margins(z)
        print("margins", _CACHE["m"])
    return _CACHE["z"], _CACHE["m"]


def _dev(x, channels_last=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases(name):
    """value and gradient of every case within the CPU-derived margins, in both storage orders; the gradient is ADDED to a non-zero
    g; the value-only and gradient-only modes give the combined mode's bits"""
    from nmf_amd import hip
    z, m = fixture()
    x, kind = cpu.case_input(z, name), str(z[f"{name}_kind"])
    ref_v, ref_g = float(z[f"{name}_value"]), z[f"{name}_grad"]
    for cl in (False, True):
        xt = _dev(x, cl)
        v, (g,) = hip.tv_value_grad([xt], [kind], [1.0], 1.0)
        dv = abs(float(v) - ref_v) / abs(ref_v)
        dg = float(np.abs(cpu.case_grad(z, name, g.cpu().numpy()).astype(np.float64) - ref_g).max() / np.abs(ref_g).max())
        print(name, "channels_last" if cl else "contiguous", "value dev", dv, "grad dev", dg, "margins", m)
        assert dv <= m["value"] and dg <= m["grad"]
        # added to a non-zero g, with a weight and a device-side scale; g in the OTHER storage order than x
        g0 = torch.randn(x.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
        g0 = g0 if cl else g0.contiguous(memory_format=torch.channels_last)
        g1 = g0.clone(memory_format=torch.preserve_format)
        scale = torch.full((), 0.5, device=DEV)
        v2, _ = hip.tv_value_grad([xt], [kind], [3.0], scale, grads=[g1])
        want = g0.double() + 1.5 * g.double()
        assert float((g1.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
        assert abs(float(v2) - 1.5 * float(v)) <= 2.0 ** -22 * abs(float(v))
        # modes
        v_only = hip.tv_value([xt], [kind], [3.0], scale)
        g2 = g0.clone(memory_format=torch.preserve_format)
        none, _ = hip.tv_value_grad([xt], [kind], [3.0], scale, grads=[g2], value=False)
        assert none is None and torch.equal(v_only, v2) and torch.equal(g2, g1)


def test_all_tensors_in_one_launch_are_deterministic_on_any_stream():
    """the whole field + an env map (13 tensors, one launch): two runs and a run on a side stream give identical bytes, and the value
    and gradients are the per-tensor results"""
    from nmf_amd import hip
    z, m = fixture()
    ts, kinds, ws, ref = [], [], [], 0.0
    for k, kind, fac in cpu.field_table(z):
        ts.append(_dev(z[f"field_{k}"], True)); kinds.append(kind); ws.append(fac)
    ts.append(_dev(z["env_5x130_x"])); kinds.append("env"); ws.append(0.25)
    ref = float(z["field_density_value"]) + float(z["field_app_value"]) + 0.25 * float(z["env_5x130_value"])
    fx = hip.HOST_EXT
    fx.kernel_timing_begin()
    v1, g1 = hip.tv_value_grad(ts, kinds, ws, 1.0)
    probe = {k: c[1] for k, c in fx.kernel_timing_end().items() if not k.startswith("@")}
    assert probe == {"k_tv_fwd_bwd": 1}, probe
    v2, g2 = hip.tv_value_grad(ts, kinds, ws, 1.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v3, g3 = hip.tv_value_grad(ts, kinds, ws, 1.0)
    side.synchronize()
    assert torch.equal(v1, v2) and torch.equal(v1, v3)
    for a, b, c in zip(g1, g2, g3):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert abs(float(v1) - ref) <= (m["value"] + 2.0 ** -22) * abs(ref)
    rows = z["field_rows"]
    for (k, kind, fac), g in zip(cpu.field_table(z), g1):
        got = g.cpu().numpy()[:, :, rows, :] if kind == "plane" else g.cpu().numpy()
        rg = z[f"field_g_{k}"]
        assert np.abs(got.astype(np.float64) - rg).max() <= (m["grad"] + 2.0 ** -23) * np.abs(rg).max()


def test_refused_shapes_write_nothing():
    from nmf_amd import hip
    for shape, kind in (((1, 16, 1, 8), "plane"), ((1, 16, 8, 1), "plane"), ((1, 16, 1, 1), "line"), ((1, 3, 1, 8), "env")):
        x = torch.randn(shape, device=DEV)
        ok = torch.randn(1, 4, 6, 6, device=DEV)
        g = [torch.full(shape, 7.0, device=DEV), torch.full((1, 4, 6, 6), 7.0, device=DEV)]
        with pytest.raises(hip.NmfHipError) as e:
            hip.tv_value_grad([ok, x], ["plane", kind], [1.0, 1.0], 1.0, grads=[g[1], g[0]])
        assert "[-2]" in str(e.value)
        with pytest.raises(hip.NmfHipError):
            hip.tv_value([x], [kind], [1.0], 1.0)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in g)


def test_autograd_route():
    """TVLoss / tv_loss on CUDA tensors through autograd; TV_loss_density / TV_loss_app with the new TVLoss and with a plain torch
    lambda agree within the margin"""
    from nmf_amd.config import build_model
    from nmf_amd.utils import TVLoss, tv_reference
    z, m = fixture()
    reg = TVLoss()
    for name in ("plane_C16_3x5", "line_C24_65", "plane_C1_65x64"):
        x = _dev(cpu.case_input(z, name)).requires_grad_(True)
        v = reg(x) * 2.0
        v.backward()
        ref_v, ref_g = float(z[f"{name}_value"]), z[f"{name}_grad"]
        assert abs(float(v) / 2 - ref_v) <= m["value"] * abs(ref_v)
        assert np.abs(x.grad.cpu().numpy().astype(np.float64) / 2 - ref_g).max() <= m["grad"] * np.abs(ref_g).max()
    with pytest.raises(NotImplementedError):
        reg(torch.zeros(2, 4, 5, 5, device=DEV))
    nerf, _ = build_model(grid=20, bg_resolution=32, device=DEV)
    rf, bgm = nerf.rf, nerf.bg_module
    bgm.bg_mat = torch.nn.Parameter(_dev(z["env_8x16_x"]))
    with torch.no_grad():
        for tag, f in (("d", rf.density_rf), ("a", rf.app_rf)):
            for i in range(3):
                f.app_plane[i].copy_(_dev(z[f"field_{tag}p{i}"]))
                f.app_line[i].copy_(_dev(z[f"field_{tag}l{i}"]))
    rows = z["field_rows"]
    for tag, fn, key in (("d", rf.TV_loss_density, "field_density_value"), ("a", rf.TV_loss_app, "field_app_value")):
        f = rf.density_rf if tag == "d" else rf.app_rf
        ps = list(f.app_plane) + list(f.app_line)
        res = []
        for r in (reg, tv_reference):
            v = fn(r)
            gs = torch.autograd.grad(v, ps)
            res.append((float(v), gs))
            assert abs(float(v) - float(z[key])) <= (m["value"] + 2.0 ** -21) * abs(float(z[key]))
        for i in range(3):
            for j, k in ((i, f"{tag}p{i}"), (3 + i, f"{tag}l{i}")):
                rg = z[f"field_g_{k}"]
                for _, gs in res:
                    got = gs[j].cpu().numpy()
                    got = got[:, :, rows, :] if j < 3 else got
                    assert np.abs(got.astype(np.float64) - rg).max() <= (m["grad"] + 2.0 ** -22) * np.abs(rg).max()
    v = bgm.tv_loss()
    (g,) = torch.autograd.grad(v, bgm.bg_mat)
    assert abs(float(v) - float(z["env_8x16_value"])) <= m["value"] * abs(float(z["env_8x16_value"]))
    rg = z["env_8x16_grad"]
    assert np.abs(g.cpu().numpy().astype(np.float64) - rg).max() <= m["grad"] * np.abs(rg).max()


# ---- the Trainer ---------------------------------------------------------------------------------------------------------------
GRID, BG, CHUNK = 32, 32, 256
# Weights at which the TV gradient of every tensor is at least of the size of the rendering gradient of this small scene.  The TV
# gradient of a tensor is w / lbatch * factor / n_terms per element: 1e-9 at the command line's 0.1, eight orders below the rendering
# gradient and far below one fp32 ulp of it -- a step that dropped the term would pass, and the sum's own rounding (half an ulp of
# the rendering gradient) would be larger than the kernel margin, which is relative to the TV gradient.  The Trainer tests assert
# that every TV gradient is at least 1 % of the gradient it is added to.
TV = dict(TV_weight_density=3e8, TV_weight_app=3e9, TV_weight_bg=1e7)


def _build(dev=DEV):
    from nmf_amd import synthetic
    from nmf_amd.config import build_model, resolved_config
    torch.manual_seed(0)
    over = {"sampler.max_samples": 60000, "model.max_brdf_rays": [120000, 80000], "model.rays_per_ray": 32}
    nerf, _ = build_model(grid=GRID, bg_resolution=BG, device=dev, overrides=over)
    nerf.load_state_dict(synthetic.state_dict_s1(grid=GRID, bg_resolution=BG, seed=0), strict=False)
    nerf.train()
    nerf.sampler.update(nerf.rf, init=False)
    nerf.sampler.update(nerf.rf, init=True)
    nerf.model.detach_N = False
    nerf.model.max_retrace_rays = [nerf.model.max_brdf_rays[0]]
    return nerf, dict(resolved_config()["params"])


def _data(dev=DEV):
    from nmf_amd import synthetic
    rays, focal = synthetic.camera_rays(2 * CHUNK, seed=77)
    gt = torch.rand(2 * CHUNK, 3, generator=torch.Generator().manual_seed(5)) * 0.6 + 0.2
    return rays.to(dev), gt.to(dev), focal


def _tv_params(nerf):
    rf = nerf.rf
    return ([("d", p) for p in list(rf.density_rf.app_plane) + list(rf.density_rf.app_line)]
            + [("a", p) for p in list(rf.app_rf.app_plane) + list(rf.app_rf.app_line)] + [("b", nerf.bg_module.bg_mat)])


def _expected_tv(nerf, sums):
    """(sum_k w_k / lbatch) * TV and its gradient per TV parameter, in float64 on the CPU by the fixture-pinned expressions"""
    from nmf_amd.utils import tv_reference
    total, grads = 0.0, []
    for tag, p in _tv_params(nerf):
        x = p.detach().cpu().double().contiguous().requires_grad_(True)
        if tag == "b":
            img = x[0]
            v = ((img[1:, :-1] - img[:-1, :-1]).abs() + (img[:-1, 1:] - img[:-1, :-1]).abs() + 1e-8).mean() * sums[2]
        else:
            v = tv_reference(x) * (1e-3 if x.shape[-1] == 1 else 1e-2) * sums[0 if tag == "d" else 1]
        (g,) = torch.autograd.grad(v, x)
        total += float(v)
        grads.append(g)
    return total, grads


def _grads(nerf):
    return [p.grad.detach().double().cpu().clone() for _, p in _tv_params(nerf)]


@pytest.mark.parametrize("tape_free", [True, False])
def test_trainer_step_adds_the_tv_gradient(tape_free):
    """S1 at G = 32, 512 rays as two chunks, injected noise, three steps: every TV parameter's .grad = the same step with the weights 0
    (from the same parameters) + (sum_k w_k / lbatch) grad TV; tolerance = the kernel margin + twice the largest difference between
    two TV-off runs of that step; last_tv is the weighted value; the weights decay as train.py:684-709 says"""
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.trainer import Trainer
    z, m = fixture()
    rays, gt, focal = _data()
    nerf, params = _build()
    on = Trainer(nerf, dict(params, **TV), tape_free=tape_free)
    offs = []
    for _ in range(2):
        n2, p2 = _build()
        offs.append((n2, Trainer(n2, p2, tape_free=tape_free)))
    lbatch = 2 * CHUNK
    sched, _ = cpu.reference_schedule(dict(params, **TV), -1, 0.1, [[True, True]] * 3, lbatch)
    for it in range(3):
        ref = []
        for n2, t2 in offs:
            with torch.no_grad():
                for a, b in zip(n2.parameters(), nerf.parameters()):
                    a.copy_(b)
            t2.step(rays, gt, focal, noise=DeviceNoise(torch.device(DEV), seed=100 + it), update_controllers=False, fixed_chunk=CHUNK)
            ref.append(_grads(n2))
        want_v, want_g = _expected_tv(nerf, sched[it])
        out = on.step(rays, gt, focal, noise=DeviceNoise(torch.device(DEV), seed=100 + it), update_controllers=False,
                      fixed_chunk=CHUNK)
        assert out["chunks"] == 2 and tuple(on.tv.sums) == sched[it]
        got = _grads(nerf)
        for (tag, p), g, r0, r1, tg in zip(_tv_params(nerf), got, ref[0], ref[1], want_g):
            spread = float((r0 - r1).abs().max())
            tol = m["grad"] * float(tg.abs().max()) + 2 * spread
            err = float((g - (r0 + tg)).abs().max())
            print(f"step {it} {tag} {tuple(p.shape)}: |err| {err:.3e} tol {tol:.3e} (two TV-off runs differ by {spread:.3e}, "
                  f"max |w grad TV| {float(tg.abs().max()):.3e}, max |grad| {float(r0.abs().max()):.3e})")
            assert float(tg.abs().max()) >= 1e-2 * float(r0.abs().max()), "the TV gradient is too small for this test to see it"
            assert err <= tol
        assert abs(float(on.last_tv) - want_v) <= m["value"] * abs(want_v), (float(on.last_tv), want_v)
        assert abs(out["tv"] - want_v) <= m["value"] * abs(want_v)
    _, final = cpu.reference_schedule(dict(params, **TV), -1, 0.1, [[True, True]] * 3, lbatch)
    assert (on.tv_weight_density, on.tv_weight_app) == final
    if tape_free:
        assert nerf.operator_graph_forwards == 0


def test_launch_counts():
    """weights 0: the TV entry point is not reached and the step launches what it launched before; weights on: one launch more"""
    from nmf_amd import hip
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.trainer import Trainer
    rays, gt, focal = _data()
    counts = []
    for extra in ({}, TV):
        nerf, params = _build()
        tr = Trainer(nerf, dict(params, **extra))
        torch.cuda.synchronize()
        hip.HOST_EXT.kernel_timing_begin()
        tr.step(rays, gt, focal, noise=DeviceNoise(torch.device(DEV), seed=100), update_controllers=False, fixed_chunk=CHUNK)
        counts.append({k: c[1] for k, c in hip.HOST_EXT.kernel_timing_end().items() if not k.startswith("@")})
        assert (tr.last_tv is None) == (not extra)
    off, on = counts
    print("launches per step", sum(off.values()), "->", sum(on.values()))
    assert "k_tv_fwd_bwd" not in off
    assert on == dict(off, k_tv_fwd_bwd=1)


# ---- data parallel -----------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _PerChunkNoise:
    pins = None

    def __init__(self, sources):
        self.sources, self.k = sources, -1

    def begin_pass(self):
        self.k = (self.k + 1) % len(self.sources)
        self.sources[self.k].begin_pass()

    def __getattr__(self, name):
        return getattr(self.sources[self.k], name)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.trainer import Trainer, rank_slice
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    nerf, params = _build(dev)
    tr = Trainer(nerf, dict(params, **TV), world_size=world, rank=rank, check_every=1)
    rays, gt, focal = _data(dev)
    sl = rank_slice(2 * CHUNK, world, rank)
    tr.step(rays[sl], gt[sl], focal, noise=DeviceNoise(dev, seed=100 + rank), update_controllers=False, fixed_chunk=CHUNK,
            global_rays=2 * CHUNK)
    res = dict(bg=nerf.bg_module.bg_mat.grad.detach().cpu().clone(), dp=nerf.rf.density_rf.app_plane[0].grad.detach().cpu().clone(),
               tv=float(tr.last_tv))
    for it in range(2):                       # ReplicaDivergence would raise here (check_every=1)
        tr.step(rays[sl], gt[sl], focal, noise=DeviceNoise(dev, seed=300 + 2 * it + rank), update_controllers=False,
                fixed_chunk=CHUNK, global_rays=2 * CHUNK)
    res["checks"] = tr.replica_checks
    out[rank] = res
    dist.destroy_process_group()


def test_two_ranks_equal_one_process():
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.trainer import Trainer
    z, m = fixture()
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        res = dict(out)
    assert res[0]["checks"] == res[1]["checks"] == 3
    assert torch.equal(res[0]["bg"], res[1]["bg"]) and torch.equal(res[0]["dp"], res[1]["dp"])
    rays, gt, focal = _data()
    dev = torch.device(DEV)
    runs = []
    for extra in (TV, {}, {}):
        nerf, params = _build()
        tr = Trainer(nerf, dict(params, **extra))
        tr.step(rays, gt, focal, noise=_PerChunkNoise([DeviceNoise(dev, seed=100), DeviceNoise(dev, seed=101)]),
                update_controllers=False, fixed_chunk=CHUNK)
        runs.append((nerf.bg_module.bg_mat.grad.detach().cpu().clone(), nerf.rf.density_rf.app_plane[0].grad.detach().cpu().clone(),
                     tr, nerf))
    _, want_g = _expected_tv(runs[0][3], runs[0][2].tv.sums)
    for key, i, tg in (("bg", 0, want_g[-1]), ("dp", 1, want_g[0])):
        spread = float((runs[1][i].double() - runs[2][i].double()).abs().max())
        tol = m["grad"] * float(tg.abs().max()) + 2 * spread
        err = float((res[0][key].double() - runs[0][i].double()).abs().max())
        print(f"{key}: two ranks vs one process |err| {err:.3e} tol {tol:.3e} (two TV-off runs differ by {spread:.3e})")
        assert float(tg.abs().max()) >= 1e-2 * float(runs[1][i].abs().max()), "the TV gradient is too small for this test to see it"
        assert err <= tol
    assert abs(res[0]["tv"] + res[1]["tv"] - float(runs[0][2].last_tv)) <= 2.0 ** -20 * float(runs[0][2].last_tv)
