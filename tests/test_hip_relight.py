"""Relighting on the GPU: csrc/envmap_resample.hip against the float64 restatement of tests/test_relight_cpu.py (tolerance: its
restatement_margin), resampled maps through IntegralEquirect.forward, the module swap under the fused eval pass, and the command lines."""
import json
import math
import os

import numpy as np
import pytest
import torch

from nmf_amd import hip, relight, synthetic
from test_hip_metrics import _s1_model
from test_relight_cpu import H, SA, W, cases, error_ratios, lookup_bias, module_source, restatement, restatement_margin, rotations

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(name):
    src, kind, R, gain, S, h, w = cases()[name]
    out = torch.full((3, h, w), float("nan"), device=DEV)
    hip.env_resample(torch.from_numpy(src).to(DEV), kind, R, gain, S, out)
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", sorted(cases()))
def test_kernel_matches_the_float64_restatement(name):
    """rows 1..H-1, every column, within restatement_margin(); row 0 (the exact pole: its azimuth is undefined and differs between
    fp32 and float64) by its mean"""
    got, want = _run(name), restatement(name)
    margin = restatement_margin()
    err = np.abs(got - want)
    print(name, "max error", err[:, 1:].max(), "row-0 mean error", np.abs(got[:, 0].mean(axis=1) - want[:, 0].mean(axis=1)).max(),
          "margin", margin)
    assert np.isfinite(got).all()
    assert err[:, 1:].max() <= margin
    # row 0: 64 (32) samples of the pole's neighbourhood at undefined azimuths; their mean agrees to the spread of that neighbourhood
    pole_spread = np.ptp(want[:, 0], axis=1).max()
    assert np.abs(got[:, 0].mean(axis=1) - want[:, 0].mean(axis=1)).max() <= margin + pole_spread


def test_yaw_by_eight_texels_is_a_roll_and_runs_are_bit_identical():
    got = _run("module-yaw8-S1")
    want = np.log(cases()["module-yaw8-S1"][0].astype(np.float64))
    want[:, :, 1:] = np.roll(want[:, :, 1:], 8, axis=2)
    assert np.abs(got[:, 1:, 1:] - want[:, 1:, 1:]).max() <= restatement_margin()
    g = torch.Generator(device="cpu").manual_seed(0)
    src = torch.rand((3, 512, 1024), generator=g).add_(0.05).to(DEV)
    pano = src.permute(1, 2, 0).contiguous()
    R = rotations()["axis"]
    for s, kind in ((src, hip.ENV_SRC_MODULE), (pano, hip.ENV_SRC_PANORAMA)):
        a = hip.env_resample(s, kind, R, 1.0, 4, torch.empty((3, 512, 1024), device=DEV))
        b = hip.env_resample(s, kind, R, 1.0, 4, torch.zeros((1, 3, 512, 1024), device=DEV))
        assert torch.equal(a, b[0]) and bool(torch.isfinite(a).all())


def test_wrapper_refuses_what_the_kernel_must_not_see():
    src, out = torch.ones((3, 8, 16), device=DEV), torch.zeros((3, 8, 16), device=DEV)
    for bad in (lambda: hip.env_resample(src.double(), 0, np.eye(3), 1.0, 1, out),
                lambda: hip.env_resample(src[:, :, ::2], 0, np.eye(3), 1.0, 1, out),
                lambda: hip.env_resample(src, 1, np.eye(3), 1.0, 1, out),                    # [3,8,16] is no [Hp,Wp,3]
                lambda: hip.env_resample(src, 0, np.eye(3), 1.0, 1, out[:2]),
                lambda: hip.env_resample(src, 0, np.eye(3), 1.0, 1, src),
                lambda: hip.env_resample(src, 0, np.eye(3), 1.0, 9, out),
                lambda: hip.env_resample(src, 0, 2 * np.eye(3), 1.0, 1, out),
                lambda: hip.env_resample(src.cpu(), 0, np.eye(3), 1.0, 1, out)):
        with pytest.raises(hip.NmfHipError):
            bad()
    assert float(out.abs().max()) == 0


# ---- through IntegralEquirect.forward -----------------------------------------------------------------------------------------------
def _module(bg_log, brightness=0.0, mul=1.0):
    h = bg_log.shape[-2]
    m = relight._fixed_module(h, 0, DEV)
    with torch.no_grad():
        m.bg_mat.copy_(torch.as_tensor(np.asarray(bg_log), dtype=torch.float32).reshape(1, 3, h, 2 * h))
        m.brightness.fill_(brightness)
        m.mul.fill_(mul)
    return m


def _lookup(m, dirs):
    d = torch.as_tensor(np.asarray(dirs), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        return m(d, torch.full((d.shape[0],), SA, device=DEV))


def _device_lookup(bg_log, dirs):
    return _lookup(_module(bg_log), dirs).cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("rot", ["identity", "yaw90", "x90", "axis"])
def test_rotated_and_imported_maps_through_the_module_lookup(rot):
    R = rotations()[rot]
    src = _module(np.log(module_source(H, W)))
    turned = relight.rotate_env(src, R, supersample=4)
    mx, mean, n = error_ratios(turned.bg_mat.detach()[0].cpu().numpy().astype(np.float64), R, lookup=_device_lookup)
    print("rotation", rot, "queries", n, "max ratio", mx, "mean ratio", mean)
    assert mx <= 1.5 and mean <= 1.25
    imported = relight.import_panorama(cases()[f"pano-{rot}-S4"][0], H, R=R, supersample=4)
    mx, mean, n = error_ratios(imported.bg_mat.detach()[0].cpu().numpy().astype(np.float64), R, lookup=_device_lookup, target_bias=1.0)
    print("import", rot, "queries", n, "max ratio", mx, "mean ratio", mean)
    assert mx <= 1.5 and mean <= 1.25
    for m in (turned, imported):
        assert m.hw() == (H, W) and [float(p.detach()) for p in (m.brightness, m.mul, m.mipbias)] == [0, 1, 0]


def test_brightness_and_mul_are_baked_in_and_resize_keeps_the_level():
    log_src = np.log(module_source(H, W))
    src = _module(log_src, brightness=0.3, mul=0.8)
    with torch.no_grad():
        src.mipbias.fill_(1.0)
    same = relight.rotate_env(src, np.eye(3), supersample=1)
    assert [float(p.detach()) for p in (same.brightness, same.mul, same.mipbias)] == [0, 1, 1]
    assert [g["lr"] for g in same.get_optparam_groups()] == [0, 0, 0, 0]
    want = 0.3 + 0.8 * src.bg_mat.detach()[0].double().cpu().numpy()
    err = np.abs(same.bg_mat.detach()[0].double().cpu().numpy() - want)[:, 1:].max()
    print("identity with brightness / mul", err, "margin", restatement_margin())
    assert err <= restatement_margin()
    # a smaller destination: gain = bias(src) / bias(dst) on the source's activated table (the kernel at that gain is held to the
    # restatement by the case module-resize-axis-S4)
    small = relight.rotate_env(src, rotations()["axis"], res=16, supersample=4)
    assert small.hw() == (16, 32)
    direct = hip.env_resample(src._tables()[0], hip.ENV_SRC_MODULE, rotations()["axis"], lookup_bias(H, W) / lookup_bias(16, 32), 4,
                              torch.empty((3, 16, 32), device=DEV))
    assert torch.equal(small.bg_mat.detach()[0], direct)


def test_out_reuse_rebuilds_the_tables_in_place():
    rots = rotations()
    src = _module(np.log(module_source(H, W)))
    q = np.random.default_rng(7).normal(size=(3000, 3))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    m = relight.rotate_env(src, rots["yaw90"])
    first = _lookup(m, q).clone()
    sh_first = [t.clone() for t in m.get_spherical_harmonics(100)]
    tables = [t.data_ptr() for t in m._cache[1]]
    assert relight.rotate_env(src, rots["axis"], out=m) is m
    fresh = relight.rotate_env(src, rots["axis"])
    assert torch.equal(m.bg_mat, fresh.bg_mat)
    got, want = _lookup(m, q), _lookup(fresh, q)
    assert torch.equal(got, want) and not torch.equal(got, first)
    for a, b, c in zip(m.get_spherical_harmonics(100), fresh.get_spherical_harmonics(100), sh_first):
        assert torch.equal(a, b) and not torch.equal(a, c)
    assert [t.data_ptr() for t in m._cache[1]] == tables                      # rebuilt in place
    with pytest.raises(ValueError):
        relight.rotate_env(src, rots["axis"], out=src)
    with pytest.raises(ValueError):
        relight.rotate_env(src, rots["axis"], res=16, out=m)


# ---- the module swap under the fused eval pass ----------------------------------------------------------------------------------
def _frame(nerf, rays, focal):
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import render_images
    with torch.no_grad():
        return render_images(nerf, rays, focal, noise=DeviceNoise(torch.device(DEV), seed=5)).clone()


def test_relit_swaps_the_map_under_the_fused_eval_pass():
    """render, swap the map in with relit(), render: the fused pass must not go on reading the replaced module's tables"""
    R = relight.rotation(yaw=70, pitch=25)
    r, focal = synthetic.orbit_rays(1, 32, seed=2)
    rays = r.reshape(-1, 6).to(DEV)

    def fresh():
        nerf, _ = _s1_model()
        nerf.bg_module = relight.rotate_env(nerf.bg_module, R)
        return _frame(nerf, rays, focal)

    f1, f2 = fresh(), fresh()
    agreement = float((f1 - f2).abs().max())                                   # what two fresh renders show (0: bit-identity)
    nerf, _ = _s1_model()
    before = _frame(nerf, rays, focal)
    assert torch.equal(before, _frame(nerf, rays, focal))
    own = nerf.bg_module
    with relight.relit(nerf, relight.rotate_env(own, R)) as n:
        assert n is nerf and nerf.bg_module is not own
        during = _frame(nerf, rays, focal)
    assert nerf.bg_module is own
    after = _frame(nerf, rays, focal)
    print("fresh-render agreement", agreement, "relit vs fresh", float((during - f1).abs().max()),
          "relit vs before", float((during - before).abs().max()))
    assert float((during - f1).abs().max()) <= agreement
    assert float((during - before).abs().max()) > 1e-3
    assert torch.equal(after, before)


# ---- command lines ------------------------------------------------------------------------------------------------------------------
def test_render_light_turntable_and_direct_panorama_import(tmp_path, capsys):
    from PIL import Image
    from nmf_amd import pano2env
    from nmf_amd import render as Rn
    nerf, cfg = _s1_model()
    ck = str(tmp_path / "m.th")
    nerf.save(ck, cfg["arch"])
    out = tmp_path / "imgs"
    rec = Rn.main(["--ckpt", ck, "--views", "1", "--res", "32", "--light-turntable", "3", "--out", str(out)])
    line = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    assert line == json.loads(json.dumps(rec))
    assert rec["frames"] == 1 and rec["light_frames"] == 3 and not rec["relit"]
    assert len(rec["light_env_seconds"]) == len(rec["light_render_seconds"]) == 3
    assert all(v > 0 for v in rec["light_env_seconds"] + rec["light_render_seconds"])
    frames = [np.asarray(Image.open(out / f"light_{k:03d}.png")).astype(np.float32) for k in range(3)]
    assert os.path.exists(out / "000.png") and not os.path.exists(out / "light_003.png")
    for a in range(3):
        assert frames[a].shape == (32, 32, 3)
        for b in range(a + 1, 3):
            assert np.abs(frames[a] - frames[b]).mean() > 0.5, (a, b)
    plain = Rn.main(["--ckpt", ck, "--views", "1", "--res", "32"])
    assert set(rec) - set(plain) == {"light_frames", "light_env_seconds", "light_render_seconds"}

    th = str(tmp_path / "env" / "studio.th")
    prec = pano2env.main([os.path.join(GOLDEN, "studio_dwab.exr"), "--direct", "--res", "32", "--output", th])
    assert prec["direct"] and prec["resolution"] == 32 and prec["panorama"] == [512, 1024, 3] and math.isfinite(prec["psnr"])
    assert os.path.exists(tmp_path / "env" / "studio_pano.exr")
    bg = Rn.load_fixed_bg(th, DEV)
    assert bg.bg_mat.shape == (1, 3, 32, 64) and bool(torch.isfinite(bg.bg_mat).all())
    rec2 = Rn.main(["--ckpt", ck, "--views", "1", "--res", "32", "--fixed-bg", th, "--env-rotate", "40", "10", "0",
                    "--out", str(tmp_path / "relit")])
    assert rec2["relit"] and "light_frames" not in rec2
    rec3 = Rn.main(["--ckpt", ck, "--views", "1", "--res", "32", "--fixed-bg", os.path.join(GOLDEN, "studio_dwab.exr"), "--bg-res", "32",
                    "--out", str(tmp_path / "direct")])
    a = np.asarray(Image.open(tmp_path / "relit" / "000.png")).astype(np.float32)
    b = np.asarray(Image.open(tmp_path / "direct" / "000.png")).astype(np.float32)
    assert rec3["relit"] and np.abs(a - b).mean() > 0.5                        # the same map, turned
