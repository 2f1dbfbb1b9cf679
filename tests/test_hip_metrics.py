"""Evaluation metrics on the GPU: nmf_ssim against the reference's utils.rgb_ssim (tests/golden/metrics.npz) and the float64
restatement, nmf_normal_err against the torch expression of renderer.py:369-389, renderer.evaluation end to end and the
--render-test / --eval-dir command lines."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from nmf_amd import hip, synthetic
from test_metrics_cpu import GOLDEN, normal_err_np, ssim_np

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_hip_ssim_matches_the_reference_golden():
    z = np.load(GOLDEN)
    for name in z["names"]:
        a, b = (torch.from_numpy(z[f"{name}_{k}"]).to(DEV) for k in "ab")
        got = hip.ssim(a, b, max_val=1.0)
        assert got.dtype == torch.float64 and got.shape == (1,)
        assert abs(float(got[0]) - float(z[f"{name}_ssim"])) <= 1e-9, name
    mk = [k for k in z.files if k.startswith("map_")][0]
    a, b = (torch.from_numpy(z[f"{mk[4:]}_{k}"]).to(DEV) for k in "ab")
    mean, smap = hip.ssim(a, b, return_map=True)
    assert smap.shape == (1,) + z[mk].shape and smap.dtype == torch.float32
    assert np.abs(smap[0].cpu().numpy().astype(np.float64) - z[mk]).max() <= 1e-6


def _views(n, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.rand(n, H // 16 + 1, W // 16 + 1, 3, device=DEV, generator=g)
    gt = torch.nn.functional.interpolate(base.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
    gt = gt.permute(0, 2, 3, 1).contiguous()
    pred = (gt + 0.05 * torch.randn(gt.shape, device=DEV, generator=g)).clip(0, 1)
    return (torch.floor(pred * 255) / 255).contiguous(), gt


@pytest.mark.gpu
def test_hip_ssim_batched_800_views_is_deterministic_and_matches_float64():
    pred, gt = _views(8, 800, 800, seed=5)
    batched = hip.ssim(pred, gt)
    again = hip.ssim(pred, gt)
    single = torch.cat([hip.ssim(pred[i], gt[i]) for i in range(8)])
    assert torch.equal(batched, again) and torch.equal(batched, single)          # bit-identical: fixed-order fp64 sums
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    for i in range(8):
        assert abs(float(batched[i]) - ssim_np(p[i], g[i])) <= 1e-9, i
    assert hip.ssim(pred[:0], gt[:0]).shape == (0,)


@pytest.mark.gpu
def test_rgb_ssim_takes_cpu_and_device_images():
    from nmf_amd.utils import rgb_ssim
    pred, gt = _views(1, 37, 52, seed=9)
    on_dev = rgb_ssim(pred[0], gt[0], 1)
    assert isinstance(on_dev, float)
    assert rgb_ssim(pred[0].cpu(), gt[0].cpu(), 1) == on_dev
    assert rgb_ssim(pred[0].cpu().numpy(), gt[0].cpu().numpy(), 1) == on_dev
    assert on_dev == pytest.approx(ssim_np(pred[0].cpu().numpy(), gt[0].cpu().numpy()), abs=1e-9)
    m = rgb_ssim(pred[0], gt[0], 1, return_map=True)
    assert isinstance(m, np.ndarray) and m.shape == (27, 42, 3)
    assert float(m.astype(np.float64).mean()) == pytest.approx(on_dev, abs=1e-6)


def _torch_normal_err(pnorms, gt_normal, acc):
    """renderer.py:369-389 as written (fp32 torch, on the tensors' device)"""
    pnorms = (pnorms * 127 + 128).int()
    pnorms = (pnorms - 128) / 127
    gt_normal = (gt_normal * 127 + 128).int()
    gt_normal = (gt_normal - 128) / 127
    gt_normal = gt_normal / ((gt_normal ** 2).sum(dim=-1, keepdim=True) + 1e-6).sqrt()
    pnorms = pnorms / ((pnorms ** 2).sum(dim=-1, keepdim=True) + 1e-6).sqrt()
    norm_err = torch.arccos((pnorms * gt_normal).sum(dim=-1).clip(min=1e-8, max=1 - 1e-8)) * 180 / np.pi
    norm_err[torch.isnan(norm_err)] = 0
    norm_err *= acc
    return norm_err.sum() / acc.sum(), norm_err


@pytest.mark.gpu
def test_hip_normal_err_matches_the_torch_expression():
    g = torch.Generator(device=DEV).manual_seed(4)
    n, P = 3, 64 * 48 + 5
    gt = torch.nn.functional.normalize(torch.randn(n, P, 3, device=DEV, generator=g), dim=-1)
    pred = torch.nn.functional.normalize(gt + 0.3 * torch.randn(n, P, 3, device=DEV, generator=g), dim=-1)
    pred[1, : P // 2] = gt[1, : P // 2]                                           # equal normals on half a view
    acc = torch.rand(n, P, device=DEV, generator=g)
    acc[2, :100] = 0
    vals, emap = hip.normal_err(pred, gt, acc, return_map=True)
    assert vals.dtype == torch.float64 and vals.shape == (n,) and emap.shape == acc.shape
    assert torch.equal(vals, hip.normal_err(pred, gt, acc))
    for i in range(n):
        ref, ref_map = _torch_normal_err(pred[i], gt[i], acc[i])
        assert abs(float(vals[i]) - float(ref)) <= 1e-3, i
        assert (emap[i] - ref_map).abs().max().item() <= 2e-2
        assert float(hip.normal_err(pred[i], gt[i], acc[i])[0]) == float(vals[i])      # independent of the batch
    # closed forms (tests/test_metrics_cpu.py): equal, perpendicular, opposite, zero alpha, NaN pixel
    z = torch.tensor([[0.0, 0.0, 1.0]], device=DEV)
    one = torch.ones(1, device=DEV)
    assert float(hip.normal_err(z, z, one)[0]) == pytest.approx(normal_err_np(z.cpu().numpy(), z.cpu().numpy(), [1.0]), abs=1e-2)
    assert float(hip.normal_err(torch.tensor([[1.0, 0, 0]], device=DEV), z, one)[0]) == pytest.approx(90.0, abs=1e-4)
    assert float(hip.normal_err(-z, z, one)[0]) == pytest.approx(90.0, abs=1e-4)
    assert np.isnan(float(hip.normal_err(z, z, torch.zeros(1, device=DEV))[0]))
    pn = torch.tensor([[1.0, 0, 0], [float("nan"), 0, 0]], device=DEV)
    v, m = hip.normal_err(pn, torch.cat([z, z]), torch.ones(2, device=DEV), return_map=True)
    assert float(m[1]) == 0.0 and float(v[0]) == pytest.approx(float(m[0]) / 2, abs=1e-9)


# ---- renderer.evaluation -----------------------------------------------------------------------------------------------
def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _s1_model(grid=32, bg=32):
    from nmf_amd.config import build_model
    nerf, cfg = build_model(grid=grid, bg_resolution=bg, device=DEV)
    nerf.load_state_dict(synthetic.state_dict_s1(grid=grid, bg_resolution=bg, seed=0), strict=False)
    nerf.sampler.update(nerf.rf, init=False)
    nerf.sampler.update(nerf.rf, init=True)
    nerf.eval()
    return nerf, cfg


@pytest.mark.gpu
def test_evaluation_end_to_end(tmp_path):
    from PIL import Image
    from nmf_amd.dataLoader import BlenderDataset
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import evaluation, psnr_8bit, render_images
    scene = tmp_path / "scene"
    _load_tool("make_blender_scene").main(["--out", str(scene), "--views", "1", "--test-views", "3", "--res", "64",
                                           "--grid", "32", "--bg", "32"])
    rng = np.random.default_rng(2)
    for i in (0, 2):                                                  # ground-truth normals for two of the three views
        n = rng.normal(size=(64, 64, 3))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        Image.fromarray((n * 127 + 128).clip(0, 255).astype(np.uint8), "RGB").save(scene / "test" / f"r_{i}_normal.png")
    ds = BlenderDataset(str(scene), split="test", is_stack=True, N_vis=-1)
    nerf, _ = _s1_model()
    out = tmp_path / "imgs_test_all"
    res = evaluation(ds, nerf, None, None, str(out), N_vis=-1, noise=DeviceNoise(torch.device(DEV), seed=21), prtx="t_")
    assert len(res["psnrs"]) == len(res["ssims"]) == 3 and len(res["norm_errs"]) == 2
    noise = DeviceNoise(torch.device(DEV), seed=21)
    for i in range(3):
        ims = render_images(nerf, ds.all_rays[i].to(DEV), float(ds.fx), noise=noise, keys=("rgb_map", "acc_map", "world_normal"))
        gt = ds.all_rgbs[i].to(DEV)
        assert res["psnrs"][i] == pytest.approx(float(psnr_8bit(ims["rgb_map"].reshape(64, 64, 3), gt)), abs=1e-5)
        png = np.asarray(Image.open(out / f"t_{i:03d}.png")).astype(np.float32) / 255
        assert abs(res["ssims"][i] - ssim_np(png, ds.all_rgbs[i].numpy())) <= 1e-7, i
        for sub in ("world_normal", "acc_map", "err"):
            assert os.path.exists(out / sub / f"t_{i:03d}.png"), sub
    mean = np.loadtxt(out / "t_mean.txt")
    assert mean.shape == (4,) and np.isnan(mean[2:]).all()
    assert mean[0] == pytest.approx(np.mean(res["psnrs"])) and mean[1] == pytest.approx(np.mean(res["ssims"]))
    import yaml
    stats = yaml.safe_load(open(out / "statst_.yaml"))
    assert set(stats) == {"psnr", "ssim", "norm_err"}
    assert stats["norm_err"] == pytest.approx(np.mean(res["norm_errs"])) and 0 < stats["norm_err"] < 180
    # without extra metrics: one column; without normal maps norm_err is 0
    for i in (0, 2):
        os.remove(scene / "test" / f"r_{i}_normal.png")
    res2 = evaluation(ds, nerf, None, None, str(out), N_vis=1, compute_extra_metrics=False)      # every 3rd view: view 0
    assert len(res2["psnrs"]) == 1 and res2["ssims"] == [] and res2["norm_errs"] == []
    assert np.loadtxt(out / "mean.txt").shape == ()
    assert yaml.safe_load(open(out / "stats.yaml")) == {"psnr": pytest.approx(np.mean(res2["psnrs"])), "norm_err": 0}


def _tiny_scene(root):
    """the scene of tests/test_hip_e2e.py::test_train_cli_on_a_blender_scene"""
    from PIL import Image
    rng = np.random.default_rng(1)
    os.makedirs(root / "train")
    frames = []
    for i in range(3):
        rgba = rng.integers(0, 256, size=(16, 16, 4), dtype=np.uint8)
        Image.fromarray(rgba, "RGBA").save(root / "train" / f"r_{i}.png")
        ang = 2 * np.pi * i / 3
        c2w = np.eye(4)
        c2w[:3, 3] = [4 * np.cos(ang), 4 * np.sin(ang), 0.5]
        fwd = -c2w[:3, 3] / np.linalg.norm(c2w[:3, 3])
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2] = right, up, -fwd
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": c2w.tolist()})
    meta = {"camera_angle_x": 0.69, "w": 16, "h": 16, "frames": frames}
    for split in ("train", "test"):
        json.dump(meta, open(root / f"transforms_{split}.json", "w"))


def _json_lines(capsys):
    return [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_train_render_test_and_render_eval_dir(tmp_path, capsys, monkeypatch):
    from nmf_amd import render as R
    from nmf_amd import train as T
    scene = tmp_path / "tiny"
    _tiny_scene(scene)
    monkeypatch.chdir(tmp_path)                                       # ./log/<scene>_test/ lands here
    ck = str(tmp_path / "out.th")
    flags = ["--datadir", str(scene), "--near-far", "2.5", "7", "--iters", "3", "--grid", "16", "--bg", "16", "--eval-every", "3",
             "--test-views", "1", "--save", ck]
    T.main(flags)
    plain = _json_lines(capsys)
    assert len(plain) == 1 and "test_all" not in plain[0] and not os.path.exists(tmp_path / "log")
    T.main(flags + ["--render-test"])
    lines = _json_lines(capsys)
    assert len(lines) == 2 and set(lines[0]) == set(plain[0])
    ta = lines[-1]["test_all"]
    assert ta["views"] == 3 and np.isfinite(ta["psnr"]) and 0 < ta["ssim"] <= 1 and ta["norm_err"] == 0
    folder = tmp_path / "log" / "tiny_test" / "imgs_test_all"
    assert np.loadtxt(folder / "mean.txt").shape == (4,) and os.path.exists(folder / "002.png")

    rec = R.main(["--ckpt", ck, "--datadir", str(scene)])
    assert "ssim" not in rec and "norm_err" not in rec and "eval_seconds" not in rec
    rec = R.main(["--ckpt", ck, "--datadir", str(scene), "--eval-dir", str(tmp_path / "ev")])
    assert 0 < rec["ssim"] <= 1 and rec["norm_err"] == 0 and rec["eval_seconds"]["total"] > 0
    assert np.isfinite(rec["psnr"]) and np.isfinite(np.loadtxt(tmp_path / "ev" / "mean.txt")).sum() == 2
    assert os.path.exists(tmp_path / "ev" / "stats.yaml")
    capsys.readouterr()
    with pytest.raises(SystemExit):
        T.main(["--iters", "1", "--render-test"])                     # the synthetic orbit has no test split on disk
    with pytest.raises(SystemExit):
        R.main(["--ckpt", ck, "--eval-dir", str(tmp_path / "x")])
