"""Relighting evaluation on the GPU: the three kernels of csrc/relight_eval.hip against the float64 restatement of
tests/relight_eval_ref.py, `rgb_lin` from the fused evaluation pass against the module path, and `render --relight-eval` end to end.

Tolerances.  Float outputs: relight_eval_ref.margins(), 4 x the distance of the fp32 restatement (the kernels' expression order, numpy's
powf) from the float64 one over the inputs of every shape -- derived on the CPU, printed next to what the GPU shows.  Counts: exact.
Double sums: relative 1e-12 against the float64 sum of the same fp32 terms (at most 6633 terms of one sign: the order of a double sum
moves it by parts in 1e-13).  Ratio sums against the float64 restatement itself: every term is one correctly rounded fp32 quotient of
positive numbers, so the sum is within 2^-24 of it, relative."""
import json
import os

import numpy as np
import pytest
import torch

import relight_eval_ref as ref
from nmf_amd import hip, relight, synthetic
from test_hip_metrics import _load_tool, _s1_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def margins():
    return ref.margins()


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frame_kernel_matches_the_float64_restatement(shape, margins):
    lin, acc = ref.frame_inputs(*shape)
    got = hip.relight_frame(_t(lin), _t(acc))
    again = hip.relight_frame(_t(lin).reshape(-1, 3), _t(acc).reshape(-1)).reshape(got.shape)       # [N,3]: the renderer's layout
    err = ref.rel_floor1(got.cpu().numpy(), ref.frame(lin, acc))
    print("frame", shape, "max error / max(|want|, 1)", err.max(), "margin", margins["frame"])
    assert got.shape == lin.shape and bool(torch.isfinite(got).all())
    assert err.max() <= margins["frame"]
    assert torch.equal(got, again)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ratio_kernel_counts_and_sums(shape):
    pred, gt = ref.inputs(*shape)
    sums, counts = hip.relight_ratio(_t(pred), _t(gt))
    sums2, counts2 = hip.relight_ratio(_t(pred), _t(gt))
    want64, want_counts = ref.ratio(pred, gt)
    want32, _ = ref.ratio(pred, gt, np.float32)
    got = sums.cpu().numpy()
    print("ratio", shape, "counts", counts.tolist(), "max relative distance from the sum of the fp32 terms",
          (np.abs(got - want32) / np.maximum(want32, 1e-300)).max(), "from float64", (np.abs(got - want64) / np.maximum(want64, 1e-300)).max())
    assert sums.dtype == torch.float64 and counts.dtype == torch.int64 and sums.shape == (shape[0], 3)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    if shape[0] > 1:
        assert want_counts[1] == 0 and (got[1] == 0).all() and want_counts[0] > 0          # the empty image; the SPECIAL pixels count
    assert (np.abs(got - want32) <= 1e-12 * np.abs(want32)).all()
    assert (np.abs(got - want64) <= (2.0 ** -24 + 1e-12) * np.abs(want64)).all()
    assert torch.equal(sums, sums2) and torch.equal(counts, counts2)
    if shape[0] > 1:           # an image's result does not depend on what else is in the batch
        s1, c1 = hip.relight_ratio(_t(pred[2]), _t(gt[2]))
        assert torch.equal(s1[0], sums[2]) and int(c1[0]) == int(counts[2])


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_adjust_kernel_matches_the_float64_restatement(shape, margins):
    pred, gt = ref.inputs(*shape)
    tp, tg, sqerr = hip.relight_adjust(_t(pred), _t(gt), ref.GAINS)
    tp2, tg2, sqerr2 = hip.relight_adjust(_t(pred), _t(gt), ref.GAINS)
    wp, wg, _ = ref.adjust(pred, gt, ref.GAINS)
    gp, gg = tp.cpu().numpy(), tg.cpu().numpy()
    ep, eg = np.abs(gp - wp).max(), np.abs(gg - wg).max()
    d = gp - gg                                                     # the kernel's own fp32 terms, summed in float64
    terms = (d * d).astype(np.float64).sum(axis=(1, 2, 3))
    got = sqerr.cpu().numpy()
    print("adjust", shape, "max |tp - want|", ep, "margin", margins["tp"], "max |tg - want|", eg, "margin", margins["tg"],
          "sqerr relative distance", (np.abs(got - terms) / np.maximum(terms, 1e-300)).max())
    assert tp.shape == pred.shape and tg.shape == pred.shape and sqerr.dtype == torch.float64 and sqerr.shape == (shape[0],)
    assert gp.min() >= 0 and gp.max() <= 1 and gg.min() >= 0 and gg.max() <= 1
    assert ep <= margins["tp"] and eg <= margins["tg"]
    assert (np.abs(got - terms) <= 1e-12 * terms).all()
    assert torch.equal(tp, tp2) and torch.equal(tg, tg2) and torch.equal(sqerr, sqerr2)


def test_wrappers_refuse_what_the_kernels_must_not_see():
    pred, gt = (_t(a) for a in ref.inputs(1, 5, 7))
    for bad in (lambda: hip.relight_ratio(pred.double(), gt), lambda: hip.relight_ratio(pred, gt[..., :3].contiguous()),
                lambda: hip.relight_ratio(pred[:, :4], gt), lambda: hip.relight_adjust(pred, gt, (1.0, 2.0)),
                lambda: hip.relight_adjust(pred, gt, (1.0, float("nan"), 1.0)), lambda: hip.relight_frame(pred, gt[..., :2]),
                lambda: hip.relight_frame(pred.cpu(), gt[..., 3].contiguous())):
        with pytest.raises(hip.NmfHipError):
            bad()


# ---- rgb_lin out of the evaluation pass ---------------------------------------------------------------------------------------------
def test_rgb_lin_of_the_fused_pass_equals_the_module_path():
    """Tolerance: bit identity, as tests/test_hip_e2e.py::test_tape_free_evaluation_forward_equals_the_module compares rgb_map and acc_map
    of the two paths (the same kernels in the same order on the same noise stream; the forward has no atomics).  Asking for rgb_lin
    changes no bit of rgb_map."""
    from nmf_amd import renderer
    from nmf_amd.noise import DeviceNoise
    nerf, _ = _s1_model()
    r, focal = synthetic.orbit_rays(1, 32, seed=2)
    rays = r.reshape(-1, 6).to(DEV)
    keys = ("rgb_map", "acc_map", "rgb_lin")
    render = lambda k: renderer.render_images(nerf, rays, focal, noise=DeviceNoise(torch.device(DEV), seed=5), keys=k)    # noqa: E731
    fp = renderer._eval_pass(nerf)
    calls, orig = [], fp.render_chunk
    fp.render_chunk = lambda *a, **k: (calls.append(k), orig(*a, **k))[1]
    try:
        plain = render(("rgb_map", "acc_map"))
        fused = render(keys)
    finally:
        fp.render_chunk = orig
    assert len(calls) >= 2 and "want_linear" not in calls[0] and calls[-1].get("want_linear") is True       # the fused pass ran
    nerf.fused_eval_pass = False
    module = render(keys)
    assert fused["rgb_lin"].shape == (rays.shape[0], 3)
    assert torch.equal(fused["rgb_lin"], module["rgb_lin"])
    assert torch.equal(fused["rgb_map"], plain["rgb_map"]) and torch.equal(fused["acc_map"], plain["acc_map"])
    assert torch.equal(module["rgb_map"], plain["rgb_map"])
    # it is the radiance under the tonemap: rgb_map = clip(srgb(rgb_lin)) + (1 - acc) on the white background
    lin, acc = fused["rgb_lin"].double().cpu().numpy(), fused["acc_map"].double().cpu().numpy()
    want = ref.srgb(lin, np.float64, True) + (1 - acc)[:, None]
    assert np.abs(fused["rgb_map"].cpu().numpy() - want).max() <= 1e-6 and float(fused["rgb_lin"].std()) > 0.01


# ---- the command line -------------------------------------------------------------------------------------------------------------------
RES, VIEWS, ROT = 32, 3, ("40", "10", "0")


def _scene(root, frames_rgba):
    """an EXR test set of VIEWS views of RES x RES around the synthetic scene"""
    from nmf_amd import exr
    look_at = _load_tool("make_blender_scene").look_at_blender
    os.makedirs(os.path.join(root, "test"), exist_ok=True)
    frames = []
    for i, (phi, z) in enumerate(((0.3, 0.4), (2.4, 0.7), (4.5, 0.2))):
        rxy = np.sqrt(1 - z * z)
        frames.append({"file_path": f"./test/r_{i}", "transform_matrix": look_at(4.0 * np.array([rxy * np.cos(phi), rxy * np.sin(phi), z])).tolist()})
        exr.imwrite(os.path.join(root, "test", f"r_{i}.exr"), frames_rgba[i])
    with open(os.path.join(root, "transforms_test.json"), "w") as f:
        json.dump({"camera_angle_x": 0.6911112070083618, "w": RES, "h": RES, "ext": ".exr", "near_far": [2.5, 7.0], "frames": frames}, f)
    return root


def test_render_relight_eval_recovers_a_known_multiplier(tmp_path, capsys):
    """the model's own relit frames scaled by g = (0.5, 1, 2) per channel as ground truth: the fit returns g (each ratio is
    fl(g p) / p, one ulp from g, averaged in double) and the adjusted frames agree with the ground truth"""
    from PIL import Image
    from nmf_amd import exr
    from nmf_amd import render as Rn
    nerf, cfg = _s1_model()
    ck = str(tmp_path / "m.th")
    nerf.save(ck, cfg["arch"])
    del nerf
    cli = lambda scene, *more: Rn.main(["--ckpt", ck, "--datadir", scene, "--env-rotate", *ROT, *more])     # noqa: E731
    # 1. the relit views themselves, twice: a placeholder ground truth (grey, opaque) gives the loader its frames
    grey = np.full((VIEWS, RES, RES, 4), 0.5, dtype=np.float32)
    grey[..., 3] = 1.0
    draft = _scene(str(tmp_path / "draft"), grey)
    plain = cli(draft)
    first = cli(draft, "--relight-eval", str(tmp_path / "a"))
    second = cli(draft, "--relight-eval", str(tmp_path / "b"))
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 3 and lines[1] == json.loads(json.dumps(first))
    hdr = np.stack([exr.imread(str(tmp_path / "a" / f"{i:03d}.exr")) for i in range(VIEWS)])
    again = np.stack([exr.imread(str(tmp_path / "b" / f"{i:03d}.exr")) for i in range(VIEWS)])
    assert hdr.shape == (VIEWS, RES, RES, 3) and hdr.dtype == np.float32 and np.isfinite(hdr).all()
    assert np.array_equal(hdr, again) and first["relight"] == second["relight"]                 # two renders: bit-identical
    # without the flag: the keys of the parent commit's line, and nothing written
    assert set(plain) == {"frames", "width", "height", "chunk", "seconds", "rays_per_s", "relit", "psnr"}
    assert set(first) == set(plain) | {"relight"} and set(first["relight"]) == {"psnr", "ssim", "multiplier", "views"}
    # 2. the opacity of those views: the command's own sequence of renders on the same noise seed (warm-up, the frames, then
    # rgb_lin / acc_map per view), checked against the frames it wrote
    acc = _replay_acc(ck, draft, hdr)
    a = (acc > 0.5).astype(np.float32)
    assert 0.05 < a.mean() < 0.95
    g = np.asarray(ref.GAINS, dtype=np.float32)
    gt = np.concatenate([g * hdr * a[..., None], a[..., None]], axis=-1).astype(np.float32)
    scene = _scene(str(tmp_path / "scene"), gt)
    out = tmp_path / "imgs_test_ori"
    rec = cli(scene, "--relight-eval", str(out))
    rl = rec["relight"]
    print("multiplier", rl["multiplier"], "relative distance from g", (np.abs(np.array(rl["multiplier"]) / g - 1)).tolist(),
          "psnr", rl["psnr"], "ssim", rl["ssim"])
    assert np.array_equal(np.stack([exr.imread(str(out / f"{i:03d}.exr")) for i in range(VIEWS)]), hdr)
    assert (np.abs(np.array(rl["multiplier"]) / g - 1) <= 1e-6).all()
    assert rl["psnr"] >= 90 and rl["ssim"] > 0.9999 and rl["views"] == VIEWS
    # the files of the protocol
    import yaml
    stats = yaml.safe_load(open(out / "stats.yaml"))
    assert set(stats) == {"psnr", "ssim", "lpips", "multiplier", "views"} and np.isnan(stats["lpips"]) and stats["views"] == VIEWS
    # (g is made of powers of two, so fl(g p) / p is g itself and the error may be exactly zero: an infinite PSNR)
    assert stats["multiplier"] == rl["multiplier"] and (stats["psnr"] == rl["psnr"] or abs(stats["psnr"] - rl["psnr"]) < 1e-3)
    _, _, tp, _ = ref.protocol(hdr, gt)
    multi = ref.multiplier(*ref.ratio(hdr, gt, np.float32))                       # the kernel's fp32 quotients, summed in float64
    assert np.abs(multi / np.array(rl["multiplier"]) - 1).max() <= 1e-12
    for i in range(VIEWS):
        png = np.asarray(Image.open(out / "adjusted" / f"{i:03d}.png"))
        assert png.shape == (RES, RES, 3) and png.dtype == np.uint8
        assert np.abs(png.astype(np.int64) - (tp[i] * 255).astype(np.int64)).max() <= 1          # truncation next to an fp32 / float64 edge
    assert not os.path.exists(out / f"{VIEWS:03d}.exr")


def _replay_acc(ck, scene, hdr):
    """acc_map of the views `render --relight-eval` renders, by the calls nmf_amd/render.py:main makes; the HDR frames it forms must
    equal the ones the command wrote (`hdr`)"""
    from nmf_amd import render as Rn
    from nmf_amd.dataLoader import BlenderDataset
    from nmf_amd.modules.tensor_nerf import TensorNeRF
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import render_images
    dev = torch.device(DEV, 0)
    ds = BlenderDataset(scene, split="test", is_stack=True, N_vis=-1)
    rays, focal = ds.all_rays.to(dev), float(ds.fx)
    nerf = TensorNeRF.load(ck, near_far=list(ds.near_far), device=dev)
    nerf.bg_module = relight.rotate_env(nerf.bg_module, relight.rotation(*[float(v) for v in ROT]))
    nerf.eval()
    chunk, noise = nerf.eval_batch_size, DeviceNoise(dev, seed=11)
    Rn.render_frames(nerf, rays[:1, : min(chunk, rays.shape[1])], focal, chunk, noise)
    Rn.render_frames(nerf, rays, focal, chunk, noise)
    accs = []
    for i in range(VIEWS):
        ims = render_images(nerf, rays[i], focal, chunk, noise, keys=("rgb_lin", "acc_map"))
        frame = hip.relight_frame(ims["rgb_lin"].reshape(RES, RES, 3), ims["acc_map"].reshape(RES, RES))
        assert np.array_equal(frame.cpu().numpy(), hdr[i]), i
        accs.append(ims["acc_map"].reshape(RES, RES).cpu().numpy())
    return np.stack(accs)
