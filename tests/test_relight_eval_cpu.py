"""Relighting evaluation, the parts that need no GPU: EXR frames through the Blender loader, the float64 restatement of the notebook
protocol (tests/relight_eval_ref.py) on cases with known answers, the host rules of nmf_amd/relight_eval.py, and the argument checks
of the three entry points of csrc/relight_eval.hip (the library loads without a GPU)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import relight_eval_ref as ref

H, W, VIEWS = 5, 7, 3


def _exr_scene(root, channels=4):
    """3 views of 7 x 5 linear RGBA: alphas 0, 1 and fractions; colours from 1e-4 to 30 (above 1: clipped by the tonemap) and on both
    sides of the sRGB limit"""
    from nmf_amd import exr
    rng = np.random.default_rng(3)
    pose = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4], [0, 0, 0, 1]]
    frames, imgs = [], []
    for split in ("train", "test"):
        os.makedirs(os.path.join(root, split), exist_ok=True)
    for i in range(VIEWS):
        rgba = np.exp(rng.uniform(np.log(1e-4), np.log(30.0), size=(H, W, 4))).astype(np.float32)
        rgba[..., 3] = rng.uniform(size=(H, W))
        rgba[0, :, 3] = 0.0
        rgba[1, :, 3] = 1.0
        rgba[1, :3, 0] = (0.0031308 * 0.999, 0.0031308 * 1.001, 0.0)
        rgba[2, 0, :3] = (1.0, 4.0, 12.5)
        for split in ("train", "test"):
            exr.imwrite(os.path.join(root, split, f"r_{i}.exr"), rgba[..., :channels])
        imgs.append(rgba)
        frames.append({"file_path": f"./{{split}}/r_{i}", "transform_matrix": pose})
    for split in ("train", "test"):
        meta = {"camera_angle_x": 0.6, "w": W, "h": H, "ext": ".exr",
                "frames": [dict(f, file_path=f["file_path"].format(split=split)) for f in frames]}
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump(meta, f)
    return np.stack(imgs)


def _within_ulps(got, want64, ulps):
    want32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) <= ulps * np.spacing(np.abs(want32)).astype(np.float64)


def test_exr_scene_loads_blended_then_tonemapped(tmp_path):
    """reference dataLoader/blender.py:159-188: alpha to acc_maps, a testing split blended onto white, THEN the tonemap with its clip,
    hdr set; get_linear returns the stored floats; EXR frames are not resampled.  (The parent commit raised NotImplementedError.)"""
    from nmf_amd.dataLoader import BlenderDataset
    stored = _exr_scene(str(tmp_path))
    rgb, a = stored[..., :3].astype(np.float64), stored[..., 3:].astype(np.float64)
    train = BlenderDataset(str(tmp_path), split="train", is_stack=False)
    assert train.hdr is True and train.img_wh == [W, H]
    assert train.all_rgbs.shape == (VIEWS * H * W, 4) and train.all_rgbs.dtype == torch.float32
    got = train.all_rgbs.numpy().reshape(VIEWS, H, W, 4)
    want = ref.srgb(rgb, np.float64, True)                                        # no blend on a training split
    assert _within_ulps(got[..., :3], want, 2).all(), np.abs(got[..., :3] - want).max()
    assert np.array_equal(got[..., 3], stored[..., 3])
    assert len(train.acc_maps) == VIEWS and np.array_equal(train.acc_maps[1].numpy(), stored[1, ..., 3])
    test = BlenderDataset(str(tmp_path), split="test", is_stack=True)
    assert test.hdr is True and test.all_rgbs.shape == (VIEWS, H, W, 3) and test.all_rays.shape == (VIEWS, H * W, 6)
    want = ref.srgb(rgb * a + (1 - a), np.float64, True)
    got = test.all_rgbs.numpy()
    assert _within_ulps(got, want, 2).all(), np.abs(got - want).max()
    assert got.max() == 1.0 and (got[:, 2, 0, 1:] == 1.0).all()                    # values above 1 end at the clip
    assert float(np.abs(got - ref.srgb(rgb, np.float64, True) * a - (1 - a)).max()) > 1e-2      # (tonemap-then-blend is another image)
    for ds in (train, test):
        for i in range(VIEWS):
            lin = ds.get_linear(i)
            assert lin.dtype == torch.float32 and np.array_equal(lin.numpy(), stored[i])
    one = BlenderDataset(str(tmp_path), split="test", is_stack=True, N_vis=1)
    assert one.all_rays.shape[0] == 1 and np.array_equal(one.get_linear(0).numpy(), stored[0])
    with pytest.raises(ValueError, match="downsample"):
        BlenderDataset(str(tmp_path), split="test", is_stack=True, downsample=2)


def test_png_scenes_have_no_linear_frames(tmp_path):
    from PIL import Image
    from nmf_amd.dataLoader import BlenderDataset
    os.makedirs(tmp_path / "test")
    Image.fromarray(np.full((H, W, 4), 128, dtype=np.uint8), "RGBA").save(tmp_path / "test" / "r_0.png")
    meta = {"camera_angle_x": 0.6, "w": W, "h": H, "frames": [{"file_path": "./test/r_0", "transform_matrix": np.eye(4).tolist()}]}
    with open(tmp_path / "transforms_test.json", "w") as f:
        json.dump(meta, f)
    ds = BlenderDataset(str(tmp_path), split="test", is_stack=True)
    assert ds.hdr is False
    with pytest.raises(ValueError):
        ds.get_linear(0)


# ---- the float64 restatement on cases with known answers ------------------------------------------------------------------------------
def test_restatement_special_pixels_and_known_answers():
    pred, gt = ref.inputs(3, 5, 7)
    m = ref.mask(pred, gt)[0].reshape(-1)
    for k, (_, _, inside) in enumerate(ref.SPECIAL):
        assert bool(m[k]) is inside, k
    sums, counts = ref.ratio(pred, gt)
    assert counts[1] == 0 and (sums[1] == 0).all() and counts[0] > 0 and counts[2] > 0
    # a prediction that is the ground truth divided by g: the multiplier is g, the adjusted frames agree
    rng = np.random.default_rng(5)
    g = np.array(ref.GAINS)
    p = np.exp(rng.uniform(np.log(0.02), np.log(8.0), size=(2, 6, 4, 3)))
    a = (rng.uniform(size=(2, 6, 4, 1)) > 0.3).astype(np.float64)
    multi, psnrs, tp, tg = ref.protocol(p, np.concatenate([p * g * a, a], axis=-1))
    assert np.allclose(multi, g, rtol=1e-14) and (psnrs > 250).all() and np.allclose(tp, tg, atol=1e-14)
    # the sRGB pair: inverse of forward, the two limits, the published mid-grey
    x = np.array([0.0, 0.001, 0.0031308, 0.01, 0.18, 1.0, 7.5])
    assert np.allclose(ref.srgb_inverse(ref.srgb(x, np.float64, False), np.float64), x, rtol=1e-4, atol=1e-9)
    assert abs(float(ref.srgb(0.0031308, np.float64, False)) - 0.04045) < 1e-6
    assert abs(float(ref.srgb(0.2140, np.float64, True)) - 0.5) < 1e-3 and float(ref.srgb(7.5, np.float64, True)) == 1.0
    # the frame: opaque -> the radiance itself; empty -> white
    lin = np.array([[0.25, 2.0, 0.001]])
    assert np.allclose(ref.frame(lin, np.array([1.0])), lin, rtol=1e-12)
    assert np.allclose(ref.frame(np.zeros((1, 3)), np.array([0.0])), 1.0, rtol=1e-12)
    mg = ref.margins()
    assert all(1e-8 < v < 1e-5 for v in mg.values()), mg                          # fp32-sized, and not zero


# ---- host rules of the protocol ---------------------------------------------------------------------------------------------------------
def test_empty_images_are_left_out_and_an_empty_set_raises():
    from nmf_amd.relight_eval import fit_multiplier, psnr_from_sqerr
    sums = np.array([[2.0, 4.0, 8.0], [0.0, 0.0, 0.0], [9.0, 3.0, 6.0]])
    counts = np.array([2, 0, 3])
    multi, means = fit_multiplier(sums, counts)
    assert np.array_equal(multi, (np.array([1.0, 2.0, 4.0]) + np.array([3.0, 1.0, 2.0])) / 2)
    assert np.isnan(means[1]).all() and np.array_equal(means[0], [1.0, 2.0, 4.0])
    assert np.array_equal(multi, ref.multiplier(sums, counts))
    with pytest.raises(ValueError, match="multiplier"):
        fit_multiplier(np.zeros((2, 3)), np.zeros(2, dtype=np.int64))
    assert np.allclose(psnr_from_sqerr([3e-4 * 35], 35), 40.0)
    pred, gt = ref.inputs(3, 5, 7)
    s, c = ref.ratio(pred, gt)
    assert np.array_equal(fit_multiplier(s, c)[0], ref.multiplier(s, c))


# ---- entry points refuse bad arguments on the host --------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    i64, f32, vp = C.c_int64, C.c_float, C.c_void_p
    for name in ("nmf_relight_ratio_workspace_bytes", "nmf_relight_adjust_workspace_bytes"):
        getattr(lib, name).restype = C.c_int64
        getattr(lib, name).argtypes = [i64, i64, i64]
    lib.nmf_relight_frame.argtypes = [vp, vp, i64, i64, i64, vp, vp]
    lib.nmf_relight_ratio.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, i64, vp]
    lib.nmf_relight_adjust.argtypes = [vp, vp, f32, f32, f32, i64, i64, i64, vp, vp, vp, vp, i64, vp]
    # workspace sizes are host arithmetic: one partial of 4 (ratio) or 1 (adjust) doubles per workgroup of 2048 pixels
    for n, h, w in ((1, 1, 1), (3, 5, 7), (3, 33, 67), (200, 800, 800)):
        blocks = n * -(-(h * w) // 2048)
        assert lib.nmf_relight_ratio_workspace_bytes(n, h, w) == blocks * 32
        assert lib.nmf_relight_adjust_workspace_bytes(n, h, w) == blocks * 8
    assert lib.nmf_relight_ratio_workspace_bytes(0, 5, 7) == lib.nmf_relight_adjust_workspace_bytes(3, 0, 7) == 0
    p = 4096                                                        # (a non-null, 16-byte aligned address: never dereferenced)
    frame = lambda a=p, b=p, n=3, h=5, w=7, o=p: lib.nmf_relight_frame(a, b, n, h, w, o, None)                      # noqa: E731
    ratio = lambda a=p, b=p, n=3, h=5, w=7, s=p, c=p, ws=p, nb=96: lib.nmf_relight_ratio(a, b, n, h, w, s, c, ws, nb, None)   # noqa: E731
    adjust = lambda a=p, b=p, m=(1.0, 1.0, 1.0), n=3, h=5, w=7, tp=p, tg=p, e=p, ws=p, nb=24: \
        lib.nmf_relight_adjust(a, b, *m, n, h, w, tp, tg, e, ws, nb, None)                                          # noqa: E731
    EINVAL, ERANGE = -1, -2
    bad = [
        (lambda: frame(a=None), EINVAL, b"null"), (lambda: frame(b=None), EINVAL, b"null"), (lambda: frame(o=None), EINVAL, b"null"),
        (lambda: frame(n=0), EINVAL, b"at least 1"), (lambda: frame(h=0), EINVAL, b"at least 1"), (lambda: frame(w=-3), EINVAL, b"at least 1"),
        (lambda: frame(n=1 << 20, h=1 << 20, w=1 << 20), ERANGE, b"too many"),
        (lambda: ratio(a=None), EINVAL, b"null"), (lambda: ratio(b=None), EINVAL, b"null"), (lambda: ratio(s=None), EINVAL, b"null"),
        (lambda: ratio(c=None), EINVAL, b"null"), (lambda: ratio(ws=None), EINVAL, b"null"),
        (lambda: ratio(n=0), EINVAL, b"at least 1"), (lambda: ratio(h=0), EINVAL, b"at least 1"), (lambda: ratio(w=0), EINVAL, b"at least 1"),
        (lambda: ratio(nb=95), EINVAL, b"workspace too small"), (lambda: ratio(b=p + 4), EINVAL, b"aligned"), (lambda: ratio(ws=p + 8), EINVAL, b"aligned"),
        (lambda: ratio(n=1 << 22, h=1 << 12, w=1 << 12, nb=1 << 40), ERANGE, b"too many"),
        (lambda: adjust(a=None), EINVAL, b"null"), (lambda: adjust(b=None), EINVAL, b"null"), (lambda: adjust(tp=None), EINVAL, b"null"),
        (lambda: adjust(tg=None), EINVAL, b"null"), (lambda: adjust(e=None), EINVAL, b"null"), (lambda: adjust(ws=None), EINVAL, b"null"),
        (lambda: adjust(n=0), EINVAL, b"at least 1"), (lambda: adjust(h=-1), EINVAL, b"at least 1"), (lambda: adjust(w=0), EINVAL, b"at least 1"),
        (lambda: adjust(nb=23), EINVAL, b"workspace too small"), (lambda: adjust(b=p + 8), EINVAL, b"aligned"),
        (lambda: adjust(m=(1.0, float("nan"), 1.0)), EINVAL, b"not finite"), (lambda: adjust(m=(float("inf"), 1.0, 1.0)), EINVAL, b"not finite"),
        (lambda: adjust(m=(1.0, 1.0, float("-inf"))), EINVAL, b"not finite"),
    ]
    for call, code, word in bad:
        assert call() == code, (code, word)
        msg = lib.nmf_last_error_string()
        assert word in msg and b"nmf_relight_" in msg, msg


def test_wrappers_have_no_cpu_path():
    from nmf_amd import hip
    pred, gt = ref.inputs(1, 5, 7)
    with pytest.raises(hip.NmfHipError):
        hip.relight_ratio(torch.from_numpy(pred), torch.from_numpy(gt))
    with pytest.raises(hip.NmfHipError):
        hip.relight_adjust(torch.from_numpy(pred), torch.from_numpy(gt), (1.0, 1.0, 1.0))
    with pytest.raises(hip.NmfHipError):
        hip.relight_frame(torch.from_numpy(pred), torch.from_numpy(gt[..., 3].copy()))
    with pytest.raises(hip.NmfHipError):
        hip.relight_ratio(torch.from_numpy(pred), torch.from_numpy(gt[..., :3].copy()))             # gt must be RGBA
