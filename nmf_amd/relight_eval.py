"""Relighting evaluation against ground truth -- the protocol of the reference's scripts/relighting_calc.ipynb on the frames its
renderer.py:425-429 stores for an HDR test set.

The test views of a `relighting/<scene>_exr` set are rendered under the new environment map in linear radiance (render_images'
"rgb_lin"), each becomes the HDR frame srgb_inverse(srgb_noclip(rgb_lin) + (1 - acc)) (nmf_relight_frame) and is written as
{idx:03d}.exr.  One brightness multiplier per channel is fitted over the whole set (cell lines 230-234): per view the mean of
gt / max(pred, 1e-7) over the pixels with gt alpha > 0.5 and min_c pred_c > 0.01 (nmf_relight_ratio), then the mean of those means.
Each view is then scaled, blended onto white with the ground-truth alpha, tonemapped and clipped, as is the ground truth (cell lines
243-246, nmf_relight_adjust); PSNR and SSIM (nmf_ssim) are taken between the two and averaged.

Deviation: a view whose mask is empty is left out of the multiplier (the notebook's numpy mean of an empty selection is NaN and
poisons the whole set); a set without any masked pixel raises ValueError.  LPIPS is not computed (`lpips: nan` in stats.yaml).
"""
import os
import time

import numpy as np
import torch

DEVICE_FRAME_BYTES = 4 << 30          # frames and ground truth stay on the device up to this size (200 views of 800 x 800: 3.6 GB)


def fit_multiplier(sums, counts):
    """sums [n,3] and counts [n] of nmf_relight_ratio -> (multi float64 [3], per-view means [n,3] with NaN rows for empty masks): the
    mean over the views with count > 0 of sum / count.  ValueError when no view has a masked pixel."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    means = np.full(sums.shape, np.nan)
    used = counts > 0
    if not used.any():
        raise ValueError("relighting evaluation: no view has a pixel with ground-truth alpha > 0.5 and a prediction above 0.01 "
                         "in every channel, so no brightness multiplier can be fitted")
    means[used] = sums[used] / counts[used, None]
    return means[used].mean(axis=0), means


def psnr_from_sqerr(sqerr, n_px):
    """-10 log10 of the mean squared error over n_px pixels of 3 channels (cell lines 253-254); inf for identical frames"""
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(np.asarray(sqerr, dtype=np.float64) / (3.0 * n_px))


@torch.no_grad()
def relight_evaluation(nerf, test_dataset, save_path, noise=None, chunk=None, spp=1, min_spp=4, tol=None, denoise=None):
    """Evaluate `nerf` (its bg_module already the new lighting) on the stacked EXR test set `test_dataset`.  Writes
    {save_path}/{idx:03d}.exr (the HDR frames), adjusted/{idx:03d}.png (the scaled, tonemapped predictions, truncated to 8 bits) and
    stats.yaml (psnr, ssim, lpips: nan, multiplier, views).  spp > 1: the radiance and acc of a view are multisample.render_frame's
    means of up to spp passes through the data set's rays (min_spp, tol: its adaptive stop); denoise: a multisample.DenoiseParams, the
    radiance is then the filtered one (needs spp >= 2; the coverage stays the measured mean).
    -> dict(psnrs, ssims, psnr, ssim, multiplier [3], counts, views, seconds=dict(render, metrics))"""
    from . import exr, hip
    from .renderer import _png, map_to_8bit, render_images
    if not getattr(test_dataset, "hdr", False):
        raise ValueError("relighting evaluation needs an EXR test set (linear ground truth with alpha)")
    W, H = test_dataset.img_wh
    focal = float(test_dataset.fx)
    if denoise is not None and int(spp) < 2:
        raise ValueError(f"relight_evaluation: denoise needs spp >= 2, got spp = {spp}")
    rays_all = test_dataset.all_rays
    if rays_all.dim() != 3:
        raise ValueError("relighting evaluation needs a stacked test set (is_stack=True)")
    n = rays_all.shape[0]
    dev = next(nerf.parameters()).device
    os.makedirs(os.path.join(save_path, "adjusted"), exist_ok=True)
    on_device = n * H * W * 7 * 4 <= DEVICE_FRAME_BYTES
    frames, gts = [], []

    def frame_of(i):
        return frames[i] if on_device else torch.from_numpy(exr.imread(os.path.join(save_path, f"{i:03d}.exr"))[..., :3].copy()).to(dev)

    def gt_of(i):
        g = gts[i] if on_device and i < len(gts) else test_dataset.get_linear(i).to(dev)
        if g.shape != (H, W, 4):
            raise ValueError(f"relighting evaluation: view {i} is {tuple(g.shape)}, expected RGBA of {H} x {W}")
        if on_device and i == len(gts):
            gts.append(g)
        return g

    was_training = nerf.training
    nerf.eval()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(n):
        view = rays_all[i].reshape(-1, rays_all.shape[-1]).to(dev)
        if int(spp) > 1:
            from .multisample import render_frame
            ims, _ = render_frame(nerf, view, focal, spp=spp, min_spp=min_spp, tol=tol, jitter=False, noise=noise, chunk=chunk,
                                  keys=("rgb_lin", "acc_map"), denoise=denoise, frame_hw=(H, W) if denoise is not None else None)
        else:
            ims = render_images(nerf, view, focal, chunk, noise, keys=("rgb_lin", "acc_map"))
        frame = hip.relight_frame(ims["rgb_lin"].reshape(H, W, 3), ims["acc_map"].reshape(H, W))
        exr.imwrite(os.path.join(save_path, f"{i:03d}.exr"), frame.cpu().numpy())
        if on_device:
            frames.append(frame)
    nerf.train(was_training)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()

    sums, counts = [], []
    for i in range(n):
        s, c = hip.relight_ratio(frame_of(i), gt_of(i))
        sums.append(s)
        counts.append(c)
    sums, counts = torch.cat(sums).cpu().numpy(), torch.cat(counts).cpu().numpy()
    multi, _ = fit_multiplier(sums, counts)
    psnrs, ssims = [], []
    for i in range(n):
        tp, tg, sqerr = hip.relight_adjust(frame_of(i), gt_of(i), multi)
        ssims.append(hip.ssim(tp, tg, max_val=1.0))
        psnrs.append(sqerr)
        _png(os.path.join(save_path, "adjusted", f"{i:03d}.png"), map_to_8bit(tp.cpu().numpy()))
    psnrs = [float(v) for v in psnr_from_sqerr(torch.cat(psnrs).cpu().numpy(), H * W)]
    ssims = [float(v) for v in torch.cat(ssims).cpu().numpy()]
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    res = dict(psnrs=psnrs, ssims=ssims, psnr=float(np.mean(psnrs)), ssim=float(np.mean(ssims)), multiplier=[float(v) for v in multi],
               counts=[int(c) for c in counts], views=n, seconds=dict(render=t1 - t0, metrics=t2 - t1))
    import yaml
    with open(os.path.join(save_path, "stats.yaml"), "w") as f:
        yaml.dump(dict(psnr=res["psnr"], ssim=res["ssim"], lpips=float("nan"), multiplier=res["multiplier"], views=n), f)
    return res
