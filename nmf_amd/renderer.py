"""Chunked rendering -- counterpart of the reference's renderer.py: `chunk_renderer` (:56-106, the callable train.py:541
and BundleRender use), the evaluation PSNR (:399-401, :511-513) and the test-set evaluation `evaluation` / `evaluate`
(:195-560: PSNR, SSIM and normal error per view, frames and mean.txt / stats.yaml), and the camera-path render `evaluation_path`
(:564-582: views that are in no data set, rays and 8-bit frames made on the device, PNGs on a writer thread)."""
import os
import time
from collections import defaultdict

import numpy as np
import torch


def _stack(d):
    out = {}
    for k, v in d.items():
        if isinstance(v[0], torch.Tensor):
            out[k] = torch.cat([t if t.dim() > 0 else t.reshape(1) for t in v], 0)
        else:
            out[k] = v
    return out


def chunk_renderer(rays, tensorf, focal, keys=("rgb_map",), chunk=4096, render2completion=False, **kwargs):
    """renderer.py:56-106.  Rays are rendered `chunk` at a time; with render2completion every chunk is re-submitted with
    the rays the sampler's sample budget cut off (`~whole_valid`, samplers/alphagrid.py:353-364) until none is left, so the
    concatenated outputs cover every ray exactly once, in submission order per round.  Returns (images, stats): tensors of
    the requested keys concatenated over the calls (keys=None: everything the module returns)."""
    ims, stats = defaultdict(list), defaultdict(list)
    n_all = rays.shape[0]
    for start in range(0, n_all, chunk):
        rays_chunk = rays[start:start + chunk]
        if rays_chunk.numel() == 0:
            continue
        pending = rays_chunk
        while pending.shape[0] > 0:
            cims, cstats = tensorf(pending, focal, **kwargs)
            for src, dst in ((cims, ims), (cstats, stats)):
                for key in (keys if keys is not None else list(src.keys())):
                    if key in src:
                        dst[key].append(src[key])
            if not render2completion:
                break
            kept = cstats.get("rays_kept")
            if kept is None:                                   # a module without the host-side count: one read-back
                wv = cstats["whole_valid"]
                pending = pending[~wv]
            elif kept >= pending.shape[0]:
                break
            else:                                              # valid rays are a prefix (cumsum < budget)
                if kept == 0:
                    raise RuntimeError("render2completion: the sample budget admits no ray of this chunk")
                pending = pending[kept:]
    return _stack(ims), _stack(stats)


def psnr_8bit(pred, gt):
    """renderer.py:399-401: the prediction is quantised to 8 bits (floor) before the error is taken"""
    q = torch.floor(pred.clip(0, 1) * 255) / 255
    return -10.0 * torch.log10(((q - gt.clip(0, 1)) ** 2).mean())


@torch.no_grad()
def render_images(nerf, rays, focal, chunk=None, noise=None, keys=("rgb_map",), **kw):
    """evaluation render (renderer.py:119-170 without the random permutation): eval_batch_size rays per chunk, rendered
    to completion, is_train=False.  keys may name the material maps MATERIAL_KEYS (renderer.py:440-463, [N,3] each): the fused
    pass forms them (TrainPass.render_chunk(want_materials=True)); without it the whole call renders through the module with
    draw_debug=True, and a chunk the fused pass does not support through the module with draw_debug=True.  "rgb_lin" [N,3] is the
    composited radiance sum_k w_k c_k before tonemap, clip and background (the relighting evaluation's input): the buffer the compose
    kernel writes next to acc_map, handed out by the fused pass (want_linear) and by the module alike."""
    chunk = chunk or nerf.eval_batch_size
    kw.setdefault("draw_debug", False)
    module_kw = dict(bg_col=torch.ones(3, device=rays.device), is_train=False, ndc_ray=False, noise=noise, **kw)
    tensorf = nerf
    maps = bool(set(keys) & {"depth", "world_normal"})
    mats = bool(set(keys) & set(MATERIAL_KEYS))
    lin = "rgb_lin" in keys
    fast = _eval_pass(nerf) if (rays.is_cuda and not kw["draw_debug"]
                                and set(keys) <= {"rgb_map", "acc_map", "depth", "world_normal", "rgb_lin", *(MATERIAL_KEYS if mats else ())}
                                and len(kw) == 1) else None
    if mats and fast is None:
        module_kw["draw_debug"] = True            # the module's evaluation branch forms the maps (modules/tensor_nerf.py:480-566)
    if fast is not None:
        from .fast_step import Unsupported

        def tensorf(pending, focal_, **_kw):          # noqa: F811 -- the straight-line forward, the module as its fallback
            try:
                nz = noise
                if nz is None:                        # the module's own generator (tensor_nerf.py: _render)
                    if nerf._noise is None:
                        from .noise import DeviceNoise
                        nerf._noise = DeviceNoise(pending.device, seed=20211200)
                    nz = nerf._noise
                out = fast.render_chunk(pending, focal_, nz, want_maps=maps, **(dict(want_materials=True) if mats else {}),
                                        **(dict(want_linear=True) if lin else {}))
            except Unsupported:
                return nerf(pending, focal_, **(dict(module_kw, draw_debug=True) if (maps or mats) else module_kw))
            ims_ = dict(rgb_map=out[0], acc_map=out[1])
            if maps:
                ims_.update(depth=out[4], world_normal=out[5])
            if lin:
                ims_.update(rgb_lin=out[-1])
            if mats:
                ims_.update(out[-2 if lin else -1])
            return ims_, dict(rays_kept=out[2], n_samples=out[3])
    ims, _ = chunk_renderer(rays, tensorf, focal, keys=keys, chunk=chunk, render2completion=True, **module_kw)
    return ims["rgb_map"] if tuple(keys) == ("rgb_map",) else ims


MATERIAL_KEYS = ("albedo", "roughness", "diffuse", "tint", "spec")


def _eval_pass(nerf):
    """the C++ pass of nmf_amd/fast_step.py, forward only (nerf.fused_eval_pass = False: always the module path)"""
    if not getattr(nerf, "fused_eval_pass", True):
        return None
    fp = getattr(nerf, "_fused_pass", None)
    if fp is None:
        from .fast_step import TrainPass
        fp = TrainPass(nerf)
        if hasattr(nerf, "_fused_pass"):
            nerf._fused_pass = fp
        else:
            object.__setattr__(nerf, "_fused_pass", fp)
    return fp if fp.supported() else None


def _png(path, arr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(arr)).save(path)


def map_to_8bit(x):
    """the reference's 8-bit conversion of a map in [0, 1] (renderer.py:440-463: (255 * x).astype(uint8), a truncation), clipped to
    [0, 1] first: astype(uint8) wraps a value outside [0, 255] around (a spec-heavy tint above 1 would come out dark)"""
    return (np.clip(np.asarray(x, dtype=np.float32), 0.0, 1.0) * 255).astype(np.uint8)


MATERIAL_DIRS = ("albedo", "roughness", "tint", "diffuse", "spec", "rgbd")


SAMPLE_DIRS = ("spp", "noise")


def write_sample_maps(savePath, name, ims, H, W):
    """the two pictures a multi-sample frame adds (multisample.render_frame's count and se): spp/ the sample count over the frame's
    largest, grey; noise/ the standard error of the displayed colour with 8 / 255 (eight 8-bit levels) as white, both through map_to_8bit"""
    count, se = ims["count"].reshape(H, W), ims["se"].reshape(H, W)
    grey = lambda t: np.repeat(map_to_8bit(t.cpu().numpy())[..., None], 3, -1)      # noqa: E731
    _png(os.path.join(savePath, "spp", name + ".png"), grey(count / count.max().clamp(min=1.0)))
    _png(os.path.join(savePath, "noise", name + ".png"), grey(se * (255.0 / 8.0)))


def write_material_maps(savePath, name, ims, H, W):
    """renderer.py:433-463 for the material maps: albedo/, roughness/, tint/, diffuse/ 8-bit PNGs (map_to_8bit), spec/ and rgbd/
    (depth) float EXRs (nmf_amd/exr.py)"""
    from . import exr
    for key in ("albedo", "roughness", "tint", "diffuse"):
        _png(os.path.join(savePath, key, name + ".png"), map_to_8bit(ims[key].reshape(H, W, 3).cpu().numpy()))
    exr.imwrite(os.path.join(savePath, "spec", name + ".exr"), ims["spec"].reshape(H, W, 3).cpu().numpy())
    exr.imwrite(os.path.join(savePath, "rgbd", name + ".exr"), ims["depth"].reshape(H, W).cpu().numpy())


@torch.no_grad()
def evaluate(iterator, test_dataset, tensorf, renderer, savePath=None, prtx="", N_samples=-1, white_bg=False, ndc_ray=False,
             compute_extra_metrics=True, device="cuda", noise=None, material_maps=False, spp=1, min_spp=4, tol=None, denoise=None, **kw):
    """renderer.py:195-510 for the outputs the fused eval pass produces.  Per view of `iterator()` ((idx, im_idx, rays,
    gt_rgb [H,W,3] or None)): PSNR of the 8-bit prediction (psnr_8bit), with compute_extra_metrics its SSIM against the
    unclipped ground truth (renderer.py:403-404, nmf_ssim), and the normal error (renderer.py:357-390, nmf_normal_err) when
    the data set has a normal map for the view.  Writes {prtx}{idx:03d}.png, world_normal/, acc_map/ and err/ PNGs with the
    reference's 8-bit conversions, {prtx}mean.txt ([psnr, ssim, nan, nan]: LPIPS is not computed; [psnr] without extra
    metrics) and stats{prtx}.yaml (psnr, ssim, norm_err).  LPIPS, videos, the EXR frame and normal/ are not produced.
    `renderer`, `N_samples` and `white_bg` are accepted for the reference's call shape (the model's own background and
    sample budget are used).  material_maps: each view also renders depth and the material maps (render_images' MATERIAL_KEYS)
    and writes albedo/, roughness/, tint/, diffuse/ PNGs (map_to_8bit: the reference's truncation, clipped to [0, 1] first where
    its astype(uint8) would wrap), spec/ and rgbd/ (depth) EXRs, renderer.py:433-463.
    spp > 1: every view is multisample.render_frame's mean of up to spp passes (min_spp, tol: its adaptive stop; the rays stay the data
    set's, through the pixel centres, which the scores are defined on) and spp/, noise/ PNGs are written (write_sample_maps); spp = 1 is
    the single pass as before.  The material maps are not accumulated.  denoise: a multisample.DenoiseParams -- the view's rgb is the
    filtered frame (the data set's image size is the frame's shape; needs spp >= 2); noise/ keeps the measured standard error.
    -> dict(psnrs, norm_errs, ssims, seconds=dict(render, metrics))."""
    from . import hip
    if ndc_ray:
        raise NotImplementedError("evaluation: ndc rays are not used by model=microfacet_tensorf2")
    W, H = test_dataset.img_wh
    focal = float(test_dataset.fx)
    spp = int(spp)
    if spp < 1:
        raise ValueError(f"evaluate: spp is at least 1, got {spp}")
    if spp > 1 and material_maps:
        raise ValueError("evaluate: the material maps are not accumulated (material_maps needs spp = 1)")
    if denoise is not None and spp < 2:
        raise ValueError(f"evaluate: denoise needs spp >= 2, got spp = {spp}")
    if savePath is not None:
        for sub in ("", "world_normal", "acc_map", "err") + (MATERIAL_DIRS if material_maps else ()) + (SAMPLE_DIRS if spp > 1 else ()):
            os.makedirs(os.path.join(savePath, sub), exist_ok=True)
    has_normal = getattr(test_dataset, "has_normal", None)
    acc_maps = getattr(test_dataset, "acc_maps", [])
    psnrs, ssims, norm_errs = [], [], []
    t_render = t_metric = 0.0
    was_training = tensorf.training
    tensorf.eval()
    for idx, im_idx, rays, gt_rgb in iterator():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keys = ("rgb_map", "acc_map", "world_normal") + (("depth",) + MATERIAL_KEYS if material_maps else ())
        if spp > 1:
            from .multisample import render_frame
            ims, _ = render_frame(tensorf, rays.to(device), focal, spp=spp, min_spp=min_spp, tol=tol, jitter=False, noise=noise, keys=keys,
                                  denoise=denoise, frame_hw=(H, W) if denoise is not None else None)
        else:
            ims = render_images(tensorf, rays.to(device), focal, noise=noise, keys=keys)
        rgb = ims["rgb_map"].reshape(H, W, 3)
        acc = ims["acc_map"].reshape(H, W)
        wn = ims["world_normal"].reshape(H, W, 3)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t_render += t1 - t0
        if gt_rgb is not None:
            gt = gt_rgb.reshape(H, W, 3).to(rgb.device, torch.float32)
            if has_normal is not None and im_idx < len(acc_maps) and has_normal(im_idx):
                gt_n = test_dataset.get_normal(im_idx).to(rgb.device, torch.float32).reshape(1, -1, 3)
                alpha = acc_maps[im_idx].reshape(1, -1).to(rgb.device, torch.float32)
                norm_errs.append(float(hip.normal_err(wn.reshape(1, -1, 3).contiguous(), gt_n.contiguous(), alpha)[0]))
            psnrs.append(float(psnr_8bit(rgb, gt)))
            if compute_extra_metrics:
                # renderer.py:399, the 8-bit prediction: k / 255 correctly rounded (the reference divides on the host; a device
                # division by a scalar multiplies by the reciprocal, an ulp away for some k)
                q = (torch.floor(rgb.clip(0, 1) * 255).double() / 255).float()
                ssims.append(float(hip.ssim(q.contiguous(), gt.contiguous(), max_val=1.0)[0]))
        t_metric += time.perf_counter() - t1
        if savePath is not None:
            # renderer.py:343-347, 414-415, 440-451, 489-492: 8-bit conversions of the reference
            _png(os.path.join(savePath, f"{prtx}{idx:03d}.png"), (rgb.clamp(0, 1).cpu().numpy() * 255).astype("uint8"))
            _png(os.path.join(savePath, "world_normal", f"{prtx}{idx:03d}.png"),
                 (wn * 127 + 128).clamp(0, 255).byte().cpu().numpy())
            _png(os.path.join(savePath, "acc_map", f"{prtx}{idx:03d}.png"),
                 (255 * acc.clamp(0, 1).cpu().numpy()).astype(np.uint8))
            if gt_rgb is not None:
                err = (rgb.clip(0, 1) - gt.clip(0, 1)) + 0.5
                _png(os.path.join(savePath, "err", f"{prtx}{idx:03d}.png"), (err.clamp(0, 1).cpu().numpy() * 255).astype("uint8"))
            if material_maps:
                write_material_maps(savePath, f"{prtx}{idx:03d}", ims, H, W)
            if spp > 1:
                write_sample_maps(savePath, f"{prtx}{idx:03d}", ims, H, W)
    tensorf.train(was_training)

    final_stats = {}
    if psnrs:
        psnr = float(np.mean(np.asarray(psnrs)))
        final_stats["psnr"] = psnr
        final_stats["norm_err"] = float(np.mean(np.asarray(norm_errs))) if norm_errs else 0
        if compute_extra_metrics:
            final_stats["ssim"] = float(np.mean(np.asarray(ssims)))
            row = [psnr, final_stats["ssim"], np.nan, np.nan]                   # LPIPS alex / vgg: not computed
        else:
            row = [psnr]
        if savePath is not None:
            np.savetxt(os.path.join(savePath, f"{prtx}mean.txt"), np.asarray(row))
    if savePath is not None:
        import yaml
        with open(os.path.join(savePath, f"stats{prtx}.yaml"), "w") as f:
            yaml.dump(final_stats, f)
    return dict(psnrs=psnrs, norm_errs=norm_errs, ssims=ssims, seconds=dict(render=t_render, metrics=t_metric))


@torch.no_grad()
def evaluation(test_dataset, tensorf, unused, renderer, savePath=None, *, N_vis=5, prtx="", N_samples=-1, white_bg=False,
               ndc_ray=False, compute_extra_metrics=True, device="cuda", noise=None, material_maps=False, spp=1, min_spp=4, tol=None,
               denoise=None, **kw):
    """renderer.py:513-560: every max(N // N_vis, 1)-th view of a stacked test set (all views with N_vis < 0) through
    `evaluate`; the call shape of train.py:863-875.  spp, min_spp, tol, denoise: evaluate's multi-sample views."""
    n = test_dataset.all_rays.shape[0]
    step = 1 if N_vis < 0 else max(n // N_vis, 1)
    idxs = list(range(0, n, step))
    have_gt = len(test_dataset.all_rgbs) > 0

    def iterator():
        for idx, im_idx in enumerate(idxs):
            rays = test_dataset.all_rays[im_idx].reshape(-1, test_dataset.all_rays.shape[-1])
            yield idx, im_idx, rays, (test_dataset.all_rgbs[im_idx] if have_gt else None)

    return evaluate(iterator, test_dataset, tensorf, renderer, savePath, prtx=prtx, N_samples=N_samples, white_bg=white_bg,
                    ndc_ray=ndc_ray, compute_extra_metrics=compute_extra_metrics, device=device, noise=noise,
                    material_maps=material_maps, spp=spp, min_spp=min_spp, tol=tol, denoise=denoise, **kw)


PATH_PANELS = dict(rgb="rgb_map", depth="depth", normal="world_normal", acc="acc_map")       # panel -> key of render_images, in strip order
PATH_DIRS = dict(depth="depth", normal="world_normal", acc="acc_map")                        # the folders of `evaluation`


def _write_animation(path, frames, animation, fps):
    """the reference's video.mp4 / depthvideo.mp4 (renderer.py:492-497, imageio) under their names as an animated PNG (or GIF)
    written by Pillow: no video encoder is a dependency"""
    from PIL import Image
    ims = [Image.fromarray(a) for a in frames]
    kw = dict(save_all=True, append_images=ims[1:], duration=1000.0 / fps, loop=0)
    if animation == "apng":
        ims[0].save(path + ".png", format="PNG", **kw)
    else:
        ims[0].save(path + ".gif", format="GIF", **kw)


@torch.no_grad()
def evaluation_path(test_dataset, tensorf, c2ws, renderer, savePath, *, prtx="", device="cuda", noise=None, panels=("rgb", "depth"),
                    animation="apng", fps=30, camera=None, writer_depth=2, spp=1, min_spp=4, tol=None, denoise=None):
    """renderer.py:564-582 (the call shape of train.py:884-901): renders the camera path c2ws [n, 4, 4] (camera-to-world, the loader's
    convention; nmf_amd/camera_path.py) into savePath.  `renderer` is ignored, as in `evaluation`.  The camera is test_dataset's
    (size, fx / fy, centred principal point, near_far) or camera = dict(w, h, fx, fy, cx, cy, near_far), with which test_dataset may
    be None (a checkpoint rendered without a data set).

    Per frame: the rays are made on the device from the pose (hip.camera_rays, one buffer for the whole path), rendered by
    render_images with the keys the panels need, turned into ONE uint8 strip rgb | depth | normal | acc (hip.frame_finish: the 8-bit
    conversions of `evaluation`; depth between near_far through hip.depth_colour_table) and copied into a pinned buffer without
    blocking; a writer thread waits for the copy's event, slices the panels and encodes the PNGs while the next frame renders:
    {prtx}{k:03d}.png (rgb, always a panel) and depth/, world_normal/, acc_map/ as in `evaluation`.  writer_depth bounds the frames
    in flight (0: written on the calling thread); frames come out in order; an exception in the writer is raised here; the thread
    is joined before the function returns.  At the end {prtx}video.png (and {prtx}depthvideo.png with a depth panel) hold the frames
    as an animated PNG (animation="gif": .gif; "none": neither) and transforms_path.json the path (camera_path.save_path).
    spp > 1: a frame is multisample.render_frame's mean of up to spp jittered passes from the pose (min_spp, tol: its adaptive stop;
    one FrameAccumulator for the path; the frame's device time is all under `render`), spp/ and noise/ PNGs are written on the calling
    thread (write_sample_maps) and the result gains rays_rendered and passes per frame.  spp = 1 runs the single pass as before.
    denoise: a multisample.DenoiseParams -- every finished frame is filtered (needs spp >= 2; the filter's guides make every pass render
    depth and normal whatever the panels are); spp/ and noise/ keep the measured counts and errors.
    -> dict(frames, panels, seconds=dict(rays, render, finish: device time from events; write_wait: the calling thread blocked on
    the writer; total: wall clock until the last frame is on disk; animation: the container), frame_ms=dict(rays, render, finish:
    the device times per frame), rays_per_s)."""
    import queue
    import threading

    from . import camera_path, hip
    panels = tuple(p for p in PATH_PANELS if p in panels)
    if "rgb" not in panels:
        raise ValueError("evaluation_path: rgb is always a panel ({prtx}{k:03d}.png)")
    if animation not in ("apng", "gif", "none"):
        raise ValueError(f"evaluation_path: animation is apng, gif or none, got '{animation}'")
    cam = dict(camera) if camera is not None else camera_path.dataset_camera(test_dataset)
    W, H, near_far = int(cam["w"]), int(cam["h"]), cam["near_far"]
    c2ws = np.asarray(c2ws.cpu() if isinstance(c2ws, torch.Tensor) else c2ws, dtype=np.float32)
    n = c2ws.shape[0]
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    spp = int(spp)
    if spp < 1:
        raise ValueError(f"evaluation_path: spp is at least 1, got {spp}")
    if denoise is not None and spp < 2:
        raise ValueError(f"evaluation_path: denoise needs spp >= 2, got spp = {spp}")
    for sub in ("",) + tuple(PATH_DIRS[p] for p in panels if p in PATH_DIRS) + (SAMPLE_DIRS if spp > 1 else ()):
        os.makedirs(os.path.join(savePath, sub), exist_ok=True)
    keys = tuple(PATH_PANELS[p] for p in panels)
    accumulator, sampled = None, []
    if spp > 1:
        from .multisample import FrameAccumulator, render_frame
        accumulator = FrameAccumulator(H, W, device)
    rays = torch.empty((H * W, 6), dtype=torch.float32, device=device)
    strip = torch.empty((H, len(panels) * W, 3), dtype=torch.uint8, device=device)
    pool = queue.Queue()
    for _ in range(max(int(writer_depth), 0) + 1):
        pool.put(torch.empty(strip.shape, dtype=torch.uint8).pin_memory())
    kept = {p: [] for p in ("rgb", "depth") if p in panels and animation != "none"}
    failure = []

    def write(k, pin, done):
        done.synchronize()
        a = pin.numpy()
        for j, p in enumerate(panels):
            panel = a[:, j * W:(j + 1) * W]
            _png(os.path.join(savePath, PATH_DIRS.get(p, ""), f"{prtx}{k:03d}.png"), panel)
            if p in kept:
                kept[p].append(panel.copy())

    work = queue.Queue()

    def writer():
        while True:
            item = work.get()
            if item is None:
                return
            try:
                if not failure:                       # (after a failure: only hand the buffers back, so that the caller never blocks)
                    write(*item)
            except BaseException as e:                # noqa: BLE001 -- raised again on the calling thread
                failure.append(e)
            finally:
                pool.put(item[1])

    thread = None
    if writer_depth > 0:
        thread = threading.Thread(target=writer, name="nmf-path-writer", daemon=True)
        thread.start()
    marks = []
    t_wait = 0.0
    was_training = tensorf.training
    tensorf.eval()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    try:
        for k in range(n):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]      # rays 0-1, render 1-2, finish 3-4
            ev[0].record()
            if spp > 1:
                ev[1].record()
                ims, st = render_frame(tensorf, c2ws[k], cam, spp=spp, min_spp=min_spp, tol=tol, jitter=True, noise=noise, keys=keys,
                                       accumulator=accumulator, denoise=denoise)
                sampled.append(st)
                write_sample_maps(savePath, f"{prtx}{k:03d}", ims, H, W)
            else:
                hip.camera_rays(c2ws[k], cam["fx"], cam["fy"], cam["cx"], cam["cy"], H, W, out=rays)
                ev[1].record()
                ims = render_images(tensorf, rays, float(cam["fx"]), noise=noise, keys=keys)
                ims = dict(rgb_map=ims) if keys == ("rgb_map",) else ims
            ev[2].record()
            tw = time.perf_counter()
            pin = pool.get()                          # a free pinned buffer: blocks while writer_depth frames are in flight
            t_wait += time.perf_counter() - tw
            if failure:
                pool.put(pin)
                break
            ev[3].record()
            hip.frame_finish(H, W, **{p: ims[PATH_PANELS[p]] for p in panels}, near_far=near_far, out=strip)
            ev[4].record()
            pin.copy_(strip, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            marks.append(ev)
            if thread is None:
                tw = time.perf_counter()
                try:
                    write(k, pin, done)
                finally:
                    pool.put(pin)
                t_wait += time.perf_counter() - tw
            else:
                work.put((k, pin, done))
    finally:
        if thread is not None:
            tw = time.perf_counter()
            work.put(None)
            thread.join()
            t_wait += time.perf_counter() - tw
        tensorf.train(was_training)
    if failure:
        raise failure[0]
    torch.cuda.synchronize(device)
    total = time.perf_counter() - t0
    frame_ms = {name: [e[i].elapsed_time(e[i + 1]) for e in marks] for name, i in (("rays", 0), ("render", 1), ("finish", 3))}
    dev_s = [sum(frame_ms[name]) * 1e-3 for name in ("rays", "render", "finish")]
    t1 = time.perf_counter()
    if animation != "none" and n > 0:
        _write_animation(os.path.join(savePath, f"{prtx}video"), kept["rgb"], animation, fps)
        if "depth" in kept:
            _write_animation(os.path.join(savePath, f"{prtx}depthvideo"), kept["depth"], animation, fps)
    angle = 2.0 * float(np.arctan(0.5 * W / cam["fx"]))
    camera_path.save_path(os.path.join(savePath, "transforms_path.json"), c2ws, angle, W, H, near_far,
                          intrinsics=(cam["fx"], cam["fy"], cam["cx"], cam["cy"]))
    res = dict(frames=n, panels=list(panels),
               seconds=dict(rays=dev_s[0], render=dev_s[1], finish=dev_s[2], write_wait=t_wait, total=total,
                            animation=time.perf_counter() - t1),
               frame_ms=frame_ms, rays_per_s=n * H * W / total if total > 0 else 0.0)
    if spp > 1:
        res.update(rays_rendered=[st["rays_rendered"] for st in sampled], passes=[st["passes"] for st in sampled])
    return res
