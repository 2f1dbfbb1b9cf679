"""Inference entry point -- counterpart of the reference's `render_only=True` path (train.py:64-190 `render_test`,
renderer.py:56-106 `chunk_renderer`, :399-401 PSNR) for checkpoints written by TensorNeRF.save:

    python -m nmf_amd.render --ckpt log/lego.th --datadir /data/nerf_synthetic/lego [--fixed-bg forest.th] [--out imgs/]
    python -m nmf_amd.render --ckpt log/s1.th --views 4 --res 800                      (synthetic orbit cameras)

--fixed-bg swaps the learned environment map for another IntegralEquirect state_dict (relighting, train.py:96-138); the
module is rebuilt at the resolution stored in that file (the reference hard-codes 512 and fails on other sizes).
Prints one JSON line: frames, rays/s (render to completion, eval_batch_size rays per chunk), mean PSNR when ground truth exists.

    python -m nmf_amd.render --ckpt log/lego.th --datadir /data/nerf_synthetic/lego --eval-dir log/lego/imgs_test_all

--eval-dir (the reference's render_only + render_test, train.py:167-180) then evaluates the views with renderer.evaluation:
frames, mean.txt and stats.yaml go to DIR, and the line gains ssim, norm_err and the evaluation's render / metric seconds.
--material-maps adds the material maps of every view (renderer.py:433-463): albedo/, roughness/, tint/, diffuse/ PNGs, spec/ and
rgbd/ (depth) EXRs.

    python -m nmf_amd.render --ckpt log/s1.th --env-rotate 90 0 0                      (the scene's own lighting, turned)
    python -m nmf_amd.render --ckpt log/s1.th --fixed-bg studio.exr --bg-res 512 --light-turntable 36 --out imgs/

Relighting (nmf_amd/relight.py): --fixed-bg also takes a panorama (.exr, .npy or an image), imported directly at
--bg-res without an optimisation run; --env-rotate YAW PITCH ROLL (degrees, +z up) rotates the lighting -- the checkpoint's own map or
the --fixed-bg one; --light-turntable N then renders view 0 N times under a further yaw of 360 k / N (light_000.png ... in --out) and
the line gains light_frames and, per frame, the seconds of the environment update and of the render.

    python -m nmf_amd.render --ckpt log/car.th --datadir /data/relighting/car_exr --fixed-bg forest.exr --relight-eval log/car/imgs_test_ori

--relight-eval DIR (nmf_amd/relight_eval.py; the reference's scripts/relighting_calc.ipynb) scores the relit test views
of an EXR set against its ground truth: HDR frames {idx:03d}.exr, adjusted/{idx:03d}.png and stats.yaml go to DIR, and the line gains
relight = {psnr, ssim, multiplier, views}.  Combines with --env-rotate, --bg-res and --n-vis.

    python -m nmf_amd.render --ckpt log/lego.th --datadir /data/nerf_synthetic/lego --path orbit --frames 120 --out imgs/
    python -m nmf_amd.render --ckpt log/s1.th --fixed-bg studio.exr --env-rotate 90 0 0 --path spiral --panels rgb,depth,normal --out imgs/
    python -m nmf_amd.render --ckpt log/s1.th --path imgs/path/transforms_path.json --out again/

--path orbit|spiral|interp|FILE.json (nmf_amd/camera_path.py, renderer.evaluation_path; the reference's render_path,
train.py:884-901) renders views that are in no data set into OUT/path/: --frames poses around the data set's scene (without
--datadir: a --res square camera, radius 4, elevation 30 degrees) or the poses of a transforms file; {k:03d}.png, depth/,
world_normal/, acc_map/ per --panels, video.png / depthvideo.png (animated PNGs at --fps; --animation gif|none) and
transforms_path.json.  Rays and 8-bit frames are made on the device; PNGs are encoded on a writer thread.  The line gains `path`.

    python -m nmf_amd.render --ckpt log/car.th --insert 'log/toaster.th@t=0,0,0.9;r=40,0,0;s=0.4' --path orbit --out imgs/

--insert 'CKPT[@SPEC]' (repeatable; nmf_amd/compose.py; the reference's scripts/toaster_on_car.py) puts further trained
objects into the scene of --ckpt, which --place SPEC moves itself: the objects occlude, shadow and reflect each other under ONE
environment (the --ckpt model's own, carried along with it, or the --fixed-bg / --env-rotate one).  SPEC is t=x,y,z;r=yaw,pitch,roll;s=scale
(local -> world, degrees, +z up; any subset).  --near-far is then in world units, and without it every object is marched over the range
its box limits.  Works with --views, --path, --panels, --fixed-bg, --env-rotate and --light-turntable; orbit and spiral paths circle
the box around all objects.  The line gains `parts` and `placements`.

    python -m nmf_amd.render --ckpt log/lego.th --path orbit --spp 16 --adaptive 1 --out imgs/

--spp N (nmf_amd/multisample.py) renders every frame as the mean of up to N passes per pixel, averaged in linear radiance
on the device and tonemapped afterwards; a frame of one pass carries the Monte-Carlo grain of its secondary rays, which flickers
along a path.  --adaptive [TOL] stops a pixel once the standard error of its displayed colour is below TOL / 255 (in 8-bit levels; without
a value: multisample.ADAPTIVE_DEFAULT), after at least --min-spp passes (default 4).  --path frames are jittered inside the pixel; the
views of --views, --eval-dir, --relight-eval and --light-turntable keep their rays through the pixel centres.  --path and --eval-dir
also write spp/ (sample count) and noise/ (standard error) PNGs.  Works with --insert and --edit; --material-maps is refused (the
material maps are not accumulated).  The line gains `sampling`.

    python -m nmf_amd.render --ckpt log/lego.th --path orbit --spp 4 --denoise --out imgs/

--denoise [LEVELS] (with --spp 2 or more; multisample.DenoiseParams) filters every finished frame with the
variance-guided, edge-stopping a-trous filter of csrc/denoise.hip: LEVELS levels of steps 1, 2, 4, ... (default 3, at most 8), stopped
by the frame's own mean depth, normal and coverage; pixels whose samples all agreed keep their bytes.  --denoise-strength K_C is the
width of the colour test in standard errors (default 4; larger smooths more).  Works with everything --spp works with, --adaptive
among them; spp/ and noise/ keep showing the measured counts and errors.  `sampling` gains `denoise`, the parameters.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from . import edit, synthetic
from .modules.integral_equirect import IntegralEquirect
from .modules.tensor_nerf import TensorNeRF
from .multisample import ADAPTIVE_DEFAULT
from .noise import DeviceNoise
from .renderer import psnr_8bit, render_images


PANORAMA_SUFFIXES = (".exr", ".npy", ".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def load_fixed_bg(path, device, bg_res=512):
    """train.py:96-138: an IntegralEquirect with mipbias 0 / activation exp, its learning rates zeroed.  A panorama (.exr, .npy, an
    image) instead of a state_dict is imported directly at bg_res (relight.import_panorama)"""
    if str(path).lower().endswith(PANORAMA_SUFFIXES):
        from .pano2env import read_panorama
        from .relight import import_panorama
        return import_panorama(read_panorama(path), bg_res, device=device)
    from .checkpoint import load_checkpoint
    sd = load_checkpoint(path)
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) and "bg_mat" not in sd else sd
    res = int(sd["bg_mat"].shape[-2])
    bg = IntegralEquirect(bg_resolution=res, mipbias=0, activation="exp", lr=0.0, init_val=-1.897, mul_lr=0.0,
                          brightness_lr=0, betas=[0.0, 0.0], mul_betas=[0.9, 0.9], mipbias_lr=0.0, mipnoise=0.0)
    bg.load_state_dict({k: v for k, v in sd.items() if k in bg.state_dict()}, strict=False)
    return bg.to(device)


@torch.no_grad()
def render_frames(nerf, rays, focal, chunk, noise, sampling=None, wh=None):
    """rays [F, h*w, 6] -> rgb [F, h*w, 3], seconds; render2completion over `chunk`-ray slices (renderer.py:56-106).  sampling =
    dict(spp, min_spp, tol[, denoise]) with spp > 1: every frame is multisample.render_frame's mean over passes of the same rays; a
    denoised frame needs wh = [w, h], the shape its rays form"""
    out = []
    frame = dict(frame_hw=(int(wh[1]), int(wh[0]))) if sampling and sampling.get("denoise") is not None else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in range(rays.shape[0]):
        if sampling and sampling["spp"] > 1:
            from .multisample import render_frame
            out.append(render_frame(nerf, rays[f], focal, jitter=False, noise=noise, chunk=chunk, **sampling, **(frame or {}))[0]["rgb_map"])
        else:
            out.append(render_images(nerf, rays[f], focal, chunk, noise))
    torch.cuda.synchronize()
    return torch.stack(out), time.perf_counter() - t0


@torch.no_grad()
def light_turntable(nerf, rays, focal, chunk, noise, n, wh, out_dir=None, sampling=None):
    """view rays [1, h*w, 6] rendered n times under nerf's lighting turned by a yaw of 360 k / n: ONE map module is rewritten per frame
    (relight.rotate_env(out=)), its tables rebuild in place.  -> the keys the JSON line gains; light_%03d.png in out_dir"""
    from . import relight
    base = nerf.bg_module
    turned = relight.rotate_env(base, relight.rotation(0.0))
    env_s, render_s = [], []
    with relight.relit(nerf, turned):
        for k in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            relight.rotate_env(base, relight.rotation(yaw=360.0 * k / n), out=turned)
            turned._tables_checked()                                         # SAT rebuild
            turned.get_spherical_harmonics(100)                             # SH irradiance of the turned map
            torch.cuda.synchronize()
            env_s.append(round(time.perf_counter() - t0, 6))
            rgb, dt = render_frames(nerf, rays, focal, chunk, noise, sampling, wh)
            render_s.append(round(dt, 6))
            if out_dir:
                from PIL import Image
                os.makedirs(out_dir, exist_ok=True)
                a = (rgb[0].clip(0, 1).reshape(wh[1], wh[0], 3) * 255).byte().cpu().numpy()
                Image.fromarray(a).save(os.path.join(out_dir, f"light_{k:03d}.png"))
    return dict(light_frames=n, light_env_seconds=env_s, light_render_seconds=render_s)


def _model_aabb(nerf):
    from . import hip
    return hip.host(nerf.rf.aabb).astype(np.float64).reshape(2, 3)


def render_path(nerf, args, ds, near_far, panels, noise, dev, sampling=None):
    """--path: the poses (nmf_amd/camera_path.py) and the camera, rendered by renderer.evaluation_path into <out>/path/ under the
    lighting the command set up (--fixed-bg, --env-rotate, --bg-res).  Without a data set the camera is --res square with the
    synthetic scene's camera_angle_x and the orbit has radius 4 at elevation 30 degrees around the origin.  -> the `path` key"""
    import math

    from . import camera_path
    from .renderer import evaluation_path
    if ds is not None:
        camera = camera_path.dataset_camera(ds)
    else:
        fx = 0.5 * args.res / math.tan(0.5 * synthetic.CAMERA_ANGLE_X)
        camera = dict(w=args.res, h=args.res, fx=fx, fy=fx, cx=args.res / 2, cy=args.res / 2, near_far=list(near_far))
    if args.path in ("orbit", "spiral", "interp"):
        if ds is not None:
            c2ws = camera_path.from_dataset(ds, args.path, args.frames)
        else:
            center, radius = (0.0, 0.0, 0.0), 4.0
            if hasattr(nerf, "world_aabb"):
                # a composed scene: around the box of all objects, at the distance that shows it as radius 4 shows one object
                box = nerf.world_aabb()
                own = _model_aabb(nerf.parts[0][0])
                center = tuple(float(v) for v in 0.5 * (box[0] + box[1]))
                radius = 4.0 * max(float(np.linalg.norm(box[1] - box[0]) / np.linalg.norm(own[1] - own[0])), 1.0)
            if args.path == "orbit":
                c2ws = camera_path.orbit(args.frames, center, radius, 30.0)
            else:
                c2ws = camera_path.spiral(args.frames, center, radius, (15.0, 45.0))
    else:
        c2ws, camera = camera_path.load_path(args.path, with_camera=True)
        if "near_far" not in json.load(open(args.path)):
            camera["near_far"] = list(near_far)
    out = os.path.join(args.out, "path")
    res = evaluation_path(None, nerf, c2ws, None, out, device=dev, noise=noise, panels=panels, animation=args.animation, fps=args.fps,
                          camera=camera, **(sampling or {}))
    rec = dict(kind=args.path, dir=out, frames=res["frames"], panels=res["panels"], width=camera["w"], height=camera["h"],
               seconds={k: round(v, 4) for k, v in res["seconds"].items()}, rays_per_s=round(res["rays_per_s"], 1))
    if "rays_rendered" in res:
        rec.update(rays_rendered=res["rays_rendered"], passes=res["passes"])
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--datadir", default=None)
    ap.add_argument("--near-far", type=float, nargs=2, default=None,
                    help="near and far plane of the synthetic cameras (default 2.5 7.0; with --insert / --place: world units, default: "
                         "every object over the range its box limits)")
    ap.add_argument("--fixed-bg", default=None)
    ap.add_argument("--out", default=None, help="directory for PNG frames")
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--n-vis", type=int, default=-1)
    ap.add_argument("--chunk", type=int, default=None, help="rays per chunk (default: the model's eval_batch_size)")
    ap.add_argument("--eval-dir", default=None,
                    help="with --datadir: evaluate the test views (PSNR, SSIM, normal error) into this directory")
    ap.add_argument("--material-maps", action="store_true",
                    help="with --eval-dir: also write the material maps (albedo/, roughness/, tint/, diffuse/ PNGs, spec/ and rgbd/ EXRs)")
    ap.add_argument("--bg-res", type=int, default=512, help="resolution a --fixed-bg PANORAMA is imported at")
    ap.add_argument("--env-rotate", type=float, nargs=3, default=None, metavar=("YAW", "PITCH", "ROLL"),
                    help="rotate the lighting (degrees, +z up): the checkpoint's own environment map or the --fixed-bg one")
    ap.add_argument("--light-turntable", type=int, default=0, metavar="N",
                    help="render view 0 N times under a yaw of 360 k / N of the lighting (light_000.png ... in --out)")
    ap.add_argument("--relight-eval", default=None, metavar="DIR",
                    help="with --datadir of an EXR test set: fit the brightness multiplier and write HDR frames, adjusted/ and stats.yaml")
    ap.add_argument("--path", default=None, metavar="orbit|spiral|interp|FILE.json",
                    help="render a camera path into --out/path/: a fly-around, a spiral, an interpolation through poses of the test "
                         "set, or a transforms file written by an earlier run (transforms_path.json) or by hand")
    ap.add_argument("--frames", type=int, default=120, help="frames of a generated --path")
    ap.add_argument("--fps", type=float, default=30.0, help="frame rate of the path's animation")
    ap.add_argument("--panels", default="rgb,depth", help="panels of a --path frame, from rgb,depth,normal,acc (rgb always)")
    ap.add_argument("--animation", choices=("apng", "gif", "none"), default="apng",
                    help="container of the path's video.png / depthvideo.png (an animated PNG), .gif, or none")
    ap.add_argument("--insert", action="append", default=[], metavar="CKPT[@SPEC]",
                    help="a further trained object in the scene, repeatable: a checkpoint and its placement "
                         "'t=x,y,z;r=yaw,pitch,roll;s=scale' (local -> world, degrees, +z up; any subset; default: the identity)")
    ap.add_argument("--place", default=None, metavar="SPEC", help="the placement of the --ckpt model itself in a composed scene")
    ap.add_argument("--spp", type=int, default=1, metavar="N",
                    help="passes per pixel of every frame, averaged in linear radiance on the device (default 1: the single pass)")
    ap.add_argument("--adaptive", type=float, nargs="?", const=ADAPTIVE_DEFAULT, default=None, metavar="TOL",
                    help="with --spp: stop a pixel once the standard error of its displayed colour is below TOL / 255 "
                         f"(8-bit levels; without a value: {ADAPTIVE_DEFAULT:g})")
    ap.add_argument("--min-spp", type=int, default=None, metavar="N", help="with --adaptive: passes every pixel gets (default 4, at most --spp)")
    ap.add_argument("--denoise", type=int, nargs="?", const=-100, default=None, metavar="LEVELS",
                    help="with --spp 2 or more: filter every finished frame (variance-guided a-trous filter; LEVELS levels, default 3, 0 to 8)")
    ap.add_argument("--denoise-strength", type=float, default=None, metavar="K_C",
                    help="with --denoise: the width of the colour test in standard errors (default 4; larger smooths more)")
    edit.add_arguments(ap)
    args = ap.parse_args(argv)
    if args.spp < 1:
        ap.error("--spp is at least 1")
    if args.adaptive is not None and args.spp < 2:
        ap.error("--adaptive needs --spp N with N > 1 (the most passes a pixel may get)")
    if args.adaptive is not None and not args.adaptive >= 0:
        ap.error("--adaptive takes a tolerance of 0 or more (in 8-bit levels)")
    if args.min_spp is not None and (args.min_spp < 1 or args.min_spp > args.spp):
        ap.error("--min-spp lies between 1 and --spp")
    if args.material_maps and args.spp > 1:
        ap.error("--material-maps with --spp above 1: the material maps are not accumulated")
    denoise = None
    if args.denoise_strength is not None and args.denoise is None:
        ap.error("--denoise-strength needs --denoise")
    if args.denoise is not None:
        from .multisample import DenoiseParams
        if args.spp < 2:
            ap.error("--denoise needs --spp N with N > 1 (the filter is steered by the variance of a pixel's samples)")
        if args.denoise != -100 and not 0 <= args.denoise <= 8:
            ap.error("--denoise takes a number of levels from 0 to 8")
        if args.denoise_strength is not None and not 0 < args.denoise_strength < float("inf"):
            ap.error("--denoise-strength takes a finite width above 0 (in standard errors)")
        given = dict(levels=args.denoise) if args.denoise != -100 else {}
        if args.denoise_strength is not None:
            given["k_c"] = args.denoise_strength
        denoise = DenoiseParams(**given)
    sampling = None
    if args.spp > 1:
        sampling = dict(spp=args.spp, min_spp=args.min_spp if args.min_spp is not None else min(4, args.spp),
                        tol=None if args.adaptive is None else args.adaptive / 255.0)
        if denoise is not None:
            sampling["denoise"] = denoise
    composed = bool(args.insert) or args.place is not None
    placements = None
    if composed:
        from .compose import Placement
        for flag, given in (("--eval-dir", args.eval_dir), ("--relight-eval", args.relight_eval), ("--material-maps", args.material_maps),
                            ("--edit", args.edit or args.edit_file)):
            if given:
                ap.error(f"{flag} is not built for a composed scene (--insert / --place)")
        if len(args.insert) > 7:
            ap.error("--insert: a composed scene has at most 8 objects")
        try:
            placements = [Placement.from_spec(args.place or "")]
            inserts = []
            for item in args.insert:
                ckpt, _, spec = item.partition("@")
                if not ckpt:
                    ap.error(f"--insert '{item}': no checkpoint")
                inserts.append(ckpt)
                placements.append(Placement.from_spec(spec))
        except ValueError as e:
            ap.error(f"--insert / --place: {e}")
    explicit_near_far = args.near_far is not None
    if args.near_far is None:
        args.near_far = [2.5, 7.0]
    try:
        material_edits = edit.from_args(args)
    except (edit.EditError, OSError) as e:
        ap.error(str(e))
    if args.path:
        if not args.out:
            ap.error("--path needs --out (the frames go to OUT/path/)")
        if args.frames < 1:
            ap.error("--frames is at least 1")
        path_panels = tuple(p for p in args.panels.split(",") if p)
        if not path_panels or set(path_panels) - {"rgb", "depth", "normal", "acc"} or "rgb" not in path_panels:
            ap.error("--panels is a comma-separated choice of rgb,depth,normal,acc that includes rgb")
        if args.path == "interp" and not args.datadir:
            ap.error("--path interp needs --datadir (it interpolates poses of the test set)")
        if args.path not in ("orbit", "spiral", "interp") and not os.path.isfile(args.path):
            ap.error(f"--path: '{args.path}' is neither orbit, spiral, interp nor a file")
    if args.light_turntable < 0:
        ap.error("--light-turntable takes a number of frames")
    if args.eval_dir and not args.datadir:
        ap.error("--eval-dir needs --datadir (ground truth of a Blender scene)")
    if args.relight_eval and not args.datadir:
        ap.error("--relight-eval needs --datadir (an EXR test set with ground truth)")
    if args.material_maps and not args.eval_dir:
        ap.error("--material-maps needs --eval-dir")
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    gt = None
    if args.datadir:
        from .dataLoader import BlenderDataset
        ds = BlenderDataset(args.datadir, split="test", is_stack=True, N_vis=args.n_vis)
        if args.relight_eval and not ds.hdr:
            ap.error("--relight-eval needs an EXR test set (linear RGBA ground truth); this scene's frames are not EXR files")
        rays, focal, near_far = ds.all_rays.to(dev), float(ds.fx), tuple(ds.near_far)
        gt = ds.all_rgbs.reshape(rays.shape[0], -1, 3).to(dev)
        wh = ds.img_wh
    else:
        r, focal = synthetic.orbit_rays(args.views, args.res, seed=2)
        rays, near_far, wh = r.reshape(args.views, -1, 6).to(dev), tuple(args.near_far), [args.res, args.res]
    nerf = TensorNeRF.load(args.ckpt, near_far=list(near_far), device=dev)
    if composed:
        from .compose import ComposedScene
        models = [nerf.eval()] + [TensorNeRF.load(c, near_far=list(near_far), device=dev).eval() for c in inserts]
        nerf = ComposedScene(list(zip(models, placements)), near_far=tuple(args.near_far) if explicit_near_far else None)
    if args.fixed_bg:
        nerf.bg_module = load_fixed_bg(args.fixed_bg, dev, args.bg_res)
    if args.env_rotate is not None:
        from . import relight
        nerf.bg_module = relight.rotate_env(nerf.bg_module, relight.rotation(*args.env_rotate))
    nerf.eval()
    if not composed:
        nerf.set_material_edits(material_edits)          # every mode below renders the edited materials
    chunk = args.chunk or nerf.eval_batch_size
    noise = DeviceNoise(dev, seed=11)
    render_frames(nerf, rays[:1, : min(chunk, rays.shape[1])], focal, chunk, noise)          # warm-up (table builds)
    rgb, dt = render_frames(nerf, rays, focal, chunk, noise, sampling, wh)
    rec = dict(frames=int(rays.shape[0]), width=wh[0], height=wh[1], chunk=chunk, seconds=round(dt, 4),
               rays_per_s=round(rays.shape[0] * rays.shape[1] / dt, 1), relit=bool(args.fixed_bg))
    if composed:
        rec.update(parts=len(placements), placements=[p.spec() for p in placements])
    if sampling:
        rec["sampling"] = dict(spp=sampling["spp"], min_spp=sampling["min_spp"], adaptive=args.adaptive)
        if denoise is not None:
            rec["sampling"]["denoise"] = denoise.record()
    if gt is not None:
        rec["psnr"] = round(float(torch.stack([psnr_8bit(rgb[i], gt[i]) for i in range(rgb.shape[0])]).mean()), 3)
    if args.out:
        from PIL import Image
        os.makedirs(args.out, exist_ok=True)
        for i in range(rgb.shape[0]):
            a = (rgb[i].clip(0, 1).reshape(wh[1], wh[0], 3) * 255).byte().cpu().numpy()
            Image.fromarray(a).save(os.path.join(args.out, f"{i:03d}.png"))
    if args.light_turntable:
        rec.update(light_turntable(nerf, rays[:1], focal, chunk, noise, args.light_turntable, wh, args.out, sampling))
    if args.eval_dir:
        from .renderer import evaluation
        from .train import test_all_record
        t0 = time.perf_counter()
        res = evaluation(ds, nerf, None, None, args.eval_dir, N_vis=-1, device=dev, noise=noise,
                         **(dict(material_maps=True) if args.material_maps else {}), **(sampling or {}))
        rec_all = test_all_record(res)
        rec.update(ssim=rec_all["ssim"], norm_err=rec_all["norm_err"],
                   eval_seconds=dict(total=round(time.perf_counter() - t0, 4), render=round(res["seconds"]["render"], 4),
                                     metrics=round(res["seconds"]["metrics"], 4)))
    if args.relight_eval:
        from .relight_eval import relight_evaluation
        res = relight_evaluation(nerf, ds, args.relight_eval, noise=noise, chunk=chunk, **(sampling or {}))
        rec["relight"] = dict(psnr=round(res["psnr"], 3), ssim=round(res["ssim"], 5), multiplier=res["multiplier"], views=res["views"])
    if args.path:
        rec["path"] = render_path(nerf, args, ds if args.datadir else None, near_far, path_panels, noise, dev, sampling)
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
