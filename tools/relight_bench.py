"""Relighting costs: the resampling kernel alone, a light-turntable frame's environment update against its render,
and the direct panorama import against pano2env.fit.

    python tools/relight_bench.py [--reps 20] [--res 400] [--frames 8] [--skip-fit]
HIP events, median (min / max) of --reps launches after a warm-up:
  kernel   nmf_env_resample 512x1024 -> 512x1024 at S = 4 (a rotation of the bench's map size) and a 2048x4096 panorama -> 1024x2048
           at the default S
  frame    per turntable frame on bench.py's S1 model: resample + SAT rebuild + SH projection, each and together, against the
           render of a --res x --res view under that map
  import   relight.import_panorama against pano2env.fit at its defaults on tests/golden/studio_dwab.exr: seconds and the figure both
           tools print (pano2env.panorama_error over the same pixels)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from nmf_amd import exr, hip, pano2env, relight, synthetic  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.renderer import render_images  # noqa: E402


def events_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return dict(median=round(statistics.median(out), 1), min=round(min(out), 1), max=round(max(out), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--skip-fit", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    R = relight.axis_angle((1, 2, 0.5), 0.9)
    g = torch.Generator().manual_seed(0)

    # ---- the kernel alone
    src = torch.rand((3, 512, 1024), generator=g).add_(0.05).to(dev)
    dst = torch.empty((3, 512, 1024), device=dev)
    rec = dict(kernel_rotate_512_S4_us=events_us(lambda: hip.env_resample(src, hip.ENV_SRC_MODULE, R, 1.0, 4, dst), a.reps))
    pano = torch.rand((2048, 4096, 3), generator=g).add_(0.05).to(dev)
    dst2 = torch.empty((3, 1024, 2048), device=dev)
    S = relight.default_supersample(4096, 1024)
    rec[f"kernel_import_2048x4096_to_1024_S{S}_us"] = events_us(lambda: hip.env_resample(pano, hip.ENV_SRC_PANORAMA, R, 1.0, S, dst2), a.reps)
    print(json.dumps(rec), flush=True)

    # ---- a turntable frame
    nerf, _ = bench.build(dev, grid=128)
    nerf.eval()
    base = nerf.bg_module
    turned = relight.rotate_env(base, R)
    rays, focal = synthetic.orbit_rays(1, a.res, seed=2)
    rays = rays.reshape(-1, 6).to(dev)
    noise = DeviceNoise(dev, seed=11)
    yaw = [0]

    def resample():
        yaw[0] += 1
        relight.rotate_env(base, relight.rotation(yaw=360.0 * yaw[0] / a.frames), out=turned)

    def update():
        resample()
        turned._tables_checked()
        turned.get_spherical_harmonics(100)

    def sat():
        torch.autograd.graph.increment_version(turned.bg_mat)
        turned._tables_checked()

    def shp():
        torch.autograd.graph.increment_version(turned.bg_mat)
        turned._tables_checked()
        turned.get_spherical_harmonics(100)

    H, W = base.hw()
    frame = dict(map=[H, W], resample_us=events_us(resample, a.reps), sat_rebuild_us=events_us(sat, a.reps),
                 sat_and_sh_us=events_us(shp, a.reps), env_update_us=events_us(update, a.reps))
    with relight.relit(nerf, turned), torch.no_grad():
        render_images(nerf, rays, focal, noise=noise)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.frames):
            update()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render_images(nerf, rays, focal, noise=noise)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    frame["render_ms"] = dict(res=a.res, median=round(statistics.median(ts), 2), min=round(min(ts), 2), max=round(max(ts), 2))
    print(json.dumps(dict(turntable_frame=frame)), flush=True)

    # ---- direct import against the fit
    p = exr.imread(os.path.join(ROOT, "tests", "golden", "studio_dwab.exr"))[..., :3]
    relight.import_panorama(p, 1024, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bg = relight.import_panorama(p, 1024, device=dev)
    torch.cuda.synchronize()
    imp = dict(direct_seconds=round(time.perf_counter() - t0, 5), direct_psnr=round(pano2env.panorama_error(bg, p), 3))
    if not a.skip_fit:
        t0 = time.perf_counter()
        fitted, _ = pano2env.fit(p, device=dev)
        torch.cuda.synchronize()
        imp.update(fit_seconds=round(time.perf_counter() - t0, 3), fit_psnr=round(pano2env.panorama_error(fitted, p), 3))
    print(json.dumps(dict(import_studio_1024=imp)), flush=True)


if __name__ == "__main__":
    main()
