"""Camera-path measurements of DESIGN.md 10.7 on one MI355X: an orbit of bench.py's S1 model (128^3, 800 x 800, 36 frames, panels
rgb | depth) through renderer.evaluation_path -- one warm-up path, then --reps per writer depth (2 and 0, alternating), device times
per frame from HIP events as median (min / max); the animated-PNG container; nmf_camera_rays and nmf_frame_finish alone (warm, 50
calls on buffers allocated once, bytes moved over the median); the pinned device-to-host copy of a strip; the PNG encode of a panel;
and the host route of a data-set frame (get_rays, upload, float32 read-back, numpy quantisation).  Prints one JSON document.

    python tools/path_bench.py [--reps 3] [--frames 36] [--res 800] [--out FILE.json]
"""
import argparse
import json
import os
import shutil
import statistics as st
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nmf_amd import camera_path as cp  # noqa: E402
from nmf_amd import hip, synthetic  # noqa: E402
from nmf_amd.config import build_model  # noqa: E402
from nmf_amd.dataLoader.blender import get_ray_directions, get_rays  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.renderer import _png, evaluation_path, render_images  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--frames", type=int, default=36)
ap.add_argument("--res", type=int, default=800)
ap.add_argument("--out", default=None, help="also write the JSON document to this file")
args = ap.parse_args()
RES, FRAMES = args.res, args.frames
mmm = lambda v: [round(st.median(v), 4), round(min(v), 4), round(max(v), 4)]      # noqa: E731
out = {}

nerf, _ = build_model(grid=128, bg_resolution=512, device=dev)
nerf.load_state_dict(synthetic.state_dict_s1(grid=128, bg_resolution=512, seed=0), strict=False)
nerf.sampler.update(nerf.rf, init=False)
nerf.sampler.update(nerf.rf, init=True)
nerf.eval()
fx = 0.5 * RES / np.tan(0.5 * synthetic.CAMERA_ANGLE_X)
camera = dict(w=RES, h=RES, fx=fx, fy=fx, cx=RES / 2, cy=RES / 2, near_far=[2.5, 7.0])
c2ws = cp.orbit(FRAMES, (0, 0, 0), 4.0, 30.0)
tmp = tempfile.mkdtemp()


def path(depth, animation="none", tag="p"):
    return evaluation_path(None, nerf, c2ws, None, os.path.join(tmp, tag), noise=DeviceNoise(dev, seed=3), camera=camera,
                           animation=animation, writer_depth=depth)


path(2, tag="warm")
runs = {0: [], 2: []}
for rep in range(args.reps):
    for depth in (2, 0):
        r = path(depth, tag=f"d{depth}_{rep}")
        runs[depth].append(r)
        print("path", depth, rep, {k: round(v, 4) for k, v in r["seconds"].items()}, flush=True)
for depth in (0, 2):
    rs = runs[depth]
    out[f"writer_depth_{depth}"] = dict(
        total_s=[round(r["seconds"]["total"], 4) for r in rs], frames_per_s=[round(FRAMES / r["seconds"]["total"], 3) for r in rs],
        write_wait_s=[round(r["seconds"]["write_wait"], 4) for r in rs],
        rays_ms=mmm([v for r in rs for v in r["frame_ms"]["rays"]]), render_ms=mmm([v for r in rs for v in r["frame_ms"]["render"]]),
        finish_ms=mmm([v for r in rs for v in r["frame_ms"]["finish"]]))
r = path(2, animation="apng", tag="apng")
out["apng_container_s"] = round(r["seconds"]["animation"], 3)

# the two kernels alone, warm
P = RES * RES
rays = torch.empty(P, 6, device=dev)
ims = render_images(nerf, hip.camera_rays(c2ws[0], fx, fx, RES / 2, RES / 2, RES, RES, out=rays), fx, noise=DeviceNoise(dev, seed=3),
                    keys=("rgb_map", "depth", "world_normal", "acc_map"))


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]                  # microseconds


us = timed(lambda: hip.camera_rays(c2ws[0], fx, fx, RES / 2, RES / 2, RES, RES, out=rays))
out["camera_rays_us"] = mmm(us)
out["camera_rays_TBps"] = round(24 * P / (st.median(us) * 1e-6) / 1e12, 3)
strip2 = torch.empty(RES, 2 * RES, 3, dtype=torch.uint8, device=dev)
us = timed(lambda: hip.frame_finish(RES, RES, rgb=ims["rgb_map"], depth=ims["depth"], near_far=(2.5, 7.0), out=strip2))
out["frame_finish_rgb_depth_us"] = mmm(us)
out["frame_finish_rgb_depth_TBps"] = round((16 + 6) * P / (st.median(us) * 1e-6) / 1e12, 3)       # reads 12 + 4, writes 3 + 3 bytes per pixel
strip4 = torch.empty(RES, 4 * RES, 3, dtype=torch.uint8, device=dev)
us = timed(lambda: hip.frame_finish(RES, RES, rgb=ims["rgb_map"], depth=ims["depth"], normal=ims["world_normal"], acc=ims["acc_map"],
                                    near_far=(2.5, 7.0), out=strip4))
out["frame_finish_4_panels_us"] = mmm(us)
out["frame_finish_4_panels_TBps"] = round((32 + 12) * P / (st.median(us) * 1e-6) / 1e12, 3)
pin = torch.empty(strip2.shape, dtype=torch.uint8).pin_memory()
out["d2h_strip_2_panels_us"] = mmm(timed(lambda: pin.copy_(strip2, non_blocking=True), reps=20))

rgb8 = strip2[:, :RES].cpu().numpy()
dep8 = strip2[:, RES:].cpu().numpy()
enc = {"rgb": [], "depth": []}
for _ in range(8):
    for name, a in (("rgb", rgb8), ("depth", dep8)):
        t = time.perf_counter()
        _png(os.path.join(tmp, "enc.png"), a)
        enc[name].append((time.perf_counter() - t) * 1e3)
out["png_encode_ms"] = {k: mmm(v) for k, v in enc.items()}

# the host route of a data-set frame: rays on the host (the loader), upload, float32 read-back, numpy quantisation
d = get_ray_directions(RES, RES, [fx, fx])
d = d / torch.norm(d, dim=-1, keepdim=True)
host = dict(get_rays=[], upload=[], readback_quantise=[])
for k in range(6):
    t = time.perf_counter()
    o, dd = get_rays(d, torch.from_numpy(c2ws[k % FRAMES]))
    r_host = torch.cat([o, dd], 1)
    host["get_rays"].append((time.perf_counter() - t) * 1e3)
    torch.cuda.synchronize()
    t = time.perf_counter()
    r_dev = r_host.to(dev)
    torch.cuda.synchronize()
    host["upload"].append((time.perf_counter() - t) * 1e3)
    rgb = ims["rgb_map"].reshape(RES, RES, 3)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a = (rgb.clamp(0, 1).cpu().numpy() * 255).astype("uint8")
    host["readback_quantise"].append((time.perf_counter() - t) * 1e3)
out["host_route_ms"] = {k: mmm(v[1:]) for k, v in host.items()}
out["rays_equal_host_route"] = float((r_dev[:, 3:] - hip.camera_rays(c2ws[5 % FRAMES], fx, fx, RES / 2, RES / 2, RES, RES, device=dev)[:, 3:]).abs().max())

shutil.rmtree(tmp, ignore_errors=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
