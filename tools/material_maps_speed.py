"""Cost of the material maps on one 800 x 800 frame of bench.py's model: the fused evaluation pass without maps, with the material
maps (render_images keys MATERIAL_KEYS: one appearance query + nmf_material_maps per chunk) and the operator-graph module path
(draw_debug=True).  One warm-up frame per mode, then `reps` rounds that alternate the three modes; prints per mode the median,
min and max ms per frame.
    python tools/material_maps_speed.py [reps] [mode ...]      (modes: plain maps module; default all three, reps 3)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
from nmf_amd import synthetic  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.renderer import MATERIAL_KEYS, render_images  # noqa: E402

args = sys.argv[1:]
reps = int(args.pop(0)) if args and args[0].isdigit() else 3
modes = args or ["plain", "maps", "module"]
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
nerf, _ = bench.build(dev)
nerf.eval()
rays, focal = synthetic.camera_rays(0, all_pixels=True, wh=bench.FRAME)
rays = rays.to(dev)
base = ("rgb_map", "acc_map", "depth", "world_normal")
kw = dict(plain=dict(keys=base), maps=dict(keys=base + MATERIAL_KEYS), module=dict(keys=base + MATERIAL_KEYS, draw_debug=True))


def frame(mode):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ims = render_images(nerf, rays, focal, None, DeviceNoise(dev, seed=11), **kw[mode])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, ims


times = {m: [] for m in modes}
out = {}
for m in modes:
    out[m] = frame(m)[1]
for _ in range(reps):
    for m in modes:
        times[m].append(frame(m)[0])
for m in modes:
    t = times[m]
    print(f"{m:7s}: median {statistics.median(t):8.1f} ms / frame  (min {min(t):8.1f}, max {max(t):8.1f}, {len(t)} frames, "
          f"{rays.shape[0]} rays)", flush=True)
if "maps" in out and "module" in out:
    for k in ("albedo", "roughness", "diffuse"):
        print(f"max |fused - module| {k}: {float((out['maps'][k] - out['module'][k]).abs().max()):.2e}")
if "maps" in out and "plain" in out:
    print("rgb_map equal with and without maps:", bool(torch.equal(out["maps"]["rgb_map"], out["plain"]["rgb_map"])))
