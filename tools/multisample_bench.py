"""Cost and grain of multi-sample frames, by HIP events: median (min / max) of 20 launches or frames after a warm-up.
usage: python tools/multisample_bench.py [--reps 20] [--res 400] [--design DESIGN.md]
  kernels   nmf_camera_rays_at, nmf_accum_update, nmf_accum_active and nmf_accum_resolve alone on a RES x RES frame
  frames    bench.py's S1 model from the S1 camera: one pass on the single-sample path (hip.camera_rays + render_images), then
            render_frame at 4 and 16 fixed samples and, with at most 16, adaptive at tol = 4, 2, 1 and 0.5 8-bit levels -- the frame time,
            the share rays_rendered / (16 H W) of the fixed-16 work and the mean standard error of the result (8-bit levels)
  grain     the mean standard error of a 2-pass frame times sqrt(2): the grain of a single-sample frame, in 8-bit levels
It asserts nothing about speed.  One JSON line per measurement, then the table; --design splices the table between the
multisample_bench markers of that file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nmf_amd import camera_path, hip, synthetic  # noqa: E402
from nmf_amd.multisample import FrameAccumulator, render_frame  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.renderer import render_images  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--res", type=int, default=400)
ap.add_argument("--design", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
BEGIN, END = "<!-- multisample_bench:begin -->", "<!-- multisample_bench:end -->"
RES = args.res
P = RES * RES


def timed(fn, n=args.reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


rows = []


def report(name, what, t, unit="us", note="", **extra):
    k = 1e3 if unit == "us" else 1.0
    rec = dict(name=name, what=what, **{f"{s}_{unit}": round(v * k, 2 if unit == "us" else 3) for s, v in zip(("median", "min", "max"), t)},
               **extra)
    print(json.dumps(rec), flush=True)
    d = 1 if unit == "us" else 2
    rows.append(f"| {name} | {what} | {t[0] * k:.{d}f} {unit} ({t[1] * k:.{d}f} / {t[2] * k:.{d}f}) | {note} |")


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------------
fx = 0.5 * RES / np.tan(0.5 * synthetic.CAMERA_ANGLE_X)
camera = dict(w=RES, h=RES, fx=fx, fy=fx, cx=RES / 2, cy=RES / 2, near_far=[2.5, 7.0])
c2w = camera_path.look_at((2.4, -2.8, 1.6), (0.0, 0.0, 0.0))
rng = np.random.default_rng(0)
f = dict(dtype=torch.float32, device=dev)
half = torch.from_numpy(np.flatnonzero(rng.random(P) < 0.5).astype(np.int32)).to(dev)
rays = torch.empty(P, 6, **f)
report("nmf_camera_rays_at", f"{RES} x {RES}, all pixels, hashed offset",
       timed(lambda: hip.camera_rays_at(c2w, fx, fx, RES / 2, RES / 2, RES, RES, jitter=(0.25, 0.75), seed=3, out=rays)))
report("nmf_camera_rays_at", f"a list of {half.numel()} pixels",
       timed(lambda: hip.camera_rays_at(c2w, fx, fx, RES / 2, RES / 2, RES, RES, jitter=(0.25, 0.75), seed=3, pix=half, out=rays)))
acc = FrameAccumulator(RES, RES, dev)
one = dict(rgb_lin=torch.rand(P, 3, **f), acc_map=torch.rand(P, **f), rgb_map=torch.rand(P, 3, **f), depth=torch.rand(P, **f),
           world_normal=torch.rand(P, 3, **f))
part = {k: v[: half.numel()].contiguous() for k, v in one.items()}
report("nmf_accum_update", f"{RES} x {RES}, all pixels, every map", timed(lambda: acc.update(one)))
report("nmf_accum_update", f"a list of {half.numel()} pixels", timed(lambda: acc.update(part, half)))
acc.reset()
for _ in range(4):
    acc.update({k: torch.rand_like(v) for k, v in one.items()})
med = float(acc.resolve(keys=())["se"].median())
report("nmf_accum_active", f"{RES} x {RES}, half of the pixels active, three launches, no read-back",
       timed(lambda: hip.accum_active(acc.state, RES, RES, 4, 16, med, out=acc._list, n_out=acc._n)))
report("FrameAccumulator.active", "the same with the read-back of the length", timed(lambda: acc.active(4, 16, med)))
report("nmf_accum_resolve", f"{RES} x {RES}, all six maps",
       timed(lambda: hip.accum_resolve(acc.state, RES, RES)))

# ---- frames -----------------------------------------------------------------------------------------------------------------------------
torch.manual_seed(3)
nerf, _ = bench.build(dev)
nerf.eval()
noise = DeviceNoise(dev, seed=11)
KEYS = ("rgb_map", "depth")


def single():
    hip.camera_rays(c2w, fx, fx, RES / 2, RES / 2, RES, RES, out=rays)
    return render_images(nerf, rays, float(fx), noise=noise, keys=KEYS)


t1 = timed(single, warm=3)
report("frame, spp 1", f"{RES} x {RES}, the single-sample path (camera_rays + render_images)", t1, unit="ms")
acc = FrameAccumulator(RES, RES, dev)
last = {}


def frame(**kw):
    def run():
        last["ims"], last["stats"] = render_frame(nerf, c2w, camera, noise=noise, keys=KEYS, accumulator=acc, **kw)
    return run


def se_levels():
    return float(last["ims"]["se"].mean()) * 255.0


t2 = timed(frame(spp=2, tol=None), warm=2)
grain = se_levels() * 2 ** 0.5
report("frame, spp 2", "fixed count", t2, unit="ms", note=f"mean se {se_levels():.3f} levels: single-sample grain {grain:.3f} levels",
       mean_se_levels=round(se_levels(), 4), single_sample_grain_levels=round(grain, 4))
fixed = {}
for spp in (4, 16):
    fixed[spp] = timed(frame(spp=spp, tol=None), warm=2)
    report(f"frame, spp {spp}", "fixed count", fixed[spp], unit="ms", note=f"mean se {se_levels():.3f} levels; {fixed[spp][0] / t1[0]:.2f} x spp 1",
           mean_se_levels=round(se_levels(), 4), ratio_to_spp_1=round(fixed[spp][0] / t1[0], 3))
host_ms = (fixed[16][0] - 16 * t1[0]) / 16
for levels in (4.0, 2.0, 1.0, 0.5):
    t = timed(frame(spp=16, min_spp=4, tol=levels / 255.0), warm=2)
    share = last["stats"]["rays_rendered"] / (16.0 * P)
    report(f"frame, adaptive {levels:g}", f"at most 16, at least 4, tol = {levels:g} / 255", t, unit="ms",
           note=f"{100 * share:.1f} % of the fixed-16 rays, {last['stats']['passes']} passes, mean se {se_levels():.3f} levels; "
                f"{t[0] / fixed[16][0]:.2f} x fixed 16",
           rays_share_of_fixed_16=round(share, 4), passes=last["stats"]["passes"], mean_se_levels=round(se_levels(), 4),
           ratio_to_fixed_16=round(t[0] / fixed[16][0], 3))
rows.append(f"| | (fixed 16 - 16 x spp 1) / 16: what a pass costs beyond a single-sample frame | {host_ms:.2f} ms | |")
print(json.dumps(dict(name="per-pass overhead", ms=round(host_ms, 3))), flush=True)

table = "\n".join(["| measurement | what | median (min / max) | |", "|---|---|---|---|"] + rows)
print(table)
if args.design:
    text = open(args.design).read()
    i, j = text.index(BEGIN) + len(BEGIN), text.index(END)
    open(args.design, "w").write(text[:i] + "\n" + table + "\n" + text[j:])
