"""Error and cost of denoised frames on bench.py's S1 model at RES x RES, by HIP events: median (min / max) of 20
launches after a warm-up.
usage: python tools/denoise_bench.py [--reps 20] [--res 400] [--ref-spp 256] [--design DESIGN.md]
  reference the undenoised mean of --ref-spp jittered passes (render_frame without denoise: the path of DESIGN 10.11)
  error     RMSE of the displayed colour against the reference, in 8-bit levels, over the pixels whose reference se is above 0:
            raw frames of 2, 4 and 16 samples, and the SAME 2- and 4-sample states through FrameAccumulator.denoise for k_c in
            {1, 2, 4, 8} and levels in {3, 5} (the other widths at their defaults); the raw sample count a denoised 4-sample frame
            matches, from the raw errors' 1 / sqrt(n) law
  cost      nmf_denoise_prepare, nmf_denoise_level at steps 1 to 16 and nmf_denoise_finish alone, and nmf_denoise as a whole at the
            defaults and at five levels, against one rendering pass of the same frame
It asserts nothing about speed.  One JSON line per measurement, then the table; --design splices the table between the denoise_bench
markers of that file."""
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
from nmf_amd.multisample import DenoiseParams, FrameAccumulator, render_frame  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--res", type=int, default=400)
ap.add_argument("--ref-spp", type=int, default=256)
ap.add_argument("--design", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
BEGIN, END = "<!-- denoise_bench:begin -->", "<!-- denoise_bench:end -->"
RES = args.res
P = RES * RES
rows = []


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


def row(name, what, value, note="", **rec):
    print(json.dumps(dict(name=name, what=what, **rec)), flush=True)
    rows.append(f"| {name} | {what} | {value} | {note} |")


fx = 0.5 * RES / np.tan(0.5 * synthetic.CAMERA_ANGLE_X)
camera = dict(w=RES, h=RES, fx=fx, fy=fx, cx=RES / 2, cy=RES / 2, near_far=[2.5, 7.0])
c2w = camera_path.look_at((2.4, -2.8, 1.6), (0.0, 0.0, 0.0))
torch.manual_seed(3)
nerf, _ = bench.build(dev)
nerf.eval()
noise = DeviceNoise(dev, seed=11)
KEYS = ("rgb_map", "depth", "world_normal")

# ---- the error ------------------------------------------------------------------------------------------------------------------------
ref, _ = render_frame(nerf, c2w, camera, spp=args.ref_spp, tol=None, noise=noise, keys=KEYS)
sel = ref["se"] > 0
ref8 = ref["rgb_map"].clamp(0, 1)[sel].double() * 255.0


def rmse(rgb):
    return float(((rgb.clamp(0, 1)[sel].double() * 255.0 - ref8) ** 2).mean().sqrt())


row("reference", f"{args.ref_spp} spp, undenoised", f"{int(sel.sum())} of {P} pixels with se > 0",
    f"its own mean se {float(ref['se'][sel].mean()) * 255:.3f} levels", pixels=int(sel.sum()), mean_se_levels=round(float(ref["se"][sel].mean()) * 255, 4))
acc = FrameAccumulator(RES, RES, dev)
raw, best = {}, {}
for spp in (2, 4, 16):
    ims, _ = render_frame(nerf, c2w, camera, spp=spp, tol=None, noise=noise, keys=KEYS, accumulator=acc)
    raw[spp] = rmse(ims["rgb_map"])
    row(f"raw, {spp} spp", "RMSE against the reference", f"{raw[spp]:.3f} levels", rmse_levels=round(raw[spp], 4))
    if spp == 16:
        continue
    for levels in (3, 5):
        for k_c in (1.0, 2.0, 4.0, 8.0):
            prm = DenoiseParams(levels=levels, k_c=k_c)
            e = rmse(acc.denoise(prm, noclip=bool(getattr(nerf, "hdr", False)))["rgb_map"])
            if spp not in best or e < best[spp][0]:
                best[spp] = (e, prm)
            row(f"denoised, {spp} spp", f"levels {levels}, k_c {k_c:g}", f"{e:.3f} levels", f"{e / raw[spp]:.2f} x raw {spp} spp",
                rmse_levels=round(e, 4), ratio_to_raw=round(e / raw[spp], 4), levels=levels, k_c=k_c)
# the raw error falls as c / sqrt(n) (+ the reference's own error, below 1 / 16 of a single sample's): c from the 4-sample frame
for spp in (2, 4):
    e, prm = best[spp]
    n_eq = spp * (raw[spp] / e) ** 2
    row(f"best at {spp} spp", f"levels {prm.levels}, k_c {prm.k_c:g}", f"{e:.3f} levels",
        f"the error of a raw frame of {n_eq:.1f} samples (raw {spp} spp: {raw[spp]:.3f}, raw 16 spp: {raw[16]:.3f})",
        rmse_levels=round(e, 4), equivalent_raw_spp=round(n_eq, 2), levels=prm.levels, k_c=prm.k_c)

# ---- the cost -------------------------------------------------------------------------------------------------------------------------
d = DenoiseParams()
w = (d.k_c, d.k_n, d.k_z, d.eps_z, d.k_a)
ws = torch.empty(hip.denoise_workspace_bytes(RES, RES) // 4, dtype=torch.float32, device=dev)
out = dict(rgb_map=torch.empty(P, 3, device=dev))


def us(t):
    return f"{t[0] * 1e3:.1f} us ({t[1] * 1e3:.1f} / {t[2] * 1e3:.1f})"


t = timed(lambda: hip.denoise_prepare(acc.state, ws, RES, RES))
row("nmf_denoise_prepare", f"{RES} x {RES}", us(t), median_us=round(t[0] * 1e3, 2), min_us=round(t[1] * 1e3, 2), max_us=round(t[2] * 1e3, 2))
for l in range(5):
    t = timed(lambda: hip.denoise_level(acc.state, ws, RES, RES, 1 << l, l & 1, *w))
    row("nmf_denoise_level", f"step {1 << l}", us(t), f"{25 * 12 * 4 * P / (t[0] * 1e-3) / 1e9:.0f} GB/s of tap loads (25 taps x 12 planes)",
        step=1 << l, median_us=round(t[0] * 1e3, 2), min_us=round(t[1] * 1e3, 2), max_us=round(t[2] * 1e3, 2))
t = timed(lambda: hip.denoise_finish(ws, RES, RES, 1, out=out))
row("nmf_denoise_finish", "rgb_map only", us(t), median_us=round(t[0] * 1e3, 2), min_us=round(t[1] * 1e3, 2), max_us=round(t[2] * 1e3, 2))
t_all = {n: timed(lambda: hip.denoise(acc.state, RES, RES, n, *w, workspace=ws, out=out)) for n in sorted({d.levels, 5})}
rays = torch.empty(P, 6, device=dev)


def one_pass():
    from nmf_amd.renderer import render_images
    hip.camera_rays(c2w, fx, fx, RES / 2, RES / 2, RES, RES, out=rays)
    return render_images(nerf, rays, float(fx), noise=noise, keys=KEYS)


t_pass = timed(one_pass, warm=3)
for n, t in t_all.items():
    row("nmf_denoise", f"prepare, {n} levels, finish" + (" (the defaults)" if n == d.levels else ""), us(t),
        f"{100 * t[0] / t_pass[0]:.2f} % of one rendering pass ({t_pass[0]:.1f} ms)", levels=n, median_us=round(t[0] * 1e3, 2),
        pass_ms=round(t_pass[0], 3), share_of_a_pass=round(t[0] / t_pass[0], 5))

table = "\n".join(["| measurement | what | value | |", "|---|---|---|---|"] + rows)
print(table)
if args.design:
    text = open(args.design).read()
    i, j = text.index(BEGIN) + len(BEGIN), text.index(END)
    open(args.design, "w").write(text[:i] + "\n" + table + "\n" + text[j:])
