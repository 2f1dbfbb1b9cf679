"""Cost of scene composition, by HIP events: median (min / max) of 20 launches or frames after a warm-up.
usage: python tools/compose_bench.py [--reps 20] [--res 400] [--design DESIGN.md]
  kernels  nmf_rays_place, nmf_merge_rank and nmf_merge_scatter alone at 4096 rays, K = 2 lists of ~64 samples per ray
  frame    one RES x RES frame of bench.py's S1 model placed twice (identity and t=1.6,0.4,0;r=40,0,0;s=0.7) as a ComposedScene,
           against the sum of the two placements' own frames through the module path (fused_eval_pass = False), and the share of the
           composed frame spent in the three glue kernels (events around every call of them inside the frame)
One JSON line per measurement, then the table; --design splices the table between the compose_bench markers of that file."""
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
from nmf_amd import hip, synthetic  # noqa: E402
from nmf_amd.compose import ComposedScene, Placement  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.renderer import render_images  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--res", type=int, default=400)
ap.add_argument("--design", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
BEGIN, END = "<!-- compose_bench:begin -->", "<!-- compose_bench:end -->"


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


def report(name, what, t, unit="us", **extra):
    k = 1e3 if unit == "us" else 1.0
    rec = dict(name=name, what=what, **{f"{s}_{unit}": round(v * k, 2 if unit == "us" else 3) for s, v in zip(("median", "min", "max"), t)},
               **extra)
    print(json.dumps(rec), flush=True)
    rows.append(f"| {name} | {what} | {t[0] * k:.{1 if unit == 'us' else 2}f} {unit} ({t[1] * k:.{1 if unit == 'us' else 2}f} / "
                f"{t[2] * k:.{1 if unit == 'us' else 2}f}) |")


# ---- the three kernels alone ------------------------------------------------------------------------------------------------------------
B, K = 4096, 2
rng = np.random.default_rng(0)
P = Placement((40.0, 10.0, -5.0), (1.6, 0.4, 0.0), 0.7)
rays = torch.from_numpy(rng.normal(size=(B, 6)).astype(np.float32)).to(dev)
out = torch.empty_like(rays)
report("nmf_rays_place", f"{B} rays, world -> local", timed(lambda: hip.rays_place(rays, P, inverse=True, out=out)))
counts = rng.integers(32, 97, size=(K, B))
offsets = [torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev) for c in counts]
zs = [torch.from_numpy(np.concatenate([np.sort(rng.random(c) * 4 + 2) for c in counts[k]]).astype(np.float32)).to(dev) for k in range(K)]
M = int(counts.sum())
report("nmf_merge_rank", f"{B} rays, K = {K}, {M} samples", timed(lambda: hip.merge_rank(offsets, zs, [1.0, 0.7], B)))
dst, _ = hip.merge_rank(offsets, zs, [1.0, 0.7], B)
m0 = int(counts[0].sum())
f = dict(dtype=torch.float32, device=dev)
src = dict(sigma=torch.rand(m0, **f), dist=torch.rand(m0, **f), z=zs[0], normal=torch.rand(m0, 3, **f),
           ray_id=torch.zeros(m0, dtype=torch.int32, device=dev))
merged = dict(sigma=torch.zeros(M, **f), dist=torch.zeros(M, **f), z=torch.zeros(M, **f), normal=torch.zeros(M, 3, **f),
              ray_id=torch.zeros(M, dtype=torch.int32, device=dev), part=torch.zeros(M, dtype=torch.int32, device=dev),
              src=torch.zeros(M, dtype=torch.int32, device=dev))
report("nmf_merge_scatter", f"one list of {m0} samples, seven arrays", timed(lambda: hip.merge_scatter(dst[0], M, R=P.R, out=merged, **src)))

# ---- one frame --------------------------------------------------------------------------------------------------------------------------
torch.manual_seed(3)
nerf, _ = bench.build(dev)
nerf.eval()
nerf.fused_eval_pass = False
W, focal = synthetic.camera_rays(0, all_pixels=True, wh=args.res)
W = W.to(dev).contiguous()
places = [Placement.identity(), Placement.from_spec("t=1.6,0.4,0;r=40,0,0;s=0.7")]
scene = ComposedScene([(nerf, p) for p in places])
noise = DeviceNoise(dev, seed=11)
own = []
for k, p in enumerate(places):
    local = hip.rays_place(W, p, inverse=True)
    own.append(timed(lambda: render_images(nerf, local, focal, None, noise), warm=3))
    report(f"own frame {k}", f"{args.res} x {args.res}, part {k} alone, module path", own[-1], unit="ms")
frame = timed(lambda: render_images(scene, W, focal, None, noise), warm=3)
report("composed frame", f"{args.res} x {args.res}, both parts", frame, unit="ms", own_sum_ms=round(own[0][0] + own[1][0], 3),
       ratio_to_own_sum=round(frame[0] / (own[0][0] + own[1][0]), 3))

# the glue inside the frame: events around every call of the three wrappers
marks = []


def wrap(fn):
    def inner(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*a, **k)
        e1.record()
        marks.append((e0, e1))
        return r
    return inner


saved = {n: getattr(hip, n) for n in ("rays_place", "merge_rank", "merge_scatter")}
glue = []
try:
    for n, fn in saved.items():
        setattr(hip, n, wrap(fn))
    for _ in range(args.reps):
        marks.clear()
        render_images(scene, W, focal, None, noise)
        torch.cuda.synchronize()
        glue.append((sum(a.elapsed_time(b) for a, b in marks), len(marks)))
finally:
    for n, fn in saved.items():
        setattr(hip, n, fn)
g = [v for v, _ in glue]
report("glue in the frame", f"{glue[0][1]} calls of the three kernels per frame", (statistics.median(g), min(g), max(g)), unit="ms",
       share_of_frame=round(statistics.median(g) / frame[0], 4))
rows.append(f"| | composed frame / sum of own frames | {frame[0] / (own[0][0] + own[1][0]):.2f} |")
rows.append(f"| | glue / composed frame | {100 * statistics.median(g) / frame[0]:.1f} % |")

table = "\n".join(["| measurement | what | median (min / max) |", "|---|---|---|"] + rows)
print(table)
if args.design:
    text = open(args.design).read()
    i, j = text.index(BEGIN) + len(BEGIN), text.index(END)
    open(args.design, "w").write(text[:i] + "\n" + table + "\n" + text[j:])
