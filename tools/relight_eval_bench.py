"""Relighting evaluation costs: the three kernels of csrc/relight_eval.hip alone, and the protocol's metric phase
against its render phase.

    python tools/relight_eval_bench.py [--reps 20] [--frames 200] [--res 800] [--views 4] [--view-res 400]
HIP events, one warm-up, median (min / max) of --reps launches:
  kernels   nmf_relight_frame / nmf_relight_ratio / nmf_relight_adjust (with their reduction launch) on 1 and on --frames frames of
            --res x --res, buffers allocated once, called through the C ABI; with the bytes each must move (frame 28, ratio 28,
            adjust 52 per pixel) over the median, to set against the copy rate DESIGN.md 10.3 quotes
  protocol  relight_eval.relight_evaluation on bench.py's S1 model under a rotated map: --views orbit views of --view-res x --view-res
            against random linear RGBA ground truth held in memory; seconds of its render phase (render, HDR frame, EXR write) and
            of its metric phase (ratio, adjust, SSIM, PNG write)"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from nmf_amd import hip, relight, synthetic  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.relight_eval import relight_evaluation  # noqa: E402

BYTES_PER_PIXEL = dict(frame=12 + 4 + 12, ratio=12 + 16, adjust=12 + 16 + 12 + 12)


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


def kernels(n, res, reps, dev):
    """the three entry points on n frames of res x res, straight through the C ABI on buffers allocated once"""
    lib, p, st = hip._lib, hip._p, hip._stream
    g = torch.Generator(device=dev).manual_seed(n)
    pred = torch.rand((n, res, res, 3), generator=g, device=dev).mul_(4.0)
    gt = torch.rand((n, res, res, 4), generator=g, device=dev)
    gt[..., :3].mul_(4.0)
    acc = gt[..., 3].contiguous()
    out, out2 = torch.empty_like(pred), torch.empty_like(pred)
    sums = torch.empty((n, 3), dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.nmf_relight_ratio_workspace_bytes(n, res, res)), dtype=torch.uint8, device=dev)
    calls = dict(
        frame=lambda: hip._check(lib.nmf_relight_frame(p(pred), p(acc), n, res, res, p(out), st()), "nmf_relight_frame"),
        ratio=lambda: hip._check(lib.nmf_relight_ratio(p(pred), p(gt), n, res, res, p(sums), p(count), p(ws), ws.numel(), st()),
                                 "nmf_relight_ratio"),
        adjust=lambda: hip._check(lib.nmf_relight_adjust(p(pred), p(gt), 0.9, 1.1, 1.3, n, res, res, p(out), p(out2), p(sums), p(ws),
                                                         ws.numel(), st()), "nmf_relight_adjust"))
    rec = {}
    for name, fn in calls.items():
        t = events_us(fn, reps)
        nbytes = n * res * res * BYTES_PER_PIXEL[name]
        rec[name] = dict(us=t, megabytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / (t["median"] * 1e-6) / 1e12, 3))
    return rec


class MemoryViews:
    """what relight_evaluation reads of a stacked EXR test set, held in memory"""
    hdr = True

    def __init__(self, views, res, seed=2):
        rays, focal = synthetic.orbit_rays(views, res, seed=seed)
        self.all_rays, self.fx, self.img_wh = rays.reshape(views, -1, 6), focal, [res, res]
        g = torch.Generator().manual_seed(seed)
        self.gt = torch.rand((views, res, res, 4), generator=g)

    def get_linear(self, idx):
        return self.gt[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--view-res", type=int, default=400)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for n in (1, a.frames):
        print(json.dumps({f"kernels_{n}x{a.res}x{a.res}": kernels(n, a.res, a.reps, dev)}), flush=True)
        torch.cuda.empty_cache()

    nerf, _ = bench.build(dev, grid=128)
    nerf.eval()
    nerf.bg_module = relight.rotate_env(nerf.bg_module, relight.axis_angle((1, 2, 0.5), 0.9))
    ds = MemoryViews(a.views, a.view_res)
    with tempfile.TemporaryDirectory() as tmp:
        relight_evaluation(nerf, MemoryViews(1, a.view_res), os.path.join(tmp, "warm"), noise=DeviceNoise(dev, seed=11))
        res = relight_evaluation(nerf, ds, os.path.join(tmp, "out"), noise=DeviceNoise(dev, seed=11))
    print(json.dumps(dict(protocol=dict(views=a.views, res=a.view_res, render_seconds=round(res["seconds"]["render"], 4),
                                        metric_seconds=round(res["seconds"]["metrics"], 4), psnr=round(res["psnr"], 3),
                                        ssim=round(res["ssim"], 5), multiplier=res["multiplier"]))), flush=True)


if __name__ == "__main__":
    main()
