"""Timing of the evaluation metrics (nmf_amd/csrc/metrics.hip): `hip.ssim` over N views of H x W in one call and view by
view, `hip.normal_err` over the same views, next to the float64 NumPy restatement of SSIM (tests/test_metrics_cpu.py) on one
view on the host.  Prints one JSON line.

    python tools/metrics_bench.py [--views 200] [--res 800] [--reps 3]
    rocprofv3 --kernel-trace --stats -d OUT -o metrics -- python tools/metrics_bench.py     (per-kernel device time)

Bytes per view of the SSIM kernels: both images read once (2 x H x W x 3 x 4 B; halo re-reads come from L2) plus one fp64
partial per 16 x 32 tile; the map is not written here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from nmf_amd import hip  # noqa: E402


def timed(fn, reps):
    """device ms per call (HIP events around `reps` calls after one warm-up)"""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args(argv)
    n, H = args.views, args.res
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand(n, H, H, 3, device=dev, generator=g)
    pred = (torch.floor((gt + 0.05 * torch.randn(gt.shape, device=dev, generator=g)).clip(0, 1) * 255) / 255).contiguous()
    rec = dict(views=n, res=H)
    ms = timed(lambda: hip.ssim(pred, gt), args.reps)
    rec["ssim_batched_ms_per_view"] = round(ms / n, 4)
    k = min(n, 16)
    ms1 = timed(lambda: [hip.ssim(pred[i], gt[i]) for i in range(k)], args.reps)
    rec["ssim_single_ms_per_view"] = round(ms1 / k, 4)
    bytes_per_view = 2 * H * H * 3 * 4
    rec["ssim_input_bytes_per_view"] = bytes_per_view
    rec["ssim_batched_input_TBps"] = round(bytes_per_view / (ms / n * 1e-3) / 1e12, 3)
    nrm = torch.nn.functional.normalize(gt.reshape(n, -1, 3) - 0.5, dim=-1)
    nrm2 = torch.nn.functional.normalize(pred.reshape(n, -1, 3) - 0.5, dim=-1)
    acc = gt[..., 0].reshape(n, -1).contiguous()
    msn = timed(lambda: hip.normal_err(nrm2, nrm, acc), args.reps)
    rec["normal_err_batched_ms_per_view"] = round(msn / n, 4)
    if not args.no_numpy:
        from test_metrics_cpu import ssim_np
        p0, g0 = pred[0].cpu().numpy(), gt[0].cpu().numpy()
        t0 = time.perf_counter()
        ref = ssim_np(p0, g0)
        rec["numpy_float64_ms_one_view"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["abs_diff_view0"] = abs(float(hip.ssim(pred[0], gt[0])[0]) - ref)
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    main()
