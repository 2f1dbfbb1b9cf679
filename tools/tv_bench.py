"""Total-variation terms on one MI355X, device events, warm-up, alternating rounds:
  (a) ONE nmf_tv_fwd_bwd launch (value + gradient) over the S1 model's 12 field tensors at 128^3 and 300^3, beside the torch
      autograd evaluation of the CPU expression (utils.tv_reference) moved to the GPU, forward + backward, on the same tensors;
  (b) Trainer.step at bench.py's default shape with the TV weights 0 and with TV_weight_density=0.1, TV_weight_app=0.01,
      the two trainers alternating in blocks of steps.
    python tools/tv_bench.py [--rounds 7] [--reps 50] [--block 40] [--skip-step]
Prints one JSON line per leg: medians with (min, max) over the rounds."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from nmf_amd import hip  # noqa: E402
from nmf_amd.noise import DeviceNoise  # noqa: E402
from nmf_amd.trainer import Trainer, tv_table  # noqa: E402
from nmf_amd.utils import tv_reference  # noqa: E402


def timed_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def mmm(xs):
    return [round(statistics.median(xs), 3), round(min(xs), 3), round(max(xs), 3)]


def leg_a(dev, grid, rounds, reps):
    nerf, _ = bench.build(dev, grid=grid)
    ts, kinds, ws = tv_table(nerf, 0.1, 0.01, 0.0)
    grads = [torch.zeros_like(t, memory_format=torch.preserve_format) for t in ts]
    leaves = [t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in ts]

    def kernel():
        hip.tv_value_grad(ts, kinds, ws, 1.0, grads=grads)

    def eager():
        v = sum(tv_reference(x) * w for x, w in zip(leaves, ws))
        torch.autograd.grad(v, leaves)

    for _ in range(3):
        kernel(); eager()
    torch.cuda.synchronize()
    k, e = [], []
    for _ in range(rounds):
        k.append(timed_us(kernel, reps))
        e.append(timed_us(eager, max(reps // 10, 3)))
    elems = sum(t.numel() for t in ts)
    med = statistics.median(k)
    print(json.dumps(dict(leg="a", grid=grid, tensors=len(ts), elements=elems, mb_moved=round(12e-6 * elems, 1),
                          kernel_us=mmm(k), torch_autograd_us=mmm(e), tb_per_s=round(12.0 * elems / med * 1e-6, 3))), flush=True)


def leg_b(dev, rounds, block):
    trainers = []
    for extra in ({}, dict(TV_weight_density=0.1, TV_weight_app=0.01)):
        nerf, params = bench.build(dev)
        tr = Trainer(nerf, dict(params, **extra))
        batches, focal = bench.make_batches(nerf, 16, bench.CHUNK, 0, dev, distinct=16)
        trainers.append((tr, batches, focal, DeviceNoise(dev, seed=1)))

    def run(i, n):
        tr, batches, focal, noise = trainers[i]
        for j in range(n):
            tr.step(*batches[j % len(batches)], focal, noise=noise, update_controllers=False, fixed_chunk=bench.CHUNK)

    for i in (0, 1):
        run(i, bench.STARTUP_STEPS)
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(rounds):
        for i in (0, 1):
            run(i, 5)
            ms[i].append(timed_us(lambda: run(i, 1), block) / 1e3)
    print(json.dumps(dict(leg="b", rays=bench.CHUNK, tv_off_ms=mmm(ms[0]), tv_on_ms=mmm(ms[1]),
                          operator_graph_forwards=trainers[1][0].nerf.operator_graph_forwards)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    for grid in (128, 300):
        leg_a(dev, grid, a.rounds, a.reps)
    if not a.skip_step:
        leg_b(dev, a.rounds, a.block)


if __name__ == "__main__":
    main()
