"""Writes metrics.npz: SSIM of the reference's utils.rgb_ssim (utils.py:90-136, float64 scipy convolutions) on fp32 images.
    python tests/golden/make_metrics_golden.py

Cases (images stored as fp32; the reference is called on their float64 values, so x^2 / xy are exact as in nmf_ssim):
  rand_HxW      smooth random images and a noisy copy, odd / even / non-square sizes down to the minimum 11 x 11
  quant8        an 8-bit-quantised prediction floor(clip(x) * 255) / 255 against its ground truth (renderer.py:399-404)
  identical     an image against itself (SSIM 1)
  constant      two constant images (variances 0: only the luminance term)
  gt_outside    ground truth with values outside [0, 1] (the reference does not clip gt_rgb for SSIM)
Keys: names, <name>_a, <name>_b, <name>_ssim (float64 scalar); map_<MAP_CASE> is the full map of one case.
Only this generator imports the reference; the tests read the .npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.install_stubs()
from utils import rgb_ssim  # noqa: E402  (the reference's utils.py)

MAP_CASE = "rand_33x20"


def smooth(rng, h, w):
    """a low-frequency field plus fine noise in [0, 1]"""
    y, x = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(3):
            kx, ky, ph = rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5), rng.uniform(0, 2 * np.pi)
            f[..., c] += np.sin(kx * x + ky * y + ph)
    f = 0.5 + 0.15 * f + 0.05 * rng.standard_normal((h, w, 3))
    return np.clip(f, 0, 1).astype(np.float32)


def main():
    rng = np.random.default_rng(20240611)
    cases = {}
    for h, w in ((11, 11), (12, 12), (13, 17), (33, 20), (48, 64), (64, 48)):
        a = smooth(rng, h, w)
        b = np.clip(a + 0.08 * rng.standard_normal(a.shape), 0, 1).astype(np.float32)
        cases[f"rand_{h}x{w}"] = (a, b)
    gt = smooth(rng, 40, 36)
    pred = np.clip(gt + 0.05 * rng.standard_normal(gt.shape), -0.1, 1.1).astype(np.float32)
    cases["quant8"] = ((np.floor(np.clip(pred, 0, 1) * 255) / 255).astype(np.float32), gt)
    a = smooth(rng, 25, 30)
    cases["identical"] = (a, a.copy())
    cases["constant"] = (np.full((16, 21, 3), 0.5, np.float32), np.full((16, 21, 3), 0.3, np.float32))
    a = smooth(rng, 27, 24)
    cases["gt_outside"] = (a, (1.4 * a - 0.2 + 0.1 * rng.standard_normal(a.shape)).astype(np.float32))

    out = {"names": np.array(list(cases))}
    for name, (a, b) in cases.items():
        out[f"{name}_a"], out[f"{name}_b"] = a, b
        out[f"{name}_ssim"] = np.float64(rgb_ssim(a.astype(np.float64), b.astype(np.float64), 1))
        print(f"{name:12s} {a.shape} ssim {out[f'{name}_ssim']:.15f}")
    a, b = cases[MAP_CASE]
    out[f"map_{MAP_CASE}"] = rgb_ssim(a.astype(np.float64), b.astype(np.float64), 1, return_map=True)
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
