"""Writes tv.npz: the reference's total-variation terms in float64 on small seeded fp32 inputs, with their autograd gradients.
    python tests/golden/make_tv_golden.py

Called: utils.TVLoss (utils.py:139-151) on planes and lines, IntegralEquirect.tv_loss (modules/integral_equirect.py:399-407) on
environment maps, TensorVMSplit.TV_loss_density / TV_loss_app (fields/tensoRF.py:342-360) on one whole field.

Cases (inputs are fp32 values; the reference is called on their float64 values):
  plane_C{c}_{h}x{w}   C in {1, 16, 24}, (H, W) in {(2,2), (3,5), (65,64), (130,67)}; plane_C16_65x64 holds a constant block
                       (zero differences: the term is sqrt(1e-5), its gradient 0).  The four cases with C > 1 and H >= 65 would
                       not fit a committed file as fp32 input + float64 gradient (6 MB): their inputs are multiples of 1/128 stored
                       as int8 (<name>_x int8, <name>_xscale = 128; many equal neighbours), their float64 value covers every
                       element, and their gradient is stored for the rows <name>_rows (first two, middle, last two) only
  line_C{c}_{g}        G in {2, 65, 300}; line_C16_65 holds runs of repeated values (sign(0) = 0 in the gradient)
  env_{h}x{w}          [1,3,8,16] and [1,3,5,130]
  field                G = 20, 16 density and 24 appearance components: the 1e-2 / 1e-3 factors
Keys: names; <name>_x (fp32, or int8 with <name>_xscale), <name>_kind ('plane' / 'line' / 'env'), <name>_value (float64 scalar), <name>_grad (float64);
field_dp{i} / field_dl{i} / field_ap{i} / field_al{i} (inputs), field_density_value, field_app_value and
field_g_dp{i} ... (gradient of TV_loss_density through the density tensors, of TV_loss_app through the appearance tensors; the
plane gradients for the rows field_rows only, the line gradients whole).
Only this generator imports the reference; the tests read the .npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.install_stubs()
from utils import TVLoss  # noqa: E402  (the reference's utils.py)
from fields.tensoRF import TensorVMSplit  # noqa: E402
from modules.integral_equirect import IntegralEquirect  # noqa: E402


def value_grad(fn, x32):
    x = torch.from_numpy(x32.astype(np.float64)).requires_grad_(True)
    v = fn(x)
    (g,) = torch.autograd.grad(v, x)
    return np.float64(v.item()), g.numpy()


def main():
    rng = np.random.default_rng(20241017)
    out, names = {}, []
    reg = TVLoss()

    def add(name, kind, x, fn):
        v, g = value_grad(fn, x)
        names.append(name)
        out[f"{name}_x"], out[f"{name}_kind"], out[f"{name}_value"], out[f"{name}_grad"] = x, np.array(kind), v, g

    for c in (1, 16, 24):
        for h, w in ((2, 2), (3, 5), (65, 64), (130, 67)):
            name = f"plane_C{c}_{h}x{w}"
            if c > 1 and h >= 65:
                q = rng.integers(-3, 4, size=(1, c, h, w)).astype(np.int8)
                if (c, h, w) == (16, 65, 64):
                    q[:, :, 20:41, 10:33] = 9
                x = q.astype(np.float32) / np.float32(128)
                v, g = value_grad(reg, x)
                rows = np.array([0, 1, h // 2, h - 2, h - 1])
                names.append(name)
                out[f"{name}_x"], out[f"{name}_xscale"], out[f"{name}_kind"] = q, np.float32(128), np.array("plane")
                out[f"{name}_value"], out[f"{name}_rows"], out[f"{name}_grad"] = v, rows, g[:, :, rows, :]
                continue
            x = (0.1 * rng.standard_normal((1, c, h, w))).astype(np.float32)
            add(name, "plane", x, reg)
        for g in (2, 65, 300):
            x = (0.1 * rng.standard_normal((1, c, g, 1))).astype(np.float32)
            if (c, g) == (16, 65):
                x[:, :, 10:30] = x[:, :, 10:11]
                x[:, 3] = np.float32(-0.5)
            add(f"line_C{c}_{g}", "line", x, reg)
    for h, w in ((8, 16), (5, 130)):
        x = (-0.6 + 0.3 * rng.standard_normal((1, 3, h, w))).astype(np.float32)
        if h == 8:
            x[:, :, 2:4, 3:9] = np.float32(-0.6)             # equal neighbours: sign(0) in both differences
        env = IntegralEquirect(bg_resolution=h, mipbias=1, activation="exp", lr=0.02, init_val=-0.6, mul_lr=0, brightness_lr=0,
                               betas=[0.9, 0.99], mul_betas=[0.9, 0.9], mipbias_lr=1e-4, mipnoise=0.0).double()
        xd = torch.from_numpy(x.astype(np.float64))
        env.bg_mat = torch.nn.Parameter(xd)
        v = env.tv_loss()
        (g,) = torch.autograd.grad(v, env.bg_mat)
        names.append(f"env_{h}x{w}")
        out[f"env_{h}x{w}_x"], out[f"env_{h}x{w}_kind"] = x, np.array("env")
        out[f"env_{h}x{w}_value"], out[f"env_{h}x{w}_grad"] = np.float64(v.item()), g.numpy()

    # one whole field: TV_loss_density / TV_loss_app with the reference's per-tensor factors
    G = 20
    rows = out["field_rows"] = np.array([0, 1, G // 2, G - 2, G - 1])
    rf = TensorVMSplit(aabb=torch.tensor([[-1.5] * 3, [1.5] * 3]), **rh.field_kwargs(G)).double()
    with torch.no_grad():
        for tag, f in (("d", rf.density_rf), ("a", rf.app_rf)):
            for i in range(3):
                for kind, plist in (("p", f.app_plane), ("l", f.app_line)):
                    x = (0.1 * rng.standard_normal(tuple(plist[i].shape))).astype(np.float32)
                    plist[i].copy_(torch.from_numpy(x.astype(np.float64)))
                    out[f"field_{tag}{kind}{i}"] = x
    for tag, f, loss in (("d", rf.density_rf, rf.TV_loss_density), ("a", rf.app_rf, rf.TV_loss_app)):
        ps = list(f.app_plane) + list(f.app_line)
        v = loss(reg)
        gs = torch.autograd.grad(v, ps)
        out["field_density_value" if tag == "d" else "field_app_value"] = np.float64(v.item())
        for i in range(3):
            out[f"field_g_{tag}p{i}"], out[f"field_g_{tag}l{i}"] = gs[i].numpy()[:, :, rows, :], gs[3 + i].numpy()
    out["names"] = np.array(names)
    path = os.path.join(HERE, "tv.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "cases")


if __name__ == "__main__":
    main()
