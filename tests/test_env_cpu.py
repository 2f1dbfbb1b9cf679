"""The environment map (csrc/env.hip) without a GPU: the inputs, the float64 references, the fp32 restatements and the margins that
the GPU tests (tests/test_hip_env.py) hold nmf_sat_build / _build_bwd / _lookup_fwd / _lookup_bwd / _lookup_bwd_binned to -- and the
tests that show that the inputs reach every branch they are named for and that the margins are not blind.

Maps are (H, W) = (16, 32), (32, 64), (48, 96), (64, 128); (80, 160) for the build alone.  (48, 96) is 2 x 2 tiles of 32 x 64 that
are partial in both directions and a W scan with a partial second 64-chunk, (80, 160) an H scan with a partial second and a W scan
with a partial third chunk, (16, 32) one partial tile that the full batch fills with more than ENV_ITEM = 4096 corner records and
the only map on which the combos 5 and 8 (pole wrap + left-seam wrap, sw > 2) can occur.

Lookups are drawn in (cx, cy, sa): a quarter with |cx| in [0.9, 1] (the table seam, a > 0, b ~ 0), a quarter with |cy| within 0.15
below the pole cutoff 1 - 6 / H, sa uniform in [-12, 8], mipbias 0.25, ~6000 per map plus 200 above the cutoff (pole rows, d_pole).
Every gate -- x1 - 1, x0 + 1 (also of the rotated pole boxes), y1 - 1, y0 + 1, x0 (rotation), y1 - 1.5, y0 + 1.5 (the clip of
`over`), |cy| - cutoff, both mip levels against 0 and 7 on the UNCLAMPED level, and the fractional texel coordinate of every
unclipped corner of every box (the bilinear kink) -- is CLEAR = 1e-3 away in float64 on the fp32 inputs; lookups that are not are
dropped, not moved.  test_inputs_reach_every_branch asserts the reject cap (5 %), >= 64 lookups per reachable combo and per side
of the `over` clip, of both mip clamps and of the rotation choice.

References: oracle.env_lookup on doubles with the fp32 table as doubles (values; d_dirs, d_sat, per-lookup d_mip -- an [R] mipbias
-- and d_pole by autograd); exp, float64-carried prefix sums rounded per element, pole means and the reverse sums for the build.
Restatement32: lookup_model() in float32 -- the oracle's own operations in its own order (test_model_is_the_oracle: bit for bit)
with the faults below as switches --, the table scatter as a sequential fp32 np.add.at in lookup order, the d_mip total in the
kernel's order (64-lane tree, four wave partials, workgroups in index order).

Metrics are in table units: |got - want| * size / 1000 for values, * size * norm2d / 1000 for d_dirs, each per footprint class
(size < 1, 1 .. 16, > 16 texels); margins are margins() of tests/test_shading_rows_cpu.py (8 x the restatement's error, at least
2^-23 x the largest |reference|), for a d_mip total max(8 |sum e_r|, sum |e_r|, 2^-23 sum |term_r|) over the per-lookup errors e_r.

A second restatement, dual_restatement32(), restates the dual-number role itself (csrc/dual.hpp: env_geometry, box_wrap and the
taps on a value and four tangents in fp32) in its two orders: "direct" (k_env_lookup_bwd: three channels, contracted with d_out at
the end) and "binned" (env_role_dirs: SumAccQ contracts the channels before the taps).  The kernels' d_dirs and d_mip are held to
IT, in the order of the path they took, with the same factor 8: forward mode rounds every product (tangent of a tap weight) x
(table entry ~ |SAT|) before the four taps cancel, reverse mode in fp32 differences the taps first, so the first restatement's
d_dirs is 3 to 57 times closer to float64 than the kernels' arithmetic can be.  On the GPU the kernels land at 0.3 .. 2.2 x the
second restatement (about half of their d_dirs elements are its bits), at 6 .. 58 x the first.

The restatements' largest errors against float64 on the full batches (test_restatement_table prints them), in units of
2^-23 max|SAT| for the scaled metrics (per class <1 / 1..16 / >16), error / scale for the sums:
    H    values             d_dirs, autograd   d_dirs, direct     d_dirs, binned     d_mip    d_sat               d_pole
                                                                                     /lookup
    16   2.0 / 1.7 / 14     4.3 / 3.3 / 24     29 / 11 / 191      25 / 27 / 208      43.0     4.7e-02 / 1.9e+04   2.3e-06 / 1.3e+01
    32   1.8 / 1.6 / 6.0    12 / 11 / 20       38 / 30 / 372      46 / 47 / 531      8.6      6.8e-02 / 7.9e+03   3.9e-06 / 3.0e+01
    48   1.9 / 2.2 / 3.6    18 / 21 / 12       53 / 105 / 215     133 / 150 / 676    6.8      1.0e-01 / 6.9e+03   6.0e-06 / 1.8e+01
    64   2.6 / 2.2 / 2.4    24 / 22 / 15       91 / 154 / 320     104 / 415 / 802    4.2      9.4e-02 / 5.2e+03   3.5e-06 / 2.2e+01

Faults (test_faults_miss_their_margins; each leaves its metric outside the margin on these inputs): right-seam wrap box dropped,
rot sign flipped, `over` clipped at 1.0, pole cutoff 4 / H, pole rows swapped, mip clamp at 8, tangent of a clipped corner kept,
extra boxes divided by their own size (values / d_pole / d_mip / d_dirs as named there); activation gate >= and d_pole / H (d_bg).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import nmf_oracle as O
from test_shading_rows_cpu import CLEAR, FLOOR, _big, errors_over, margins

F32, F64 = np.float32, np.float64
MAPS = ((16, 32), (32, 64), (48, 96), (64, 128))
BUILD_MAPS = MAPS + ((80, 160),)
MIPBIAS = 0.25
BRIGHT, MUL = F32(0.3), F32(0.8)                 # the fp32 values the kernels get
BRIGHT2, MUL2 = F32(4.0), F32(0.5)               # the clip set: 4 + 0.5 * 32 == 20 exactly
N_DRAW, N_POLE = 6000, 200
SHAPES = (1, 31, 32, 33, 255, 256, 257)
CLASSES = ("<1", "1..16", ">16")
FAULTS = ("no_right", "rot", "over1", "cutoff2", "pole_swap", "mip8", "tangent", "own_size")
TILE_H, TILE_W, ENV_ITEM = 32, 64, 4096          # csrc/env.hip


def _ro(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def _t(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype))


# ---- build: float64 and fp32 --------------------------------------------------------------------------------------------------------
def sat_from_act(act):
    """k_sat_cols / k_sat_rows on a given fp32 activation: act / 1000 in fp32, float64 running sums down H rounded to fp32 per
    element, then across W -> [3, H, W] float32"""
    v = (act / F32(1000)).astype(F32)
    v = np.cumsum(v.astype(F64), axis=1).astype(F32)
    return np.cumsum(v.astype(F64), axis=2).astype(F32)


def build_reference64(bg, brightness, mul):
    """act = exp(min(x, 20)), x = brightness + mul bg in float64 on the fp32 inputs; pole-row means of it"""
    x = F64(brightness) + F64(mul) * bg.astype(F64)
    act = np.exp(np.minimum(x, 20.0))
    return {"act": act, "pole": np.stack([act[:, 0].mean(-1), act[:, -1].mean(-1)])}


def build_restatement32(bg, brightness, mul):
    x = (F32(brightness) + (F32(mul) * bg).astype(F32)).astype(F32)
    act = np.exp(np.minimum(x, F32(20)).astype(F64)).astype(F32)          # a correctly rounded expf
    pole = np.stack([act[:, 0].astype(F64).mean(-1), act[:, -1].astype(F64).mean(-1)]).astype(F32)
    return {"act": act, "sat": sat_from_act(act), "pole": pole, "x": x}


def _planar(d_sat4):
    return np.ascontiguousarray(np.moveaxis(d_sat4[..., :3], -1, 0))


def build_bwd_reference64(d_sat4, bg, act, d_pole, brightness, mul):
    """d_bg = (reverse cumsum over W, then over H, of d_sat / 1000 + d_pole / W on rows 0 and H - 1) act mul where x <= 20"""
    H, W = bg.shape[-2:]
    d = _planar(d_sat4).astype(F64)
    d = np.flip(np.cumsum(np.flip(d, 2), axis=2), 2)
    d = np.flip(np.cumsum(np.flip(d, 1), axis=1), 1) / 1000.0
    d[:, 0] += d_pole.astype(F64)[0][:, None] / W
    d[:, H - 1] += d_pole.astype(F64)[1][:, None] / W
    x = F64(brightness) + F64(mul) * bg.astype(F64)
    return np.where(x <= 20.0, d * act.astype(F64) * F64(mul), 0.0)


def build_bwd_restatement32(d_sat4, bg, act, d_pole, brightness, mul, fault=None):
    """k_sat_rows_rev / k_sat_cols_rev: float64 reverse sums rounded to fp32 per element (W, then H), / 1000.f, the pole adjoint
    / (float) W on rows 0 and H - 1, (da act) mul, zero where the fp32 x > 20.  fault: "gate_ge" (x >= 20), "pole_H" (/ H)"""
    H, W = bg.shape[-2:]
    d = _planar(d_sat4)
    d = np.flip(np.cumsum(np.flip(d, 2).astype(F64), axis=2), 2).astype(F32)
    d = (np.flip(np.cumsum(np.flip(d, 1).astype(F64), axis=1), 1).astype(F32) / F32(1000)).astype(F32)
    div = F32(H if fault == "pole_H" else W)
    d[:, 0] = d[:, 0] + (d_pole[0] / div)[:, None]
    d[:, H - 1] = d[:, H - 1] + (d_pole[1] / div)[:, None]
    x = (F32(brightness) + (F32(mul) * bg).astype(F32)).astype(F32)
    clipped = x >= F32(20) if fault == "gate_ge" else x > F32(20)
    return np.where(clipped, F32(0), ((d * act).astype(F32) * F32(mul)).astype(F32)).astype(F32)


@functools.lru_cache(maxsize=None)
def table(H):
    """bg = -0.6 + 0.7 randn [3, H, W] and what the build makes of it with brightness 0.3, mul 0.8, computed here in the kernels'
    rounding: act, sat [3, H, W], its interleaved copy sat4 [H, W, 4], pole [2, 3]; the clip set bg2 (brightness 4, mul 0.5) with 32
    texels each at x == 20, one float above, one float below (at32 / above / below: flat indices); read-only, built once"""
    W = dict(BUILD_MAPS)[H]
    rng = np.random.default_rng([19, H])
    bg = (-0.6 + 0.7 * rng.standard_normal((3, H, W))).astype(F32)
    own = build_restatement32(bg, BRIGHT, MUL)
    sat4 = np.zeros((H, W, 4), dtype=F32)
    sat4[..., :3] = np.moveaxis(own["sat"], 0, -1)
    bg2 = bg.copy()
    at = rng.permutation(3 * H * W)[:96]
    flat = bg2.reshape(-1)
    flat[at[:32]] = F32(32.0)
    flat[at[32:64]] = np.nextafter(F32(32.0), F32(64.0))                   # 32 + 2^-18: x == 20 + 2^-19, the float above 20
    flat[at[64:]] = F32(32.0) - F32(2.0 ** -18)                             # x == 20 - 2^-19, the float below 20
    return _ro(SimpleNamespace(H=H, W=W, bg=bg, act=own["act"], sat=own["sat"], sat4=sat4, pole=own["pole"], bg2=bg2,
                               at20=np.sort(at[:32]), above=np.sort(at[32:64]), below=np.sort(at[64:]),
                               d_sat_rand=np.concatenate([rng.standard_normal((H, W, 3)), np.zeros((H, W, 1))], -1).astype(F32),
                               d_pole_rand=rng.standard_normal((2, 3)).astype(F32)))


# ---- the lookup: one model, float64 or float32 ----------------------------------------------------------------------------------------
def lookup_model(sat, pole, dirs, sa, mip, fault=None):
    """oracle.env_lookup / env_mip_levels / _box_wrap / _box_lr / _box operation by operation on torch tensors of one dtype, with the
    pole rows given ([2, 3]: top, bottom) and mip an [R] tensor -> (vals [R, 3], info).  info: cx, cy, the unclamped mip levels, the
    rect, size, and `boxes`, the list of (combo, lookup indices, x0, x1, y0, y1 unclipped) in the order they are added.
    fault: one of FAULTS"""
    h, w = sat.shape[-2:]
    cos = (1 - dirs[:, 2] ** 2).clip(min=O.EPS).sqrt()
    d = h * w / (2 * math.pi ** 2 * cos).clip(min=O.EPS)
    area = ((d / 2).log() + sa.reshape(-1)).exp()
    hh = (area.clip(min=O.EPS).sqrt() * cos).clip(min=O.EPS)
    ww = area / hh
    mw_u = ww.log() / math.log(2) + mip
    mh_u = hh.log() / math.log(2) + mip
    top = 8 if fault == "mip8" else 7
    mw, mh = mw_u.clip(0, top), mh_u.clip(0, top)
    sw = 2 ** mw / h / 2
    sh = 2 ** mh / h
    offset = torch.stack([sw, sh], dim=-1).reshape(1, 1, -1, 2)
    size = (offset / 2 * torch.tensor([w, h]).reshape(1, 1, 1, 2)).prod(dim=-1).reshape(-1, 1)
    a, b, c = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    norm2d = torch.sqrt(a ** 2 + b ** 2)
    phi = O._SafeAtan2.apply(b, a)
    theta = O._SafeAtan2.apply(c, norm2d)
    coords = torch.cat([(phi % (2 * math.pi) - math.pi) / math.pi, -theta / math.pi * 2], dim=1)
    x = coords.reshape(1, 1, -1, 2)
    bl = x - offset / 2
    tr = x + offset / 2
    br = x + torch.stack([sw, -sh], dim=-1).reshape(1, 1, -1, 2) / 2
    tl = x + torch.stack([-sw, sh], dim=-1).reshape(1, 1, -1, 2) / 2
    boxes = []

    def box(bl, br, tl, tr, sz, idx, combo):
        def s(p):
            pc = p.clip(min=-1, max=1)
            if fault == "tangent":
                pc = p + (pc - p).detach()
            return TF.grid_sample(sat, pc, mode="bilinear", align_corners=True, padding_mode="zeros")
        boxes.append((combo, idx, (bl[0, 0, :, 0], tr[0, 0, :, 0], bl[0, 0, :, 1], tr[0, 0, :, 1])))
        if combo and fault == "own_size":
            sz = ((tr - bl) / 2 * torch.tensor([w, h]).reshape(1, 1, 1, 2)).prod(dim=-1).reshape(-1, 1)
        return (s(tr) + s(bl) - s(tl) - s(br)).reshape(3, -1).T / sz

    def box_lr(bl, br, tl, tr, sz, idx, v):
        vals = box(bl, br, tl, tr, sz, idx, 3 * v)
        ex = (tr[..., 0] > 1).reshape(-1)
        if ex.any() and fault != "no_right":
            bl_r, tl_r, tr_r, br_r = (p[0, 0, ex].clone().reshape(1, 1, -1, 2) for p in (bl, tl, tr, br))
            bl_r[..., 0] = -1.0
            tl_r[..., 0] = -1.0
            tr_r[..., 0] = tr_r[..., 0] - 2
            br_r[..., 0] = br_r[..., 0] - 2
            vals = vals.index_add(0, torch.where(ex)[0], box(bl_r, br_r, tl_r, tr_r, sz[ex], idx[ex], 3 * v + 1))
        ex = (bl[..., 0] < -1).reshape(-1)
        if ex.any():
            bl_l, tl_l, tr_l, br_l = (p[0, 0, ex].clone().reshape(1, 1, -1, 2) for p in (bl, tl, tr, br))
            bl_l[..., 0] = bl_l[..., 0] + 2
            tl_l[..., 0] = tl_l[..., 0] + 2
            tr_l[..., 0] = 1.0
            br_l[..., 0] = 1.0
            vals = vals.index_add(0, torch.where(ex)[0], box(bl_l, br_l, tl_l, tr_l, sz[ex], idx[ex], 3 * v + 2))
        return vals

    every = torch.arange(len(sw))
    vals = box_lr(bl, br, tl, tr, size, every, 0)
    lo, hi = (1.0, -1.0) if fault == "rot" else (-1.0, 1.0)
    cap = 1.0 if fault == "over1" else 0.5
    ex = (tl[..., 1] > 1).reshape(-1)
    if ex.any():
        tl_t, tr_t, bl_t, br_t = (p[0, 0, ex].clone().reshape(1, 1, -1, 2) for p in (tl, tr, bl, br))
        rot = torch.where(tl_t[..., 0] > 0, lo, hi)
        over = (tl_t[..., 1] - 1).clip(max=cap, min=0)
        tl_t = torch.stack([tl_t[..., 0] + rot, torch.ones_like(rot)], -1)
        tr_t = torch.stack([tr_t[..., 0] + rot, torch.ones_like(rot)], -1)
        bl_t = torch.stack([bl_t[..., 0] + rot, 1 - over], -1)
        br_t = torch.stack([br_t[..., 0] + rot, 1 - over], -1)
        vals = vals.index_add(0, torch.where(ex)[0], box_lr(bl_t, br_t, tl_t, tr_t, size[ex], every[ex], 1))
    ex = (bl[..., 1] < -1).reshape(-1)
    if ex.any():
        tl_b, tr_b, bl_b, br_b = (p[0, 0, ex].clone().reshape(1, 1, -1, 2) for p in (tl, tr, bl, br))
        rot = torch.where(tl_b[..., 0] > 0, lo, hi)
        over = (-1 - bl_b[..., 1]).clip(max=cap, min=0)
        bl_b = torch.stack([bl_b[..., 0] + rot, -torch.ones_like(rot)], -1)
        br_b = torch.stack([br_b[..., 0] + rot, -torch.ones_like(rot)], -1)
        tl_b = torch.stack([tl_b[..., 0] + rot, -1 + over], -1)
        tr_b = torch.stack([tr_b[..., 0] + rot, -1 + over], -1)
        vals = vals.index_add(0, torch.where(ex)[0], box_lr(bl_b, br_b, tl_b, tr_b, size[ex], every[ex], 2))
    cx, cy = coords[:, 0], coords[:, 1]
    rect = (bl[0, 0, :, 0], tr[0, 0, :, 0], bl[0, 0, :, 1], tr[0, 0, :, 1])
    vals = vals * 1000
    cutoff = 1 - 2 / h * (2 if fault == "cutoff2" else 3)
    top_row, bot_row = (pole[1], pole[0]) if fault == "pole_swap" else (pole[0], pole[1])
    vals = torch.where((cy > cutoff)[:, None], bot_row.expand_as(vals), vals)
    vals = torch.where((cy < -cutoff)[:, None], top_row.expand_as(vals), vals)
    info = SimpleNamespace(cx=cx, cy=cy, mw_u=mw_u, mh_u=mh_u, rect=rect, size=size[:, 0], norm2d=norm2d[:, 0], boxes=boxes,
                           cutoff=cutoff)
    return vals, info


def _model_np(m, dirs, sa, dtype, fault=None, d_out=None):
    """lookup_model on numpy inputs in float64 or float32 -> dict of numpy arrays (adjoints by autograd when d_out is given), info"""
    tt = torch.float64 if dtype == F64 else torch.float32
    sat = _t(m.sat, dtype)[None].requires_grad_(True)
    pole = _t(m.pole, dtype).requires_grad_(True)
    d = _t(dirs, dtype).requires_grad_(True)
    mip = torch.full((len(dirs),), MIPBIAS, dtype=tt, requires_grad=True)
    vals, info = lookup_model(sat, pole, d, _t(sa, dtype), mip, fault)
    out = {"values": vals.detach().numpy()}
    if d_out is not None:
        gd, gs, gp, gm = torch.autograd.grad((vals * _t(d_out, dtype)).sum(), [d, sat, pole, mip], allow_unused=True)
        z = lambda g, like: (torch.zeros_like(like) if g is None else g).numpy()      # noqa: E731
        out.update(d_dirs=z(gd, d), d_sat=z(gs, sat)[0], d_pole=z(gp, pole), dm=z(gm, mip))
    return out, info


def geometry64(m, dirs, sa):
    """what the conditioning and the classes are read from: lookup_model in float64 on the fp32 inputs -> namespace of numpy arrays:
    size, norm2d, cls (footprint class 0 / 1 / 2), mask (bit c: combo c is added), pole, gate (distance to the nearest gate), and the
    sides of the `over` clip, the mip clamps and the rotation choice"""
    with torch.no_grad():
        _, g = lookup_model(_t(m.sat, F64)[None], _t(m.pole, F64), _t(dirs, F64), _t(sa, F64),
                            torch.full((len(dirs),), MIPBIAS, dtype=torch.float64))
    n = lambda v: v.numpy()      # noqa: E731
    x0, x1, y0, y1 = (n(v) for v in g.rect)
    cy, mw, mh = n(g.cy), n(g.mw_u), n(g.mh_u)
    R = len(cy)
    wrap = (y1 > 1) | (y0 < -1)
    rot = np.where(x0 > 0, -1.0, 1.0)
    inf = np.full(R, np.inf)
    gate = np.minimum.reduce([np.abs(x1 - 1), np.abs(x0 + 1), np.abs(y1 - 1), np.abs(y0 + 1), np.abs(x0), np.abs(y1 - 1.5),
                              np.abs(y0 + 1.5), np.abs(np.abs(cy) - g.cutoff), np.abs(mw), np.abs(mw - 7), np.abs(mh), np.abs(mh - 7),
                              np.where(wrap, np.abs(x1 + rot - 1), inf), np.where(wrap, np.abs(x0 + rot + 1), inf)])
    mask = np.zeros(R, dtype=np.int64)
    for combo, idx, r in g.boxes:
        idx = n(idx)
        mask[idx] |= 1 << combo
        for k, v in enumerate(r):
            v = n(v)
            t = (v + 1) * ((m.W if k < 2 else m.H) - 1) / 2
            gate[idx] = np.minimum(gate[idx], np.where(np.abs(v) < 1, np.abs(t - np.round(t)), np.inf))
    size = n(g.size)
    pole = np.abs(cy) > g.cutoff
    return SimpleNamespace(size=size, norm2d=n(g.norm2d), cls=np.where(size < 1, 0, np.where(size <= 16, 1, 2)), mask=mask, pole=pole,
                           gate=gate, pole_gate=np.abs(np.abs(cy) - g.cutoff), cx=n(g.cx), cy=cy, over_top=y1 - 1, over_bot=-1 - y0,
                           mw_u=mw, mh_u=mh, x0=x0, wrap=wrap, n_boxes=np.array([bin(int(v)).count("1") for v in mask]))


def directions(cx, cy):
    phi, theta = (cx + 1) * np.pi, -cy * np.pi / 2
    return np.stack([np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi), np.sin(theta)], 1).astype(F32)


@functools.lru_cache(maxsize=None)
def lookups(H):
    """the full batch of a map: dirs [R, 3], sa [R], origins [R, 3], d_out and d_out_range [R, 3], the float64 geometry `g` of the
    kept lookups, and how many were drawn and dropped; float32, read-only, built once"""
    m = table(H)
    rng = np.random.default_rng([23, H])
    cutoff = 1 - 6 / H
    q = N_DRAW // 4
    cx = rng.uniform(-1, 1, N_DRAW)
    cy = rng.uniform(-cutoff, cutoff, N_DRAW)
    cx[:q] = rng.uniform(0.9, 1.0, q) * rng.choice([-1.0, 1.0], q)
    cy[q:2 * q] = (cutoff - rng.uniform(0, 0.15, q)) * rng.choice([-1.0, 1.0], q)
    cxp = rng.uniform(-1, 1, N_POLE)
    cyp = rng.uniform(cutoff, 1.0, N_POLE) * np.where(np.arange(N_POLE) % 2 == 0, 1.0, -1.0)
    dirs = directions(np.concatenate([cx, cxp]), np.concatenate([cy, cyp]))
    sa = rng.uniform(-12, 8, len(dirs)).astype(F32)
    g = geometry64(m, dirs, sa)
    drawn_pole = np.arange(len(dirs)) >= N_DRAW
    keep = np.where(g.pole | drawn_pole, g.pole_gate >= CLEAR, g.gate >= CLEAR)
    order = rng.permutation(np.nonzero(keep)[0])
    dirs, sa = dirs[order], sa[order]
    R = len(order)
    d_out = rng.standard_normal((R, 3)).astype(F32)
    d_out[rng.permutation(R)[:100]] = 0
    d_range = (d_out * (10.0 ** rng.uniform(-6, 0, R))[:, None]).astype(F32)
    return _ro(SimpleNamespace(H=H, R=R, dirs=dirs, sa=sa, origins=rng.standard_normal((R, 3)).astype(F32), d_out=d_out,
                               d_out_range=d_range, g=geometry64(m, dirs, sa), drawn=len(keep), dropped=int((~keep[:N_DRAW]).sum()),
                               dropped_pole=int((~keep[N_DRAW:]).sum())))


def _take(i, idx, d_out=None):
    g = SimpleNamespace(**{k: v[idx] for k, v in vars(i.g).items()})
    return SimpleNamespace(H=i.H, R=len(i.dirs[idx]), dirs=i.dirs[idx], sa=i.sa[idx], origins=i.origins[idx],
                           d_out=(i.d_out if d_out is None else d_out)[idx], g=g)


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, -1e-30, 0]], dtype=F32)


@functools.lru_cache(maxsize=None)
def batch(H, name):
    """"full" / "range" (the full batch under the two adjoints), "dense" (H = 16: 256 lookups with at least four extra boxes each),
    "axis" (the six unit axes and (1, -1e-30, 0) at sa = -6, 1, 6), or an integer: the first so many lookups of the full batch"""
    i = lookups(H)
    if name == "full":
        return _take(i, slice(None))
    if name == "range":
        return _take(i, slice(None), i.d_out_range)
    if name == "dense":
        return _take(i, np.nonzero((i.g.n_boxes >= 5) & ~i.g.pole)[0][:256])
    if name == "axis":
        dirs, sa = np.tile(AXES, (3, 1)), np.repeat(np.array([-6, 1, 6], dtype=F32), len(AXES))
        rng = np.random.default_rng([29, H])
        return SimpleNamespace(H=H, R=len(dirs), dirs=dirs, sa=sa, origins=rng.standard_normal((len(dirs), 3)).astype(F32),
                               d_out=rng.standard_normal((len(dirs), 3)).astype(F32), g=geometry64(table(H), dirs, sa))
    return _take(i, slice(0, int(name)))


def sub_batches(H):
    """name -> indices into the full batch: one class per combo, the lookups clamped at mip 0, at mip 7, at neither"""
    g = lookups(H).g
    live = ~g.pole
    out = {f"combo{c}": np.nonzero(live & ((g.mask >> c) & 1 == 1))[0] for c in range(1, 9)}
    lo, hi = (g.mw_u < 0) | (g.mh_u < 0), (g.mw_u > 7) | (g.mh_u > 7)
    out.update(clamp0=np.nonzero(live & lo)[0], clamp7=np.nonzero(live & hi)[0], unclamped=np.nonzero(live & ~lo & ~hi)[0])
    return {k: v for k, v in out.items() if len(v)}


# ---- references and restatements of a batch -------------------------------------------------------------------------------------------
def lookup_reference64(m, b):
    """oracle.env_lookup on doubles, the table the fp32 table as doubles, activated = exp(log act) so that the pole rows' means are
    the given activation's; adjoints by autograd -> values, d_dirs, d_sat [3, H, W], dm [R] (per lookup), d_pole [2, 3]"""
    act = _t(m.act, F64)
    x = act.log()[None].requires_grad_(True)
    sat = _t(m.sat, F64)[None].requires_grad_(True)
    d = _t(b.dirs, F64).requires_grad_(True)
    mip = torch.full((b.R,), MIPBIAS, dtype=torch.float64, requires_grad=True)
    sd = {"bg_module.bg_mat": x, "bg_module.mipbias": mip, "bg_module.brightness": torch.tensor(0.0, dtype=torch.float64),
          "bg_module.mul": torch.tensor(1.0, dtype=torch.float64)}
    vals = O.env_lookup(sd, d, _t(b.sa, F64), sat=sat)
    gd, gs, gm, gx = torch.autograd.grad((vals * _t(b.d_out, F64)).sum(), [d, sat, mip, x], allow_unused=True)
    z = lambda g, like: (torch.zeros_like(like) if g is None else g)      # noqa: E731
    gx = z(gx, x)[0]
    d_pole = torch.stack([(gx[:, 0] / act[:, 0]).sum(-1), (gx[:, -1] / act[:, -1]).sum(-1)])
    assert not bool(gx[:, 1:-1].any())
    return {"values": vals.detach().numpy(), "d_dirs": z(gd, d).numpy(), "d_sat": z(gs, sat)[0].numpy(), "dm": z(gm, mip).numpy(),
            "d_pole": d_pole.numpy()}


def scatter32(m, info, d_out):
    """the table adjoint as the kernels form it -- per corner of every box in the order they are added, g = d_out * (1000 / size),
    v = g * sign * (w | 1 - w), v (1 - n) on row y0 and v n on row y0 + 1 -- added sequentially in fp32 in lookup order -> [3, H, W]"""
    H, W = m.H, m.W
    size = info.size.detach().numpy()
    live = ~((info.cy.detach().numpy() > F32(info.cutoff)) | (info.cy.detach().numpy() < -F32(info.cutoff)))
    g = (d_out * (F32(1000) / size)[:, None]).astype(F32)
    look, key, flat, val = [], [], [], []
    for combo, idx, r in info.boxes:
        idx = idx.numpy()
        on = live[idx]
        idx = idx[on]
        x0, x1, y0, y1 = (np.clip(v.detach().numpy()[on], F32(-1), F32(1)) for v in r)
        for k, (x, y, sgn) in enumerate(((x1, y1, 1), (x0, y0, 1), (x0, y1, -1), (x1, y0, -1))):
            ix, iy = (x + F32(1)) * F32((W - 1) * 0.5), (y + F32(1)) * F32((H - 1) * 0.5)
            fx, fy = np.floor(ix), np.floor(iy)
            w, n = ix - fx, iy - fy
            for dy in (0, 1):
                for dx in (0, 1):
                    X, Y = fx.astype(np.int64) + dx, fy.astype(np.int64) + dy
                    v = (g[idx] * F32(sgn)) * (w if dx else F32(1) - w)[:, None]
                    v = (v * (n if dy else F32(1) - n)[:, None]).astype(F32)
                    ok = (X < W) & (Y < H)
                    look.append(idx[ok])
                    key.append(np.full(int(ok.sum()), combo * 16 + k * 4 + dy * 2 + dx))
                    flat.append((Y * W + X)[ok])
                    val.append(v[ok])
    look, key, flat, val = np.concatenate(look), np.concatenate(key), np.concatenate(flat), np.concatenate(val)
    order = np.lexsort((key, look))
    d = np.zeros((H * W, 3), dtype=F32)
    np.add.at(d, flat[order], val[order])
    return np.ascontiguousarray(d.reshape(H, W, 3).transpose(2, 0, 1)), len(look) // 4


def mip_total32(dm):
    """the d_mip total in the order of k_env_lookup_bwd: the 64-lane shuffle tree of each wave, the four wave partials of a
    workgroup of 256 lookups in order, the workgroups in index order"""
    n = -(-len(dm) // 256) * 256
    v = np.zeros(n, dtype=F32)
    v[:len(dm)] = dm
    v = v.reshape(-1, 4, 64)
    d = 32
    while d:
        up = np.zeros_like(v)
        up[..., :64 - d] = v[..., d:]
        v = v + up
        d //= 2
    total = F32(0)
    for wg in v[..., 0]:
        t = F32(0)
        for s in wg:
            t = F32(t + s)
        total = F32(total + t)
    return total


def lookup_restatement32(m, b, fault=None):
    own, info = _model_np(m, b.dirs, b.sa, F32, fault, b.d_out)
    own["d_sat"], own["records"] = scatter32(m, info, b.d_out)
    cy = info.cy.detach().numpy()
    dp = np.zeros((2, 3), dtype=F32)
    rows = np.where(cy < -F32(info.cutoff), 0, np.where(cy > F32(info.cutoff), 1, -1))
    if fault == "pole_swap":
        rows = np.where(rows >= 0, 1 - rows, rows)
    np.add.at(dp, rows[rows >= 0], b.d_out[rows >= 0])
    own["d_pole"] = dp
    own["d_mip"] = mip_total32(own["dm"])
    return own


# ---- the second restatement: the kernels' forward-mode dual numbers ---------------------------------------------------------------
class Dual:
    """csrc/dual.hpp on numpy float32: a value [n] and four tangents [n, 4] (d/da, d/db, d/dc, d/dmipbias), every operation rounded
    where the header rounds it (no fused multiply-add: the file is compiled with contraction off)"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v = np.asarray(v, dtype=F32)
        self.d = np.zeros(self.v.shape + (4,), dtype=F32) if d is None else d

    def __getitem__(self, i):
        return Dual(self.v[i], self.d[i])

    def __add__(self, o):
        return Dual(self.v + o.v, self.d + o.d) if isinstance(o, Dual) else Dual(self.v + F32(o), self.d)

    def __sub__(self, o):
        return Dual(self.v - o.v, self.d - o.d) if isinstance(o, Dual) else Dual(self.v - F32(o), self.d)

    def __rsub__(self, o):
        return Dual(F32(o) - self.v, -self.d)

    def __neg__(self):
        return 0.0 - self

    def __mul__(self, o):
        if isinstance(o, Dual):
            return Dual(self.v * o.v, self.d * o.v[:, None] + self.v[:, None] * o.d)
        o = np.asarray(o, dtype=F32)
        return Dual(self.v * o, self.d * (o[:, None] if o.ndim else o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Dual):
            q = self.v / o.v
            return Dual(q, (self.d - q[:, None] * o.d) / o.v[:, None])
        return Dual(self.v / F32(o), self.d / F32(o))


def _r32(f, *a):
    with np.errstate(all="ignore"):
        return f(*(np.asarray(x, dtype=F64) for x in a)).astype(F32)              # correctly rounded libm


def _un(a, v, dv):
    return Dual(v, a.d * dv[:, None])


def _dsqrt(a):
    r = np.sqrt(a.v)
    return _un(a, r, F32(0.5) / r)


def _dlog(a):
    return _un(a, _r32(np.log, a.v), F32(1) / a.v)


def _dexp(a):
    e = _r32(np.exp, a.v)
    return _un(a, e, e)


def _dpow2(a):
    p = _r32(np.exp2, a.v)
    return _un(a, p, p * F32(math.log(2)))


def _const(like, v):
    return Dual(np.full_like(like.v, v))


def _dclip(a, lo, hi=None):
    """d_clipmin / d_clip: outside the range the bound with zero tangents (on the bound the tangents pass, as torch.clamp's do)"""
    out = Dual(a.v.copy(), a.d.copy())
    low = a.v < F32(lo)
    out.v[low], out.d[low] = F32(lo), 0
    if hi is not None:
        high = a.v > F32(hi)
        out.v[high], out.d[high] = F32(hi), 0
    return out


def _datan2(x, y):
    den = x.v * x.v + y.v * y.v + F32(1e-5)
    return Dual(_r32(np.arctan2, x.v, y.v), (x.d * y.v[:, None] - y.d * x.v[:, None]) / den[:, None])


def dual_restatement32(m, b, order):
    """the dual-number role of the lookup's backward in numpy float32: env_geometry<Dual<4>>, box_wrap and the bilinear taps with dual
    weights, every lookup walking its boxes in combo order.  order = "direct": k_env_lookup_bwd, three channels through SumAcc,
    contracted with d_out at the end; order = "binned": env_role_dirs, the taps contracted with d_out first (SumAccQ), the extra
    boxes' tangents summed apart from the main box's -> d_dirs [R, 3], dm [R] float32 (zero on pole rows)"""
    H, W, R = m.H, m.W, b.R
    n = np.arange(R)
    a, bb, c, mb = Dual(b.dirs[:, 0]), Dual(b.dirs[:, 1]), Dual(b.dirs[:, 2]), Dual(np.full(R, MIPBIAS, dtype=F32))
    a.d[:, 0], bb.d[:, 1], c.d[:, 2], mb.d[:, 3] = 1, 1, 1, 1
    eps, ln2 = F32(O.EPS), F32(math.log(2))
    cosv = _dsqrt(_dclip(1.0 - c * c, eps))
    den = _dclip(cosv * F32(19.739208802178716), eps)
    d = (_const(den, 1.0) / den) * F32(H * W)
    area = _dexp(_dlog(d / 2.0) + Dual(b.sa))
    hh = _dclip(_dsqrt(_dclip(area, eps)) * cosv, eps)
    ww = area / hh
    mw = _dclip(_dlog(ww) / ln2 + mb, 0.0, 7.0)
    mh = _dclip(_dlog(hh) / ln2 + mb, 0.0, 7.0)
    sw = _dpow2(mw) / F32(H) / 2.0
    sh = _dpow2(mh) / F32(H)
    size = ((sw / 2.0) * F32(W)) * ((sh / 2.0) * F32(H))
    norm2d = _dsqrt(a * a + bb * bb)
    phi, theta = _datan2(bb, a), _datan2(c, norm2d)
    r = np.fmod(phi.v, F32(2 * math.pi))
    r = np.where((r != 0) & (r < 0), r + F32(2 * math.pi), r).astype(F32)
    cx = (Dual(r, phi.d) - F32(math.pi)) / F32(math.pi)
    cy = ((-theta) / F32(math.pi)) * 2.0
    x0, x1, y0, y1 = cx - sw / 2.0, cx + sw / 2.0, cy - sh / 2.0, cy + sh / 2.0
    cutoff = F32(1) - F32(2) / F32(H) * F32(3)
    live = ~((cy.v > cutoff) | (cy.v < -cutoff))
    go = b.d_out
    sat = m.sat

    def sample(idx, x, y):
        ix, iy = (x + 1.0) * F32((W - 1) * 0.5), (y + 1.0) * F32((H - 1) * 0.5)
        fx, fy = np.floor(ix.v), np.floor(iy.v)
        w, nn = ix - fx, iy - fy
        e, s = 1.0 - w, 1.0 - nn
        xi, yi = fx.astype(np.int64), fy.astype(np.int64)
        taps = []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            ok = (xi + dx < W) & (yi + dy < H)
            taps.append(np.where(ok[None], sat[:, np.minimum(yi + dy, H - 1), np.minimum(xi + dx, W - 1)], F32(0)))
        wts = (e * s, w * s, e * nn, w * nn)
        if order == "binned":
            q = [(go[idx, 0] * t[0] + go[idx, 1] * t[1]) + go[idx, 2] * t[2] for t in taps]
            return [wts[0] * q[0] + wts[1] * q[1] + wts[2] * q[2] + wts[3] * q[3]]
        return [wts[0] * taps[0][ch] + wts[1] * taps[1][ch] + wts[2] * taps[2][ch] + wts[3] * taps[3][ch] for ch in range(3)]

    n_out = 1 if order == "binned" else 3
    total = [Dual(np.zeros(R, dtype=F32)) for _ in range(n_out)]
    extra = [np.zeros((R, 4), dtype=F32) for _ in range(n_out)]

    def box(idx, q, combo):
        xl, xr, yb, yt = (_dclip(v, -1.0, 1.0) for v in q)
        cur = sample(idx, xr, yt)
        for k, (x, y) in enumerate(((xl, yb), (xl, yt), (xr, yb))):
            s = sample(idx, x, y)
            cur = [u + v if k == 0 else u - v for u, v in zip(cur, s)]
        for ch in range(n_out):
            add = cur[ch] / size[idx]
            if order == "binned" and combo:
                extra[ch][idx] = extra[ch][idx] + add.d
            else:
                t = total[ch][idx] + add
                total[ch].v[idx], total[ch].d[idx] = t.v, t.d

    def box_lr(idx, q, v):
        box(idx, q, 3 * v)
        on = q[1].v > 1
        if on.any():
            box(idx[on], (_const(q[0][on], -1.0), q[1][on] - 2.0, q[2][on], q[3][on]), 3 * v + 1)
        on = q[0].v < -1
        if on.any():
            box(idx[on], (q[0][on] + 2.0, _const(q[1][on], 1.0), q[2][on], q[3][on]), 3 * v + 2)

    idx = n[live]
    rect = (x0[idx], x1[idx], y0[idx], y1[idx])
    box_lr(idx, rect, 0)
    rot = np.where(rect[0].v > 0, F32(-1), F32(1))
    on = rect[3].v > 1
    if on.any():
        over = _dclip(rect[3][on] - 1.0, 0.0, 0.5)
        box_lr(idx[on], (rect[0][on] + rot[on], rect[1][on] + rot[on], 1.0 - over, _const(over, 1.0)), 1)
    on = rect[2].v < -1
    if on.any():
        over = _dclip((-1.0) - rect[2][on], 0.0, 0.5)
        box_lr(idx[on], (rect[0][on] + rot[on], rect[1][on] + rot[on], _const(over, -1.0), over - 1.0), 2)
    if order == "binned":
        g = F32(1000) * (total[0].d + extra[0])
    else:
        g = F32(1000) * ((go[:, 0:1] * total[0].d + go[:, 1:2] * total[1].d) + go[:, 2:3] * total[2].d)
    g = np.where(live[:, None], g, F32(0)).astype(F32)
    return {"d_dirs": g[:, :3], "dm": g[:, 3]}


def scaled(b, arrays):
    """values and d_dirs in table units, split by footprint class -> {"values <1": ..., "d_dirs >16": ...}"""
    s = b.g.size / 1000.0
    out = {}
    for k, name in enumerate(CLASSES):
        on = b.g.cls == k
        out[f"values {name}"] = (np.asarray(arrays["values"], dtype=F64) * s[:, None])[on]
        if "d_dirs" in arrays:
            out[f"d_dirs {name}"] = (np.asarray(arrays["d_dirs"], dtype=F64)[:, -3:] * (s * b.g.norm2d)[:, None])[on]
    return out


SCALED = tuple(f"{q} {c}" for q in ("values", "d_dirs") for c in CLASSES)
SUMS = ("d_sat", "d_pole")


def mip_margin(dm32, dm64, idx=slice(None)):
    """max(8 |sum e_r|, sum |e_r|, 2^-23 sum |term_r|) over the per-lookup errors of the restatement"""
    e = dm32.astype(F64)[idx] - dm64[idx]
    return max(8 * abs(e.sum()), np.abs(e).sum(), FLOOR * np.abs(dm64[idx]).sum())


@functools.lru_cache(maxsize=None)
def case(H, name):
    """(float64 reference, restatement, its errors, margins) of a batch, computed once.  Scaled metrics per class under their
    SCALED names, the sums under theirs, "d_mip" the total's margin"""
    m, b = table(H), batch(H, name)
    ref = lookup_reference64(m, b)
    own = lookup_restatement32(m, b)
    ref_s, own_s = scaled(b, ref), scaled(b, own)
    err = errors_over(own_s, ref_s, SCALED)
    err.update(errors_over(own, ref, SUMS))
    # d_pole is a sum of ~100 float atomics per entry in whatever order the lookups retire: the restatement's error is the largest
    # over the lookup order and 16 drawn ones, not the luck of one (six entries give the maximum nothing to average over)
    rng = np.random.default_rng([31, H])
    rows = np.where(b.g.pole, np.where(b.g.cy < 0, 0, 1), -1)
    for _ in range(16):
        p = rng.permutation(b.R)
        dp = np.zeros((2, 3), dtype=F32)
        np.add.at(dp, rows[p][rows[p] >= 0], b.d_out[p][rows[p] >= 0])
        err["d_pole"] = max(err["d_pole"], _big(dp.astype(F64) - ref["d_pole"]))
    mg = margins(err, dict(ref_s, **{k: ref[k] for k in SUMS}), SCALED + SUMS)
    mg["d_mip"] = mip_margin(own["dm"], ref["dm"])
    err["d_mip"] = abs(float(own["d_mip"]) - ref["dm"].sum())
    return ref, own, err, mg


def class_margins(H):
    """the margins of the values per footprint class of a map: those of its full batch"""
    return {k: v for k, v in case(H, "full")[3].items() if k in SCALED[:3]}


ORDERS = ("direct", "binned")                     # the two forms of the dual-number role: k_env_lookup_bwd, env_role_dirs
D_DIRS = SCALED[3:]


@functools.lru_cache(maxsize=None)
def dual_case(H, name, order):
    """(dual_restatement32 of a batch, its errors, margins) for d_dirs per class and for the d_mip total: what the kernels' d_dirs
    and d_mip are held to.  Their forward mode rounds every product of a tap's tangent weight with a table entry of magnitude
    |SAT| before the four taps cancel, where reverse mode in fp32 (lookup_restatement32) differences the taps first: the first
    restatement's d_dirs is up to 50 times closer to float64 than the kernels can be and does not model them"""
    b = batch(H, name)
    ref = case(H, name)[0]
    own = dual_restatement32(table(H), b, order)
    ref_s = scaled(b, ref)
    err = errors_over(scaled(b, dict(own, values=ref["values"])), ref_s, D_DIRS)
    mg = margins(err, ref_s, D_DIRS)
    mg["d_mip"] = mip_margin(own["dm"], ref["dm"])
    err["d_mip"] = abs(float(mip_total32(own["dm"])) - ref["dm"].sum())
    return own, err, mg


def dirs_margins(H, order):
    """the d_dirs margins per footprint class of a map under one form of the dual-number role: those of its full batch"""
    return {k: dual_case(H, "full", order)[2][k] for k in D_DIRS}


BUILD_METRICS = ("act rest", "act clip", "pole")
BWD_METRICS = ("d_bg rest", "d_bg clip")


def split_clip(m, a, key):
    """a [3, H, W] as two metrics: the 96 texels that the clip set puts at, above and below x == 20, and the rest -- exp(20) and the
    adjoints it scales are 1e7 times an ordinary texel's, and one margin over both would hide the ordinary ones"""
    flat = np.asarray(a).reshape(-1)
    at = np.concatenate([m.at20, m.above, m.below])
    on = np.zeros(flat.size, dtype=bool)
    on[at] = True
    return {key + " rest": flat[~on], key + " clip": flat[on]}


def build_metrics(m, out):
    return dict(split_clip(m, out["act"], "act"), pole=out["pole"])


@functools.lru_cache(maxsize=None)
def build_case(H, which):
    """(inputs, float64 reference, restatement's errors, margins) of the build: which = "plain" (bg, 0.3, 0.8) or "clip" (bg2, 4, 0.5);
    errors and margins over BUILD_METRICS"""
    m = table(H)
    bg, br, mul = (m.bg, BRIGHT, MUL) if which == "plain" else (m.bg2, BRIGHT2, MUL2)
    ref, own = build_reference64(bg, br, mul), build_restatement32(bg, br, mul)
    ref_m = build_metrics(m, ref)
    err = errors_over(build_metrics(m, own), ref_m, BUILD_METRICS)
    return SimpleNamespace(bg=bg, brightness=br, mul=mul, act=own["act"]), ref, err, margins(err, ref_m, BUILD_METRICS)


@functools.lru_cache(maxsize=None)
def build_bwd_case(H, which, table_of):
    """the build's backward on d_sat = "rand" (a random table and pole adjoint) or "lookups" (the restatement's table and pole adjoint
    of the full batch) -> (d_sat4 [H, W, 4], d_pole, reference d_bg, errors of the restatement, margins over BWD_METRICS)"""
    m = table(H)
    i, _, _, _ = build_case(H, which)
    if table_of == "rand":
        d_sat4, d_pole = m.d_sat_rand, m.d_pole_rand
    else:
        own = case(H, "full")[1]
        d_sat4 = np.zeros((m.H, m.W, 4), dtype=F32)
        d_sat4[..., :3] = np.moveaxis(own["d_sat"], 0, -1)
        d_pole = own["d_pole"]
    ref = build_bwd_reference64(d_sat4, i.bg, i.act, d_pole, i.brightness, i.mul)
    ref_m = split_clip(m, ref, "d_bg")
    err = errors_over(split_clip(m, build_bwd_restatement32(d_sat4, i.bg, i.act, d_pole, i.brightness, i.mul), "d_bg"), ref_m, BWD_METRICS)
    return d_sat4, d_pole, ref, err, margins(err, ref_m, BWD_METRICS)


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [h for h, _ in MAPS])
def test_inputs_reach_every_branch(H):
    """the reject cap, every gate clear, and >= 64 lookups per reachable combo and per side of every other gate"""
    i = lookups(H)
    g = i.g
    live = ~g.pole
    print(f"H {H}: {i.R} lookups kept, {i.dropped} of {N_DRAW} dropped ({100 * i.dropped / N_DRAW:.2f} %), {i.dropped_pole} of the pole draws")
    assert i.dropped <= 0.05 * N_DRAW and i.dropped_pole <= 0.05 * N_POLE
    assert g.gate[live].min() >= CLEAR and g.pole_gate.min() >= CLEAR
    assert min((g.pole & (g.cy > 0)).sum(), (g.pole & (g.cy < 0)).sum()) >= 64
    counts = {c: int((live & ((g.mask >> c) & 1 == 1)).sum()) for c in range(9)}
    print(f"H {H}: lookups per combo {counts}")
    for c in range(1, 9):
        if c in (5, 8) and H >= 32:
            assert counts[c] == 0
        else:
            assert counts[c] >= 64, (H, c, counts[c])
    if H >= 32:           # the left wrap of a rotated box needs x0 + rot < -1 with |rot| = 1 chosen against x0: sw / 2 > 1
        assert 2.0 ** 7 / H / 2 <= 2.0
    sides = {"over top clipped": live & (g.over_top > 0.5), "over top free": live & (g.over_top > 0) & (g.over_top < 0.5),
             "over bottom clipped": live & (g.over_bot > 0.5), "over bottom free": live & (g.over_bot > 0) & (g.over_bot < 0.5),
             "mw at 0": live & (g.mw_u < 0), "mw free": live & (g.mw_u > 0) & (g.mw_u < 7), "mw at 7": live & (g.mw_u > 7),
             "mh at 0": live & (g.mh_u < 0), "mh free": live & (g.mh_u > 0) & (g.mh_u < 7), "mh at 7": live & (g.mh_u > 7),
             "rot -1": live & g.wrap & (g.x0 > 0), "rot +1": live & g.wrap & (g.x0 < 0)}
    print(f"H {H}: " + ", ".join(f"{k} {int(v.sum())}" for k, v in sides.items()))
    assert all(v.sum() >= 64 for v in sides.values()), {k: int(v.sum()) for k, v in sides.items()}
    assert all((g.cls == k).sum() >= 64 for k in range(3))
    assert (np.abs(g.cx) >= 0.9).sum() >= N_DRAW // 5 and int((~i.d_out.any(axis=1)).sum()) == 100
    scale = np.abs(i.d_out_range).max(axis=1)
    assert scale[scale > 0].min() < 1e-5 < 0.1 < scale.max()


def test_batches_and_tiles_are_what_they_are_named_for():
    d = batch(16, "dense")
    assert d.R == 256 and (d.g.n_boxes - 1).sum() >= 1024 and (d.g.n_boxes >= 5).all() and not d.g.pole.any()
    a = batch(16, "axis")
    assert a.R == 21 and a.g.pole.sum() == 6 and np.array_equal(a.dirs[6], np.array([1, -1e-30, 0], dtype=F32))
    assert np.abs(a.g.cx[[0, 6]]).tolist() == [1.0, 1.0] and a.g.cx[1] == 0.0          # +x is the table seam, -x its middle
    for n in SHAPES:
        assert batch(32, n).R == n and np.array_equal(batch(32, n).dirs, lookups(32).dirs[:n])
    records = case(16, "full")[1]["records"]
    assert records > ENV_ITEM and 16 < TILE_H and 32 < TILE_W, records                 # one partial tile, several work items
    assert 48 % TILE_H and 96 % TILE_W and 96 % 64 and 64 < 96 < 128                   # partial tiles both ways, partial second W chunk
    assert 64 < 80 < 128 and 128 < 160 < 192                                           # (80, 160): partial second H and third W chunk
    for H in (16, 48):
        assert all(len(v) >= 64 for v in sub_batches(H).values())


def test_model_is_the_oracle():
    """lookup_model without a fault is oracle.env_lookup bit for bit, in float32 and in float64: values and the adjoints of the
    directions, the table and the mip bias"""
    for H in (16, 48):
        m, b = table(H), batch(H, "full")
        for dtype, tt in ((F32, torch.float32), (F64, torch.float64)):
            bg = _t(m.act, dtype).log()[None]
            sd = {"bg_module.bg_mat": bg, "bg_module.brightness": torch.tensor(0.0, dtype=tt), "bg_module.mul": torch.tensor(1.0, dtype=tt)}
            act = O.env_activation(sd)
            pole = torch.stack([act[0, :, 0, :].mean(-1), act[0, :, -1, :].mean(-1)])
            outs = []
            for fn in ("oracle", "model"):
                sat, d = _t(m.sat, dtype)[None].requires_grad_(True), _t(b.dirs, dtype).requires_grad_(True)
                mip = torch.full((b.R,), MIPBIAS, dtype=tt, requires_grad=True)
                if fn == "oracle":
                    vals = O.env_lookup(dict(sd, **{"bg_module.mipbias": mip}), d, _t(b.sa, dtype), sat=sat)
                else:
                    vals, _ = lookup_model(sat, pole, d, _t(b.sa, dtype), mip)
                outs.append((vals.detach(),) + torch.autograd.grad((vals * _t(b.d_out, dtype)).sum(), [d, sat, mip]))
            assert all(torch.equal(x, y) for x, y in zip(*outs)), (H, dtype)


def test_build_references_agree_with_the_oracle():
    """sat_from_act is the oracle's cumsum on the same activation bit for bit; the float64 reverse sums are the autograd gradient"""
    for H, _ in BUILD_MAPS:
        m = table(H)
        want = torch.cumsum(torch.cumsum(torch.from_numpy(m.act.copy())[None] / 1000, dim=2), dim=3)[0].numpy()
        assert np.array_equal(m.sat, want) and np.array_equal(m.sat4[..., :3], np.moveaxis(m.sat, 0, -1)) and not m.sat4[..., 3].any()
    H = 48
    m = table(H)
    for which in ("plain", "clip"):
        i, ref, err, mg = build_case(H, which)
        bg = _t(i.bg, F64)[None].requires_grad_(True)
        sd = {"bg_module.bg_mat": bg, "bg_module.brightness": torch.tensor(float(i.brightness), dtype=torch.float64),
              "bg_module.mul": torch.tensor(float(i.mul), dtype=torch.float64)}
        act = O.env_activation(sd)
        assert np.array_equal(act.detach().numpy()[0], ref["act"])
        sat = torch.cumsum(torch.cumsum(act / 1000, dim=2), dim=3)
        loss = (sat[0] * _t(_planar(m.d_sat_rand), F64)).sum() + (act[0, :, 0].mean(-1) * _t(m.d_pole_rand[0], F64)).sum() \
            + (act[0, :, -1].mean(-1) * _t(m.d_pole_rand[1], F64)).sum()
        (g,) = torch.autograd.grad(loss, bg)
        mine = build_bwd_reference64(m.d_sat_rand, i.bg, ref["act"], m.d_pole_rand, i.brightness, i.mul)
        assert np.allclose(mine, g.numpy()[0], rtol=1e-11, atol=1e-13 * _big(mine))
    x = (BRIGHT2 + MUL2 * m.bg2).reshape(-1)
    assert (x[m.at20] == 20).all() and (x[m.above] == np.nextafter(F32(20), F32(30))).all() and (x[m.below] == np.nextafter(F32(20), F32(0))).all()
    x64 = (F64(BRIGHT2) + F64(MUL2) * m.bg2.astype(F64)).reshape(-1)
    at = np.concatenate([m.at20, m.above, m.below])
    assert np.array_equal(x.astype(F64)[at], x64[at])                      # at the clip texels the product and the sum are exact
    assert np.abs(x64 - 20).min(initial=np.inf, where=~np.isin(np.arange(x.size), at)) > 10        # every other texel is far away
    d_bg = build_bwd_case(H, "clip", "rand")[2].reshape(-1)
    assert not d_bg[m.above].any() and d_bg[m.at20].all() and d_bg[m.below].all()


def test_mip_total_order():
    """1e8, 1, -1e8 in three lanes of a wave that the tree adds as (1e8 + -1e8) + 1 keep the 1; met in another order they lose it"""
    dm = np.zeros(300, dtype=F32)
    dm[[0, 32, 1]] = (1e8, -1e8, 1.0)          # d = 32: lane 0 += lane 32 first
    assert mip_total32(dm) == 1.0
    dm[:] = 0
    dm[[0, 1, 32]] = (1e8, -1e8, 1.0)          # lane 0 + lane 32 = 1e8 (the 1 is lost), lane 1 cancels it later
    assert mip_total32(dm) == 0.0
    dm[:] = 0
    dm[[255, 256, 299]] = (1.0, 2.0, 4.0)
    assert mip_total32(dm) == 7.0


@pytest.mark.parametrize("H", [h for h, _ in MAPS])
def test_restatement_table(H):
    """prints the restatement's error per metric (scaled metrics also in units of ulp(max|SAT|)) and holds it to its own margin"""
    m = table(H)
    ulp = FLOOR * _big(m.sat)
    for name in ("full", "range") + (("dense",) if H == 16 else ()):
        ref, own, err, mg = case(H, name)
        b = batch(H, name)
        e = np.abs(own["dm"].astype(F64) - ref["dm"]) * b.g.size / 1000
        print(f"H {H} {name}: " + "  ".join(f"{k} {err[k]:.3e} ({err[k] / ulp:.1f} ulp)" for k in SCALED))
        print(f"H {H} {name}: per-lookup d_mip (scaled) median {np.median(e) / ulp:.2f} p99 {np.quantile(e, 0.99) / ulp:.1f}"
              f" max {e.max() / ulp:.1f} ulp;  d_sat {err['d_sat']:.3e} (scale {_big(ref['d_sat']):.3e})  d_pole {err['d_pole']:.3e} (scale {_big(ref['d_pole']):.3e})"
              f"  d_mip total {err['d_mip']:.3e} of {ref['dm'].sum():.4e}, margin {mg['d_mip']:.3e};  {own['records']} corner records")
        assert all(err[k] <= mg[k] for k in mg), {k: (err[k], mg[k]) for k in mg if err[k] > mg[k]}
        for order in ORDERS:
            du, err_d, mg_d = dual_case(H, name, order)
            cells = [f"{k} {err_d[k]:.3e} ({err_d[k] / ulp:.0f} ulp, {err_d[k] / max(err[k], 1e-300):.1f} x autograd)" for k in D_DIRS]
            print(f"H {H} {name} dual numbers, {order}: " + "  ".join(cells) + f"  d_mip total {err_d['d_mip']:.3e}, margin {mg_d['d_mip']:.3e}")
            assert all(err_d[k] <= mg_d[k] for k in mg_d) and np.isfinite(du["d_dirs"]).all()
            assert not du["d_dirs"][b.g.pole].any() and not du["d_dirs"][~b.d_out.any(axis=1)].any() and not du["dm"][b.g.pole].any()
        assert np.isfinite(own["d_dirs"]).all() and not own["d_dirs"][b.g.pole].any() and not ref["d_dirs"][b.g.pole].any()
        assert not own["d_dirs"][~b.d_out.any(axis=1)].any()
    for which in ("plain", "clip"):
        _, ref, err, mg = build_case(H, which)
        bwd = {t: build_bwd_case(H, which, t) for t in ("rand", "lookups")}
        print(f"H {H} build {which}: " + "  ".join(f"{k} {err[k]:.3e} (margin {mg[k]:.3e})" for k in BUILD_METRICS) + "  "
              + "  ".join(f"{k}/{t} {v[3][k]:.3e} (margin {v[4][k]:.3e})" for t, v in bwd.items() for k in BWD_METRICS))


@pytest.mark.parametrize("H", [h for h, _ in MAPS])
def test_faults_miss_their_margins(H):
    """every fault, built into the restatement, leaves its metric outside the margin in at least one footprint class"""
    m, b = table(H), batch(H, "full")
    ref, own, err, mg = case(H, "full")
    ref_s = scaled(b, ref)
    held = dict(mg)           # d_dirs and d_mip are held to the dual-number restatements: the looser of their two margins
    for k in D_DIRS + ("d_mip",):
        held[k] = max(dual_case(H, "full", order)[2][k] for order in ORDERS)
    named = {"no_right": ("values",), "rot": ("values",), "over1": ("values",), "cutoff2": ("values",), "pole_swap": ("values", "d_pole"),
             "mip8": ("values", "d_mip"), "tangent": ("d_dirs",), "own_size": ("values",)}
    for fault in FAULTS:
        bad = lookup_restatement32(m, b, fault)
        e = errors_over(scaled(b, bad), ref_s, SCALED)
        e.update(errors_over(bad, ref, SUMS))
        e["d_mip"] = abs(bad["dm"].astype(F64).sum() - ref["dm"].sum())
        for metric in named[fault]:
            keys = [k for k in mg if k.split(" ")[0] == metric]
            ratio = max(e[k] / held[k] for k in keys)
            print(f"H {H} {fault}: {metric} at {ratio:.3g} x margin")
            assert ratio > 1, (H, fault, metric, ratio)
    for which in ("plain", "clip"):
        i, _, _, _ = build_case(H, which)
        d_sat4, d_pole, ref_b, _, mg_b = build_bwd_case(H, which, "rand")
        for fault in ("gate_ge", "pole_H"):
            bad = build_bwd_restatement32(d_sat4, i.bg, i.act, d_pole, i.brightness, i.mul, fault)
            off = np.abs(bad.astype(F64) - ref_b)
            if fault == "gate_ge" and which == "clip":         # (the plain set has no texel near the gate)
                at = off.reshape(-1)[m.at20]
                print(f"H {H} {which} {fault}: the texels at x == 20 at {at.min() / mg_b['d_bg clip']:.3g} x margin and more")
                assert (at > mg_b["d_bg clip"]).all() and not bad.reshape(-1)[m.at20].any()
            elif fault == "pole_H":
                e = errors_over(split_clip(m, bad, "d_bg"), split_clip(m, ref_b, "d_bg"), ("d_bg rest",))["d_bg rest"]
                rest = split_clip(m, np.where(np.isin(np.arange(H), (0, H - 1))[None, :, None], 0.0, off), "d_bg")["d_bg rest"]
                print(f"H {H} {which} {fault}: rows 0 / H - 1 at {e / mg_b['d_bg rest']:.3g} x margin")
                assert e > mg_b["d_bg rest"] and rest.max() <= mg_b["d_bg rest"]
