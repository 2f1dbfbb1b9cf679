"""Denoised frames without a GPU (nmf_amd/multisample.py, csrc/denoise.hip; include/nmf_hip.h "Denoised frames"):
denoise_np, the numpy restatement of the three kernels in their operation order that tests/test_hip_denoise.py compares bit for bit
(fp32 on an fp32 state; the same code on a float64 state is denoise_f64), against float64; the properties the definition has by
construction, asserted exactly; what the filter does to the grain of a synthetic frame; the refusals of the entry points, the command
line's argument errors, and render_frame's flow with denoise= through its accumulator= / render= seam."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from test_multisample_cpu import (PL_ACC, PL_DEPTH, PL_LIN, PL_M2, PL_MAP, PL_NORMAL, F, NumpyAccumulator, StubRender, U, _stub_rays,  # noqa: E402
                                  accum_resolve_np, accum_update_np, run_passes, srgb_np, state_np)

WS_PLANES, MAX_LEVELS = 19, 8                     # NMF_DENOISE_PLANES, NMF_DENOISE_MAX_LEVELS
DEFAULTS = dict(levels=3, k_c=4.0, k_n=0.5, k_z=2.0, eps_z=0.02, k_a=0.25)
# widths under which the taps of a RANDOM state (run_passes: unrelated colours, normals and depths from pixel to pixel) are accepted
# with weights all over (0, 1): the restatement is compared where the filter mixes, not only where it rejects
WIDE = dict(k_c=8.0, k_n=3.0, k_z=40.0, eps_z=6.0, k_a=1.5)
BINOMIAL = (0.0625, 0.25, 0.375, 0.25, 0.0625)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def variance_np(st):
    """V = max_c (M2_c / ((float)n (float)(n - 1))) for n >= 2, else 0, in the state's dtype (a NaN quotient is dropped, as fmaxf does)"""
    T = st["planes"].dtype.type
    n = st["count"]
    cc = n.astype(T) * (n - 1).astype(T)
    v = np.zeros(n.shape, dtype=T)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            v = np.fmax(v, st["planes"][PL_M2 + k - 1] / cc)
    return np.where(n >= 2, v, T(0)).astype(T)


def denoise_prepare_np(st, H, W):
    """nmf_denoise_prepare -> dict(fixed bool [P], gx, gy [P], set = [8, P]: L 0-2, A 3, C 4-6, Vg 7)"""
    T = st["planes"].dtype.type
    pl = st["planes"]
    V = variance_np(st).reshape(H, W)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    ym, yp, xm, xp = np.maximum(ys - 1, 0), np.minimum(ys + 1, H - 1), np.maximum(xs - 1, 0), np.minimum(xs + 1, W - 1)
    rows = [(V[yy, xm] + T(2) * V[yy, xs]) + V[yy, xp] for yy in (ym, ys, yp)]
    vg = ((rows[0] + T(2) * rows[1]) + rows[2]) * T(0.0625)
    Z = pl[PL_DEPTH - 1].reshape(H, W)
    gx = (Z[ys, xp] - Z[ys, xm]) * T(0.5)
    gy = (Z[yp, xs] - Z[ym, xs]) * T(0.5)
    s = np.concatenate([pl[PL_LIN - 1:PL_LIN + 2], pl[PL_ACC - 1:PL_ACC], pl[PL_MAP - 1:PL_MAP + 2], vg.reshape(1, -1)]).astype(T)
    assert s.shape == (8, H * W) and vg.dtype == T and gx.dtype == T
    return dict(fixed=(V == 0).reshape(-1), gx=gx.reshape(-1), gy=gy.reshape(-1), set=s)


def denoise_level_np(st, ws, H, W, step, k_c, k_n, k_z, eps_z, k_a, src=None):
    """nmf_denoise_level: one level of step `step` over ws["set"] (or `src`) -> the new [8, P] set; the taps in the kernel's order, one
    rounding per operation in the state's dtype"""
    T = st["planes"].dtype.type
    pl = st["planes"]
    s_in = ws["set"] if src is None else src
    g = lambda a: a.reshape(-1, H, W)      # noqa: E731
    Lq, Aq, Cq, Vq = g(s_in[0:3]), g(s_in[3:4])[0], g(s_in[4:7]), g(s_in[7:8])[0]
    Nq, Zq = g(pl[PL_NORMAL - 1:PL_NORMAL + 2]), g(pl[PL_DEPTH - 1:PL_DEPTH])[0]
    gx, gy = ws["gx"].reshape(H, W), ws["gy"].reshape(H, W)
    kc2, kn2, ka2 = T(F(k_c) * F(k_c)), T(F(k_n) * F(k_n)), T(F(k_a) * F(k_a))      # fp32 products taken on the host
    kz, ez, tiny = T(F(k_z)), T(F(eps_z)), T(F(1e-10))
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    sw, sv, sa = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W), T)
    sl, sc = np.zeros((3, H, W), T), np.zeros((3, H, W), T)
    others = np.zeros((H, W), dtype=np.int32)
    with np.errstate(all="ignore"):
        for i in range(-2, 3):
            for j in range(-2, 3):
                qy, qx = ys + step * i, xs + step * j
                on = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                w = np.full((H, W), T(BINOMIAL[i + 2]) * T(BINOMIAL[j + 2]), dtype=T)
                if i or j:
                    c = [Cq[k] - Cq[k][qy, qx] for k in range(3)]
                    d = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) / (kc2 * (Vq + Vq[qy, qx]) + tiny)
                    n = [Nq[k] - Nq[k][qy, qx] for k in range(3)]
                    d = d + ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) / kn2
                    dz = Zq - Zq[qy, qx]
                    e = kz * np.abs(gx * T(step * j) + gy * T(step * i)) + ez
                    d = d + (dz * dz) / (e * e)
                    da = Aq - Aq[qy, qx]
                    d = d + (da * da) / ka2
                    t = np.fmax(T(0), T(1) - d)                                          # fmaxf: 0 for a NaN
                    on = on & (t > 0)
                    w = (w * t) * t
                    others += on
                sw = np.where(on, sw + w, sw)
                for k in range(3):
                    sl[k] = np.where(on, sl[k] + w * Lq[k][qy, qx], sl[k])
                    sc[k] = np.where(on, sc[k] + w * Cq[k][qy, qx], sc[k])
                sa = np.where(on, sa + w * Aq[qy, qx], sa)
                sv = np.where(on, sv + (w * w) * Vq[qy, qx], sv)
        out = np.concatenate([sl / sw, (sa / sw)[None], sc / sw, (sv / (sw * sw))[None]]).reshape(8, H * W).astype(T)
    keep = ws["fixed"] | (others.reshape(-1) == 0)                                       # pass through bit for bit
    out[:, keep] = s_in[:, keep]
    assert out.dtype == T and sw.dtype == T
    return out


def denoise_finish_np(s, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False):
    """nmf_denoise_finish -> dict(rgb_map [P, 3], rgb_lin [P, 3], acc [P], se [P])"""
    T = s.dtype.type
    t = T(1) - s[3]
    rgb = np.stack([(srgb_np(s[k], noclip, T) if tonemap else s[k]) + t * T(F(bg[k])) for k in range(3)], -1)
    assert rgb.dtype == T
    with np.errstate(invalid="ignore"):
        return dict(rgb_map=rgb, rgb_lin=np.ascontiguousarray(s[0:3].T), acc=s[3].copy(), se=np.sqrt(s[7]))


def denoise_np(st, H, W, levels=3, k_c=4.0, k_n=0.5, k_z=2.0, eps_z=0.02, k_a=0.25, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False,
               trace=None):
    """nmf_denoise on a numpy state in the state's dtype; trace: a list that receives the [8, P] set before level 0 and after every level"""
    ws = denoise_prepare_np(st, H, W)
    s = ws["set"]
    if trace is not None:
        trace.append(s.copy())
    for l in range(levels):
        s = denoise_level_np(st, ws, H, W, 1 << l, k_c, k_n, k_z, eps_z, k_a, src=s)
        if trace is not None:
            trace.append(s.copy())
    out = denoise_finish_np(s, bg, tonemap, noclip)
    out["fixed"] = ws["fixed"]
    return out


def denoise_f64(st, H, W, **kw):
    """the same definition in float64 on the fp32 state's values"""
    return denoise_np(dict(count=st["count"].copy(), planes=st["planes"].astype(np.float64)), H, W, **kw)


def mixed_state(H, W, seed):
    """a state of run_passes (three passes with sub-lists, one of them with NaNs planted: counts 1 to 3) in which every seventh pixel is
    emptied again (count 0, zero planes): counts 0, 1 (no variance: fixed) and 2, 3"""
    P = H * W
    st = run_passes(P, 3, seed)
    st["count"][::7] = 0
    st["planes"][:, ::7] = 0
    return st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F else np.uint64)


# ---- fp32 against float64 ----------------------------------------------------------------------------------------------------------
# measured |fp32 - float64| per output, the largest over both frames, both parameter sets and levels 1, 3, 5, in units of u = 2^-24
# (test_restatement_against_float64 prints them); the asserted bound is 4 x the measurement, the project's margin for a comparison
# that is not bitwise
MEASURED_U = dict(rgb_map=4.78, rgb_lin=5.66, acc=3.33, se=1.45)


def test_restatement_against_float64():
    """The inputs are NOT kept away from d = 1: t = max(0, 1 - d) enters the weight squared, so a tap that fp32 and float64 put on
    different sides of the support's edge weighs (rounding error)^2 on one side and nothing on the other; the measurement shows no
    effect of it."""
    worst = dict.fromkeys(MEASURED_U, 0.0)
    for H, W in ((5, 7), (37, 53)):
        st = mixed_state(H, W, seed=H)
        for prm in (dict(DEFAULTS), dict(DEFAULTS, **WIDE)):
            for levels in (1, 3, 5):
                prm["levels"] = levels
                a = denoise_np(st, H, W, bg=(1.0, 0.5, 0.25), **prm)
                b = denoise_f64(st, H, W, bg=(1.0, 0.5, 0.25), **prm)
                assert np.array_equal(a["fixed"], b["fixed"]) and 0 < a["fixed"].sum() < H * W
                for k in worst:
                    assert a[k].dtype == F and b[k].dtype == np.float64
                    worst[k] = max(worst[k], float(np.abs(a[k].astype(np.float64) - b[k]).max()))
    for k, v in worst.items():
        print(f"{k}: |fp32 - float64| = {v / U:.2f} u (measured {MEASURED_U[k]} u, bound 4 x)")
    for k, v in worst.items():
        assert v <= 4 * MEASURED_U[k] * U, k


def test_wide_parameters_mix_the_random_state():
    """what WIDE is for: under it most free pixels of the random state take in other taps (under the defaults nearly none does, the
    neighbours of a random state being unrelated), so both the accepting and the rejecting side of every test are restated"""
    H, W = 37, 53
    st = mixed_state(H, W, seed=H)
    share = {}
    for name, prm in (("defaults", dict(DEFAULTS, levels=1)), ("wide", dict(DEFAULTS, **WIDE, levels=1))):
        tr = []
        out = denoise_np(st, H, W, trace=tr, **prm)
        free = ~out["fixed"]
        share[name] = float((_bits(tr[1][0:3]) != _bits(tr[0][0:3])).any(0)[free].mean())
    print("share of the free pixels a level changes:", share)
    assert share["wide"] > 0.9 and share["defaults"] < share["wide"]


# ---- properties that hold by construction ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prm", [DEFAULTS, dict(DEFAULTS, **WIDE)], ids=["defaults", "wide"])
def test_fixed_pixels_keep_their_bits_at_every_level(prm):
    H, W = 37, 53
    st = mixed_state(H, W, seed=3)
    tr = []
    out = denoise_np(st, H, W, trace=tr, **prm)
    fixed = out["fixed"]
    assert np.array_equal(fixed, variance_np(st) == 0) and fixed[::7].all() and (st["count"][fixed] < 2).all() and 0 < fixed.sum() < H * W
    assert len(tr) == prm["levels"] + 1
    for s in tr[1:]:
        assert np.array_equal(_bits(s[:, fixed]), _bits(tr[0][:, fixed]))
    raw = accum_resolve_np(st)
    assert np.array_equal(_bits(out["rgb_map"][fixed]), _bits(raw["rgb_map"][fixed]))
    assert np.array_equal(_bits(out["acc"][fixed]), _bits(raw["acc"][fixed]))
    if prm["k_n"] > 1:
        assert (_bits(out["rgb_map"][~fixed]) != _bits(raw["rgb_map"][~fixed])).any(1).mean() > 0.9


@pytest.mark.parametrize("tonemap", [True, False])
@pytest.mark.parametrize("noclip", [True, False])
def test_zero_levels_are_the_resolved_frame(tonemap, noclip):
    H, W = 37, 53
    st = mixed_state(H, W, seed=4)
    st["planes"][0, 1:7] = [0.0, 0.0031308, np.nextafter(F(0.0031308), F(1)), 1.0, 1.5, -0.25]      # the knee, the clip, a negative radiance
    bg = (1.0, 0.5, 0.25)
    out = denoise_np(st, H, W, levels=0, bg=bg, tonemap=tonemap, noclip=noclip)
    raw = accum_resolve_np(st, bg, tonemap, noclip)
    assert np.array_equal(_bits(out["rgb_map"]), _bits(raw["rgb_map"])) and np.array_equal(_bits(out["acc"]), _bits(raw["acc"]))
    assert np.array_equal(_bits(out["rgb_lin"]), _bits(np.ascontiguousarray(st["planes"][0:3].T)))
    # se of zero levels: the root of the blurred variance; on a frame of one pixel the blur is the identity (16 V / 16)
    one = dict(count=np.array([3], dtype=np.int32), planes=st["planes"][:, 20:21].copy())
    one["planes"][PL_M2 - 1:PL_M2 + 2, 0] = [0.3, 0.1, 0.2]
    assert _bits(denoise_np(one, 1, 1, levels=0)["se"])[0] == _bits(np.sqrt(variance_np(one)))[0] and variance_np(one)[0] > 0


def test_a_pixel_without_other_taps_keeps_its_input():
    """1 x 1: every other tap is off the frame at every step; 5 x 7 at step 16 likewise ((36/256 x) / (36/256) need not return x, so a
    pixel none of whose other taps contributed is copied, which the header states)"""
    st = mixed_state(5, 7, seed=6)
    one = dict(count=np.array([3], dtype=np.int32), planes=st["planes"][:, 5:6].copy())
    one["planes"][PL_M2 - 1:PL_M2 + 2, 0] = [0.3, 0.1, 0.2]
    assert variance_np(one)[0] > 0
    tr = []
    out = denoise_np(one, 1, 1, trace=tr, **DEFAULTS)
    assert not out["fixed"][0] and all(np.array_equal(_bits(s), _bits(tr[0])) for s in tr)
    assert np.array_equal(_bits(out["rgb_map"]), _bits(accum_resolve_np(one)["rgb_map"]))
    ws = denoise_prepare_np(st, 5, 7)
    prm = {k: v for k, v in dict(DEFAULTS, **WIDE).items() if k != "levels"}
    assert not ws["fixed"].all()
    assert np.array_equal(_bits(denoise_level_np(st, ws, 5, 7, 16, **prm)), _bits(ws["set"]))
    assert not np.array_equal(_bits(denoise_level_np(st, ws, 5, 7, 1, **prm)), _bits(ws["set"]))      # (step 1 does mix)


def two_region_state(H, W, edge, rng, *, colours, normals, depths, accs, strip=0, sigma=0.05, samples=4, spread=0.0, acc_map=None):
    """A frame split at column `edge`: per side a linear colour (rgb_map = rgb_lin: the tests resolve without the tonemap), a normal,
    a depth and a coverage; `samples` passes with Gaussian noise of `sigma` on the colour.  spread: the half-width of a per-pixel
    uniform offset of the colour (a texture, so that a region has a min and a max); acc_map [P]: a coverage per pixel instead of
    accs.  The top `strip` rows are background: acc 0,
    radiance 0, displayed colour 1, no noise.  -> (state, truth [P, 3], left [P] bool, background [P] bool)"""
    P = H * W
    xs = np.tile(np.arange(W), H)
    bgm = np.repeat(np.arange(H), W) < strip
    left = xs < edge
    side = np.where(left, 0, 1)
    truth = np.asarray(colours, dtype=np.float64)[side] + rng.uniform(-spread, spread, size=(P, 3))
    truth[bgm] = 0.0
    st = state_np(P)
    cover = np.asarray(accs)[side] if acc_map is None else acc_map
    for _ in range(samples):
        lin = (truth + rng.normal(0.0, sigma, size=(P, 3)) * ~bgm[:, None]).astype(F)
        mp = np.where(bgm[:, None], F(1), lin)
        accum_update_np(st, lin, np.where(bgm, 0, cover).astype(F), mp,
                        np.where(bgm, 0, np.asarray(depths)[side]).astype(F), np.where(bgm[:, None], 0, np.asarray(normals)[side]).astype(F))
    return st, truth, left, bgm


@pytest.mark.parametrize("case", ["normal", "normal_at_k_n", "coverage_at_k_a"])
def test_nothing_leaks_across_a_normal_or_coverage_edge(case):
    """k_c = 1000 opens the colour test, so only the guides stand between two regions whose colours are 0.5 apart.  Every output
    channel of a region lies inside [min, max] of that region's own inputs (a weighted mean of them; the weights vary over (0, 1] and
    the inputs by +-0.1 of texture, so no mean comes within rounding of an end).  The stronger form: adding 100 to the radiance of the
    right region (the guide colour C, which the weights read, stays) leaves every bit of the left region's radiance: its taps across
    the edge weigh exactly nothing.  |dN|^2 = k_n^2 and dA = k_a give d = 1 from that term alone: the support's edge is outside.
    The coverage case has a texture too (left 0.96875 to 1, right 0.66875 to 0.71875, the two ends side by side at the edge, exactly
    k_a apart): a mean of EQUAL values other than 1 is not exact in fp32 (sum(w a) / sum(w) wobbles by an ulp), so a constant 0.75
    would leave its own [min, max] by rounding, and the filtered coverage of a textured region stays inside the region's range."""
    H, W, edge = 24, 40, 17
    rng_a = np.random.default_rng(13)
    prm = dict(DEFAULTS, k_c=1000.0)
    kw = dict(colours=[(0.25, 0.3, 0.35), (0.75, 0.7, 0.65)], normals=[(0, 0, 1), (0, 0, 1)], depths=[3.0, 3.0], accs=[1.0, 1.0])
    flat = dict(kw)
    if case == "normal":
        kw["normals"] = [(0, 0, 1), (0, 1, 0)]
    elif case == "normal_at_k_n":
        kw["normals"] = [(0, 0, 1), (0, 0, 0.5)]                                         # |dN|^2 = 0.25 = k_n^2
    else:
        xs = np.tile(np.arange(W), H)
        cover = np.where(xs < edge, 1.0 - rng_a.uniform(0, 0.03125, size=H * W), 0.71875 - rng_a.uniform(0, 0.05, size=H * W))
        cover[5 * W + edge - 1], cover[5 * W + edge] = 0.96875, 0.71875                  # dA = 0.25 = k_a, both exact in fp32
        kw["acc_map"] = cover
    st, truth, left, _ = two_region_state(H, W, edge, np.random.default_rng(12), spread=0.1, **kw)
    tr = []
    out = denoise_np(st, H, W, tonemap=False, bg=(0.0, 0.0, 0.0), trace=tr, **prm)
    assert not out["fixed"].any()
    moved = 0
    for region in (left, ~left):
        for ch in range(7):                                                              # L, A, C
            lo, hi = tr[0][ch, region].min(), tr[0][ch, region].max()
            for s in tr[1:]:
                assert lo <= s[ch, region].min() and s[ch, region].max() <= hi, (case, ch)
        moved += int((_bits(tr[-1][0:3, region]) != _bits(tr[0][0:3, region])).any(0).sum())
    assert moved > 0.9 * H * W                                                           # the filter did work inside the regions
    lifted = dict(count=st["count"], planes=st["planes"].copy())
    lifted["planes"][PL_LIN - 1:PL_LIN + 2][:, ~left] += F(100)
    out2 = denoise_np(lifted, H, W, tonemap=False, bg=(0.0, 0.0, 0.0), **prm)
    assert np.array_equal(_bits(out2["rgb_lin"][left]), _bits(out["rgb_lin"][left]))
    assert (out2["rgb_lin"][~left] > 99).all()
    # the control: without the edge in normal or coverage the same frame does leak (this is what the guides are for)
    st, truth, left, _ = two_region_state(H, W, edge, np.random.default_rng(12), spread=0.1, **flat)
    tr = []
    denoise_np(st, H, W, tonemap=False, bg=(0.0, 0.0, 0.0), trace=tr, **prm)
    assert tr[-1][0, left].max() > tr[0][0, left].max() and tr[-1][0, ~left].min() < tr[0][0, ~left].min()


# ---- what it does to the grain -----------------------------------------------------------------------------------------------------
def _rmse(a, b, sel):
    return float(np.sqrt(((a[sel].astype(np.float64) - b[sel]) ** 2).mean()))


def test_noise_reduction_on_a_two_region_frame():
    """48 x 64, a vertical edge in colour, normal and depth at column 30, a background strip of 6 rows (acc 0, no variance), Gaussian
    noise of sigma 0.05 per sample, 4 samples; the error against the noiseless truth over the regions' interior (3 pixels off the edge,
    the strip and the frame).  With all t = 1 one level alone leaves sqrt(sum h^2) = 70 / 256 = 0.27 of the standard deviation; the
    bounds 0.5 (one level) and 0.25 (five) leave room for the taps the colour test rejects."""
    H, W, edge, strip = 48, 64, 30, 6
    st, truth, left, bgm = two_region_state(H, W, edge, np.random.default_rng(1), colours=[(0.6, 0.3, 0.2), (0.2, 0.5, 0.7)],
                                            normals=[(0, 0, 1), (1, 0, 0)], depths=[3.0, 4.0], accs=[1.0, 1.0], strip=strip)
    ys, xs = np.repeat(np.arange(H), W), np.tile(np.arange(W), H)
    inner = (ys >= strip + 3) & (ys < H - 3) & (xs >= 3) & (xs < W - 3) & (np.abs(xs - edge + 0.5) > 3)
    raw = accum_resolve_np(st, (1.0, 1.0, 1.0), False, True)
    e_raw = _rmse(raw["rgb_map"], truth, inner)
    assert abs(e_raw - 0.05 / 2) < 0.002                                                 # sigma / sqrt(4)
    ratio = {}
    for levels in (1, 2, 5):
        out = denoise_np(st, H, W, tonemap=False, noclip=True, **dict(DEFAULTS, levels=levels))
        ratio[levels] = _rmse(out["rgb_map"], truth, inner) / e_raw
        # the background keeps its bits: the displayed colour, the radiance and the coverage
        assert out["fixed"][bgm].all() and not out["fixed"][~bgm].any()
        for k in ("rgb_map", "acc"):
            assert np.array_equal(_bits(out[k][bgm]), _bits(raw[k][bgm])), k
        assert (out["rgb_map"][bgm] == 1).all() and (out["acc"][bgm] == 0).all()
    guide = float(out["se"][inner].mean())
    print(f"RMSE denoised / raw: {ratio}; raw {e_raw:.5f}; the propagated guide sqrt(Vg) reads {guide:.5f} against an error of "
          f"{ratio[5] * e_raw:.5f} after 5 levels")
    assert ratio[1] < 0.5 and ratio[5] < 0.25 and ratio[5] < ratio[2] < ratio[1]
    assert guide < ratio[5] * e_raw                                                      # a guide, not an estimate: it reads low


def test_a_colour_only_edge_is_not_blurred():
    """normal, depth and coverage equal on both sides: only the colour test can stop the filter.  The error in the 6-pixel band around
    the edge after five levels is not above the raw error there."""
    H, W, edge = 48, 64, 30
    st, truth, left, _ = two_region_state(H, W, edge, np.random.default_rng(2), colours=[(0.6, 0.3, 0.2), (0.2, 0.5, 0.7)],
                                          normals=[(0, 0, 1), (0, 0, 1)], depths=[3.0, 3.0], accs=[1.0, 1.0])
    xs = np.tile(np.arange(W), H)
    band = (xs >= edge - 3) & (xs < edge + 3)
    raw = accum_resolve_np(st, (1.0, 1.0, 1.0), False, True)
    out = denoise_np(st, H, W, tonemap=False, noclip=True, **dict(DEFAULTS, levels=5))
    e_raw, e_den = _rmse(raw["rgb_map"], truth, band), _rmse(out["rgb_map"], truth, band)
    print(f"band around a colour-only edge: raw {e_raw:.5f}, denoised {e_den:.5f}")
    assert e_den <= e_raw


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
NAMES = ("nmf_denoise_workspace_bytes", "nmf_denoise_prepare", "nmf_denoise_level", "nmf_denoise_finish", "nmf_denoise")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    f, i, p = C.c_float, C.c_int32, C.c_void_p
    lib.nmf_denoise_workspace_bytes.argtypes, lib.nmf_denoise_workspace_bytes.restype = [i, i], C.c_int64
    lib.nmf_denoise_prepare.argtypes = [p, p, i, i, p]
    lib.nmf_denoise_level.argtypes = [p, p, i, i, i, i, f, f, f, f, f, p]
    lib.nmf_denoise_finish.argtypes = [p, i, i, i, f, f, f, i, i, p, p, p, p, p]
    lib.nmf_denoise.argtypes = [p, p, i, i, i, f, f, f, f, f, f, f, f, i, i, p, p, p, p, p]
    return lib, hip


def test_symbols_are_declared_exported_and_bound():
    lib, hip = _lib()
    hdr = open(os.path.join(ROOT, "include", "nmf_hip.h")).read()
    for name in NAMES:
        assert f" {name}(" in hdr and hasattr(lib, name) and name in hip.EXPORTS
    assert "Denoised frames" in hdr and "#define NMF_DENOISE_PLANES %d" % WS_PLANES in hdr
    assert "#define NMF_DENOISE_MAX_LEVELS %d" % MAX_LEVELS in hdr and (hip.DENOISE_PLANES, hip.DENOISE_MAX_LEVELS) == (WS_PLANES, MAX_LEVELS)
    assert "#define NMF_ABI_VERSION %d" % hip.version() in hdr
    build = open(os.path.join(ROOT, "nmf_amd", "csrc", "build.sh")).read()
    line = [ln for ln in build.splitlines() if "-ffp-contract=off" in ln and "accum.hip" in ln][0]
    assert "denoise.hip" in line and "camera.hip" in line
    src = open(os.path.join(ROOT, "nmf_amd", "csrc", "denoise.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.replace("no atomics", "") and "__shared__" not in src
    for word in ("expf", "powf", "exp(", "__expf"):                                      # the weights use + - * / max fabs only
        assert word not in src
    for H, W in ((1, 1), (5, 7), (37, 53), (400, 400), (1, 70001)):
        assert lib.nmf_denoise_workspace_bytes(H, W) == 4 * WS_PLANES * H * W == hip.denoise_workspace_bytes(H, W)
    for H, W in ((0, 5), (5, -1), (46341, 46341)):
        assert lib.nmf_denoise_workspace_bytes(H, W) == 0
        with pytest.raises(hip.NmfHipError):
            hip.denoise_workspace_bytes(H, W)


def test_refusals_name_the_function():
    """every refusal without device memory: the argument checks come before the pointers', and a misaligned pointer is never read"""
    lib, _ = _lib()
    inf, nan = float("inf"), float("nan")
    odd = 0x1002                                                                         # not 4-byte aligned (and never dereferenced)
    K = dict(k_c=4.0, k_n=0.5, k_z=2.0, eps_z=0.02, k_a=0.25)

    def check(fn, name, cases):
        for kw, code, word in cases:
            assert fn(**kw) == code, (name, kw)
            msg = lib.nmf_last_error_string()
            assert name in msg and word in msg, (kw, msg)

    frame = [(dict(H=0), -1, b"below 1"), (dict(W=-2), -1, b"below 1"), (dict(H=46341, W=46341), -2, b"2^31 - 1")]
    widths = [(dict(**{k: v}), -1, b"finite and positive") for k in K for v in (0.0, -1.0, inf, nan)]

    def prepare(H=5, W=7, state=None, ws=None):
        return lib.nmf_denoise_prepare(state, ws, H, W, None)
    check(prepare, b"nmf_denoise_prepare:", frame + [(dict(), -1, b"null pointer"), (dict(state=odd + 2), -1, b"null pointer"),
                                                     (dict(state=odd, ws=odd + 2), -1, b"aligned"), (dict(state=odd + 2, ws=odd), -1, b"aligned")])

    def level(H=5, W=7, step=1, src=0, state=None, ws=None, **kw):
        k = dict(K, **kw)
        return lib.nmf_denoise_level(state, ws, H, W, step, src, k["k_c"], k["k_n"], k["k_z"], k["eps_z"], k["k_a"], None)
    check(level, b"nmf_denoise_level:", frame + widths + [(dict(), -1, b"null pointer"), (dict(step=0), -1, b"step"), (dict(step=257), -1, b"step"),
                                                         (dict(src=2), -1, b"src"), (dict(src=-1), -1, b"src"),
                                                         (dict(state=odd, ws=odd + 2), -1, b"aligned")])
    assert level(step=256) == -1 and b"null pointer" in lib.nmf_last_error_string()     # the largest step is allowed

    def finish(H=5, W=7, src=0, bg=(1.0, 1.0, 1.0), ws=None, out=None):
        return lib.nmf_denoise_finish(ws, H, W, src, *bg, 1, 0, out, None, None, None, None)
    check(finish, b"nmf_denoise_finish:", frame + [(dict(), -1, b"null workspace"), (dict(src=3), -1, b"src"), (dict(bg=(1.0, nan, 1.0)), -1, b"bg"),
                                                   (dict(bg=(inf, 0.0, 0.0)), -1, b"bg"), (dict(ws=odd), -1, b"aligned"),
                                                   (dict(ws=odd + 2), -1, b"no output")])

    def whole(H=5, W=7, levels=5, bg=(1.0, 1.0, 1.0), state=None, ws=None, out=None, **kw):
        k = dict(K, **kw)
        return lib.nmf_denoise(state, ws, H, W, levels, k["k_c"], k["k_n"], k["k_z"], k["eps_z"], k["k_a"], *bg, 1, 0, out, None, None, None, None)
    check(whole, b"nmf_denoise:", frame + widths + [(dict(), -1, b"null pointer"), (dict(levels=-1), -1, b"levels"), (dict(levels=9), -1, b"levels"),
                                                   (dict(bg=(0.0, 0.0, nan)), -1, b"bg"), (dict(state=odd, ws=odd + 2), -1, b"aligned"),
                                                   (dict(state=odd + 2, ws=odd + 6), -1, b"no output")])
    assert whole(levels=0) == -1 and whole(levels=8) == -1 and b"null pointer" in lib.nmf_last_error_string()      # both ends are allowed


def test_wrappers_and_parameters_refuse():
    _, hip = _lib()
    from nmf_amd.multisample import DenoiseParams
    state = torch.zeros(hip.accum_state_bytes(4, 4) // 4, dtype=torch.int32)
    ws = torch.zeros(hip.denoise_workspace_bytes(4, 4) // 4)
    with pytest.raises(hip.NmfHipError):
        hip.denoise_prepare(state, ws, 4, 4)
    with pytest.raises(hip.NmfHipError):
        hip.denoise_level(state, ws, 4, 4, 1, 0, 4.0, 0.5, 2.0, 0.02, 0.25)
    with pytest.raises(hip.NmfHipError):
        hip.denoise_finish(ws, 4, 4, 0)
    with pytest.raises(hip.NmfHipError):
        hip.denoise(state, 4, 4, 5, 4.0, 0.5, 2.0, 0.02, 0.25, workspace=ws)
    p = DenoiseParams()
    assert p.record() == DEFAULTS and DenoiseParams(levels=0).levels == 0 and DenoiseParams(levels=8, k_c=1).k_c == 1
    for kw in (dict(levels=-1), dict(levels=9), dict(levels=2.5), dict(k_c=0.0), dict(k_n=-1.0), dict(k_z=float("inf")), dict(eps_z=float("nan")),
               dict(k_a=0)):
        with pytest.raises(ValueError):
            DenoiseParams(**kw)


def test_render_argument_errors(capsys):
    from nmf_amd import render as R
    base = ["--ckpt", "none.th"]
    for extra, word in ((["--denoise"], "--denoise needs --spp"), (["--denoise", "3", "--spp", "1"], "--denoise needs --spp"),
                        (["--denoise-strength", "2", "--spp", "4"], "--denoise-strength needs --denoise"),
                        (["--spp", "4", "--denoise", "9"], "--denoise takes"), (["--spp", "4", "--denoise", "-1"], "--denoise takes"),
                        (["--spp", "4", "--denoise", "--denoise-strength", "0"], "--denoise-strength takes"),
                        (["--spp", "4", "--denoise", "--denoise-strength", "nan"], "--denoise-strength takes")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra


# ---- render_frame's flow -----------------------------------------------------------------------------------------------------------
class DenoisingAccumulator(NumpyAccumulator):
    """NumpyAccumulator with FrameAccumulator.denoise over denoise_np; it records its calls"""

    def __init__(self, H, W):
        super().__init__(H, W)
        self.denoised = []

    def denoise(self, params, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False, keys=("rgb_map",), frame_hw=None):
        H, W = (self.H, self.W) if frame_hw is None else frame_hw
        self.denoised.append((params, (H, W), tuple(keys)))
        r = denoise_np(self.st, H, W, bg=bg, tonemap=tonemap, noclip=noclip, **params.record())
        return {k: torch.from_numpy(r[dict(acc_map="acc").get(k, k)]) for k in keys}


def test_render_frame_flow_with_a_stub():
    from nmf_amd.multisample import DenoiseParams, render_frame
    Hf, Wf = 12, 25
    P = Hf * Wf
    rays = _stub_rays(P)
    keys = ("rgb_map", "rgb_raw", "rgb_lin", "depth")
    # off by default: the accumulator's denoise is never asked, rgb_raw is no key, depth and normal are not rendered for the filter
    acc, stub = DenoisingAccumulator(1, P), StubRender()
    plain, _ = render_frame(None, rays, 50.0, spp=4, jitter=False, accumulator=acc, render=stub)
    assert acc.denoised == [] and set(plain) == {"rgb_map", "se", "count"} and set(stub.calls[0][1]) == {"rgb_map", "acc_map", "rgb_lin"}
    with pytest.raises(ValueError):
        render_frame(None, rays, 50.0, spp=4, jitter=False, keys=("rgb_map", "rgb_raw"), accumulator=DenoisingAccumulator(1, P), render=StubRender())
    # on: one call with the frame's shape; the passes render depth and normal (the guides); rgb_raw is the undenoised frame, se and
    # count the measured ones
    prm = DenoiseParams(levels=3, k_c=2.0)
    acc, stub = DenoisingAccumulator(1, P), StubRender()
    ims, stats = render_frame(None, rays, 50.0, spp=4, jitter=False, keys=keys, accumulator=acc, render=stub, denoise=prm, frame_hw=(Hf, Wf))
    assert acc.denoised == [(prm, (Hf, Wf), ("rgb_map", "rgb_lin"))] and stats == dict(passes=4, rays_rendered=4 * P)
    assert set(ims) == set(keys) | {"se", "count"} and all({"depth", "world_normal"} <= set(k) for _, k in stub.calls)
    assert torch.equal(ims["rgb_raw"], plain["rgb_map"]) and torch.equal(ims["se"], plain["se"]) and torch.equal(ims["count"], plain["count"])
    want = denoise_np(acc.st, Hf, Wf, **prm.record())
    assert np.array_equal(ims["rgb_map"].numpy(), want["rgb_map"]) and np.array_equal(ims["rgb_lin"].numpy(), want["rgb_lin"])
    still = (ims["se"] == 0).numpy()
    assert 0 < still.sum() < P and torch.equal(ims["rgb_map"][still], ims["rgb_raw"][still])
    # only rgb_raw asked for beside the depth: no rgb_map key comes back
    ims, _ = render_frame(None, rays, 50.0, spp=2, jitter=False, keys=("rgb_raw",), accumulator=DenoisingAccumulator(1, P), render=StubRender(),
                          denoise=prm, frame_hw=(Hf, Wf))
    assert set(ims) == {"rgb_raw", "se", "count"}
    # refusals: one sample, a frame shape that is missing or does not hold the rays, something that is no DenoiseParams
    for kw, err in ((dict(spp=1), ValueError), (dict(frame_hw=None), ValueError), (dict(frame_hw=(Hf, Wf + 1)), ValueError),
                    (dict(frame_hw=(0, P)), ValueError), (dict(frame_hw=(P,)), ValueError), (dict(denoise=dict(levels=3)), TypeError),
                    (dict(denoise=True), TypeError)):
        args = dict(spp=4, jitter=False, accumulator=DenoisingAccumulator(1, P), render=StubRender(), denoise=prm, frame_hw=(Hf, Wf))
        args.update(kw)
        with pytest.raises(err):
            render_frame(None, rays, 50.0, **args)
