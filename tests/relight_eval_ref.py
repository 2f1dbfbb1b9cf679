"""The relighting evaluation restated in numpy, for tests/test_relight_eval_cpu.py and tests/test_hip_relight_eval.py.

Written from the cited lines of the reference, not copied from them: modules/tonemap.py:38-55 (the sRGB pair), renderer.py:425-429
(the HDR frame), scripts/relighting_calc.ipynb cell lines 230-234 (mask, ratio, multiplier) and 243-254 (adjusted frames, PSNR).
Every function takes `dt`: np.float64 is the restatement the kernels are held to; np.float32 follows the expression order of
nmf_amd/csrc/relight_eval.hip operation by operation (contraction is off there), so it differs from the kernels by powf alone and its
distance from the float64 one measures what fp32 rounding does to these expressions.  The GPU tolerance is 4 x that distance
(margins()), as tests/test_relight_cpu.py:restatement_margin does for the resampling kernel.

The mask compares the stored fp32 values with the fp32 constants 0.5 and 0.01 in both precisions: that is what numpy does with a
float32 array and a Python scalar, and it is a decision, not arithmetic.
"""
import numpy as np

SHAPES = ((1, 1, 1), (3, 5, 7), (3, 33, 67))       # (n_img, H, W): one pixel; less than a wave; 2211 pixels = two workgroups of 2048
GAINS = (0.5, 1.0, 2.0)


def srgb(x, dt, clip):
    x = np.asarray(x, dtype=dt)
    limit = dt(0.0031308)
    with np.errstate(invalid="ignore"):
        out = np.where(x > limit, dt(1.055) * np.power(np.maximum(x, limit), dt(1.0) / dt(2.4)) - dt(0.055), dt(12.92) * x)
    return np.clip(out, dt(0), dt(1)) if clip else out


def srgb_inverse(y, dt):
    y = np.asarray(y, dtype=dt)
    with np.errstate(invalid="ignore"):
        return np.where(y > dt(0.04045), np.power((y + dt(0.055)) / dt(1.055), dt(2.4)), y / dt(12.92))


def frame(rgb_lin, acc, dt=np.float64):
    """[..., 3], [...] -> the HDR frame srgb_inverse(srgb_noclip(rgb_lin) + (1 - acc))"""
    t = dt(1) - np.asarray(acc, dtype=dt)[..., None]
    return srgb_inverse(srgb(rgb_lin, dt, False) + t, dt)


def mask(pred, gt):
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    return (gt[..., 3] > np.float32(0.5)) & (pred.min(axis=-1) > np.float32(0.01))


def ratio(pred, gt, dt=np.float64):
    """pred [n,H,W,3], gt [n,H,W,4] -> (sums float64 [n,3] of gt_c / max(pred_c, 1e-7) over the mask, each term formed in dt,
    counts int64 [n])"""
    m = mask(pred, gt)
    term = np.asarray(gt, dtype=dt)[..., :3] / np.maximum(np.asarray(pred, dtype=dt), dt(1e-7))
    term = np.where(m[..., None], term.astype(np.float64), 0.0)
    return term.sum(axis=(1, 2)), m.sum(axis=(1, 2)).astype(np.int64)


def adjust(pred, gt, multi, dt=np.float64):
    """-> (tp, tg [n,H,W,3] in dt, sqerr float64 [n] = the sum of the dt terms (tp - tg)^2)"""
    pred, gt = np.asarray(pred, dtype=dt), np.asarray(gt, dtype=dt)
    a = gt[..., 3:4]
    w = dt(1) - a
    tp = srgb((pred * np.asarray(multi, dtype=dt).reshape(1, 1, 1, 3)) * a + w, dt, True)
    tg = srgb(gt[..., :3] + w, dt, True)
    d = tp - tg
    return tp, tg, (d * d).astype(np.float64).sum(axis=(1, 2, 3))


def multiplier(sums, counts):
    """mean over the images with a non-empty mask of their per-image means (an empty one is left out, not NaN: DESIGN.md 10.6)"""
    used = counts > 0
    return (sums[used] / counts[used, None]).mean(axis=0)


def protocol(preds, gts):
    """the whole notebook in float64 on fp32 frames: -> (multi [3], psnrs [n], tp, tg)"""
    sums, counts = ratio(preds, gts)
    multi = multiplier(sums, counts)
    tp, tg, sqerr = adjust(preds, gts, multi)
    n_px = preds.shape[1] * preds.shape[2]
    with np.errstate(divide="ignore"):
        return multi, -10.0 * np.log10(sqerr / (3.0 * n_px)), tp, tg


# ---- inputs that reach every branch -------------------------------------------------------------------------------------------------
F32 = np.float32
UP = lambda v: np.nextafter(F32(v), F32(np.inf))          # noqa: E731
DOWN = lambda v: np.nextafter(F32(v), F32(-np.inf))       # noqa: E731
# (pred rgb, gt alpha, in the mask?) placed at the first pixels of image 0.  0.5 and 0.01 exactly are excluded (strict comparisons),
# their fp32 successors are included; 0 and negative values meet the 1e-7 clip (and are excluded by the 0.01 test, like a NaN)
SPECIAL = (
    ((0.3, 0.4, 0.5), 0.5, False),
    ((0.3, 0.4, 0.5), UP(0.5), True),
    ((0.01, 0.4, 0.5), 1.0, False),
    ((UP(0.01), 0.4, 0.5), 1.0, True),
    ((0.01, 0.4, 0.5), 0.5, False),
    ((0.0, 0.4, 0.5), 1.0, False),
    ((-0.3, 0.4, 0.5), 1.0, False),
    ((5.0, 1e-9, 0.2), 0.75, False),
    ((0.0031308, UP(0.0031308), DOWN(0.0031308)), 1.0, False),
    ((0.0031308 * 1.001, 0.0031308 * 0.999, 0.02), 1.0, False),
    ((0.02, 0.0125, 40.0), 1.0, True),
    ((0.02, 0.0125, 40.0), 0.0, False),
)


def inputs(n_img, H, W, seed=0):
    """-> pred [n,H,W,3], gt [n,H,W,4] fp32.  pred: log-uniform 1e-4 .. 50 with a tenth of the values zero or negative; gt colour
    log-uniform 1e-3 .. 1e4; gt alpha from {0, 0.25, 0.5, its successor, 0.75, 1} and uniform values.  Image 0 starts with the SPECIAL
    pixels (as many as fit); with more than one image, image 1 has no alpha above 0.5: an empty mask."""
    rng = np.random.default_rng(seed + 1000 * n_img + 10 * H + W)
    shape = (n_img, H, W)
    pred = np.exp(rng.uniform(np.log(1e-4), np.log(50.0), size=shape + (3,)))
    low = rng.uniform(size=shape + (3,)) < 0.1
    pred = np.where(low, rng.uniform(-0.5, 0.0, size=shape + (3,)) * (rng.uniform(size=shape + (3,)) < 0.5), pred)
    rgb = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), size=shape + (3,)))
    fixed = np.array([0.0, 0.25, 0.5, UP(0.5), 0.75, 1.0])
    alpha = np.where(rng.uniform(size=shape) < 0.6, fixed[rng.integers(0, len(fixed), size=shape)], rng.uniform(size=shape))
    pred, gt = pred.astype(F32), np.concatenate([rgb, alpha[..., None]], axis=-1).astype(F32)
    flat_p, flat_g = pred[0].reshape(-1, 3), gt[0].reshape(-1, 4)
    for k, (p, a, _) in enumerate(SPECIAL[:flat_p.shape[0]]):
        flat_p[k] = np.asarray(p, dtype=F32)
        flat_g[k, 3] = F32(a)
    if n_img > 1:
        gt[1, ..., 3] = np.minimum(gt[1, ..., 3], F32(0.5))
    return pred, gt


def frame_inputs(n_img, H, W, seed=0):
    """-> rgb_lin [n,H,W,3], acc [n,H,W] fp32 for nmf_relight_frame: inputs()' pred values (both sides of the forward limit, negative,
    zero, above 1) and alphas; with acc = 1 the forward limit maps onto the inverse limit, so both are met from both sides"""
    pred, gt = inputs(n_img, H, W, seed)
    return pred, np.ascontiguousarray(gt[..., 3])


def rel_floor1(got, want):
    """|got - want| relative to max(|want|, 1): the HDR frame is unbounded above, and near zero it is a difference of O(1) terms"""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(np.abs(want), 1.0)


def margins(multi=GAINS):
    """4 x the largest distance of the fp32 restatement from the float64 one over the inputs of every shape in SHAPES (the worst
    case of all, as restatement_margin takes it: one pixel alone says little about rounding) -> dict(frame: relative with floor 1,
    tp, tg: absolute)"""
    worst = dict(frame=0.0, tp=0.0, tg=0.0)
    for shape in SHAPES:
        lin, acc = frame_inputs(*shape)
        pred, gt = inputs(*shape)
        tp32, tg32, _ = adjust(pred, gt, multi, np.float32)
        tp64, tg64, _ = adjust(pred, gt, multi, np.float64)
        worst["frame"] = max(worst["frame"], float(rel_floor1(frame(lin, acc, np.float32), frame(lin, acc, np.float64)).max()))
        worst["tp"] = max(worst["tp"], float(np.abs(tp32.astype(np.float64) - tp64).max()))
        worst["tg"] = max(worst["tg"], float(np.abs(tg32.astype(np.float64) - tg64).max()))
    return {k: 4 * v for k, v in worst.items()}
