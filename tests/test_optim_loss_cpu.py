"""The kernels that close every training step (csrc/adam.hip, csrc/loss.hip) on the CPU: inputs, float64 references, fp32 restatements
and the bounds that tests/test_hip_optim_loss.py holds the kernels to -- and the proof that those bounds mean something.

ADAM.  adam_ref() is one step per element as the header comment of adam.hip states it, in float64 (np.longdouble for an fp64 slot), on
the slot's double hyperparameters.  Beside it runs a first-order running-error bound: every operation of adam_one contributes 2^-24 of
its result's magnitude plus one denormal spacing 2^-149 (2^-53 / 2^-1074 in an fp64 slot), every hyperparameter cast 2^-24 of its
value, propagated through products (|a| E_b + |b| E_a), the square root (E_v / (2 sqrt v), capped at sqrt(E_v)) and the quotient
(E_m / den + |r| E_den / den) -> E_p, E_m, E_v per element.  What the bound rests on in csrc/build.sh: -fno-fast-math and hipcc's
default -fhip-fp32-correctly-rounded-divide-sqrt (the device code of adam.hip divides with v_div_scale / v_div_fmas / v_div_fixup and
refines its square root: both correctly rounded, so neither term carries an extra ulp); no flush flag (the code object sets
float_denorm_mode_32 = 3, denormals are kept: the 2^-149 terms); adam.hip and loss.hip are not in the -ffp-contract=off list, so a
multiply may be fused into an add, which removes a rounding and stays inside the same bound.

adam_f32() restates adam_one in numpy float32 (one rounded operation at a time, both lerp branches, no fma) and must stay inside the
bound in every regime and hyperparameter set of the GPU test.  Worst ratio |restatement - ref64| / E over the 54 hyperparameter sets
(beta1 x beta2 x weight decay x step count), 20 000 elements each:

    regime          m       v       p
    ordinary        0.998   0.789   0.987
    tiny            0.999   0.442   0.748
    zero_g_live     0.846   0.716   0.993
    zero_g_denorm   0.278   0.450   0.750
    large_g         0.712   0.761   0.890
    all_zero        0.000   0.000   0.000      (p, m, v keep their bits)
    chained (4 st.) 0.840   0.786   0.967      (one gradient, then three zero gradients, each step from the fp32 state before it)

and the five wrong variants are outside it.  Share of the elements with p, m or v outside the bound, per regime in the order above
without all_zero (where every variant is the identity: 0 %), for the hyperparameter set that shows it best (4 000 elements each):

    eps_before_bc2     46.5 %  100 %  95.5 %  100 %   2.1 %     (needs sqrt v near eps, or bc2_sqrt far from 1: step 1 and 7)
    no_bc2            100 %    100 %  100 %   100 %  100 %
    beta1_as_weight   100 %    100 %  100 %   100 %  100 %      (beta1 = 0.5 is its own mutant and is left out)
    wd_after_moments  100 %    100 %  100 %   100 %  100 %      (the sets with weight decay 0.01)
    v_from_g          100 %    100 %  100 %   100 %  100 %      (with g = 0 only through the weight-decay term)

REDUCTIONS.  k_l1_fwd / k_mix_fwd / k_sqerr_fwd / k_loss_head sum in this shape: ceil(n / (blocks 256)) sequential adds per thread, a
6-level shuffle tree, 4 waves added by thread 0, then `blocks` float atomics per tensor in any order (k_loss_head: a second pass of
ceil(blocks / 256) adds, the tree and the 4 waves again).  Each level contributes 2^-24 of the sum of magnitudes, so the bound is
gamma(L) x sum |terms| with gamma(L) = L u / (1 - L u) and L = the levels an element passes through, the roundings of the term itself
(2 casts + the division of the mean, 2 casts + 2 products of the mix, 3 for the squared difference) included.  l1_f32 / mix_f32 / sqerr_f32 /
head_f32 restate the shape in numpy float32 with the atomics in block order, reversed and shuffled.  Worst ratio |restatement - ref64| /
bound: l1 0.0084, mix 0.0019, sqerr 0.0219, loss_head 0.0413.  The bound is a worst case over all orders and signs, about 2e-5 of the sum at
256 workgroups: it sees a lost workgroup, not a lost element (test_what_the_reduction_bounds_catch), so the GPU tests also sum one-hot
tensors whose result is known exactly (one_hot_positions).

The backward kernels have no summation and no fusable multiply-add: their restatements (l1_bwd_f32, sqerr_bwd_f32, head_const_f32) are
the kernels' bits.
"""
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest

F32, F64 = np.float32, np.float64
U32, D32 = 2.0 ** -24, 2.0 ** -149
U64, D64 = 2.0 ** -53, 2.0 ** -1074

BETA1, BETA2, WDS, STEPS = (0.9, 0.5, 0.3), (0.9, 0.99, 0.999), (0.0, 0.01), (1, 7, 20000)
LR, EPS = 0.02, 1e-8
# (g, m, v) scales
REGIMES = {"ordinary": (1e-2, 1e-2, 1e-4), "tiny": (1e-20, 1e-20, 1e-40), "zero_g_live": (0.0, 1e-3, 1e-6),
           "zero_g_denorm": (0.0, 1e-39, 1e-41), "large_g": (1e1, 1e-6, 1e-30), "all_zero": (0.0, 0.0, 0.0)}
MUTANTS = ("eps_before_bc2", "no_bc2", "beta1_as_weight", "wd_after_moments", "v_from_g")


def hyper(beta1, beta2, wd, t, lr=LR, eps=EPS):
    """one slot's hyperparameters, bias-corrected on the host in double precision as FusedAdam does"""
    return SimpleNamespace(beta1=beta1, beta2=beta2, eps=eps, weight_decay=wd, step_size=lr / (1 - beta1 ** t),
                           bc2_sqrt=math.sqrt(1 - beta2 ** t), t=t)


HYPERS = [hyper(*c) for c in itertools.product(BETA1, BETA2, WDS, STEPS)]


def random_hyper(rng):
    """a slot whose every hyperparameter is its own: read with another slot's row it leaves its bound"""
    return SimpleNamespace(beta1=float(rng.choice([0.3, 0.9]) + 0.05 * rng.random()), beta2=float(0.9 + 0.099 * rng.random()),
                           eps=float(10.0 ** rng.uniform(-8, -6)), weight_decay=float(0.02 * rng.random()),
                           step_size=float(0.01 + 0.04 * rng.random()), bc2_sqrt=float(0.03 + 0.97 * rng.random()), t=0)


def make_state(n, regime, wd, rng, dtype=F32):
    """(p, g, m, v) of one regime.  all_zero: p is random without weight decay and zero with it, so that the step is the identity"""
    sg, sm, sv = REGIMES[regime]
    p = 0.5 * rng.standard_normal(n)
    if regime == "all_zero" and wd != 0:
        p = np.zeros(n)
    g, m, v = sg * rng.standard_normal(n), sm * rng.standard_normal(n), sv * rng.standard_normal(n) ** 2
    g, m = np.abs(g) if sg == 0 else g, np.abs(m) if sm == 0 else m          # a scale of 0 means +0.0
    return tuple(np.ascontiguousarray(x.astype(dtype)) for x in (p, g, m, v))


def make_mixed(n, wd, rng, run=37):
    """every regime in one tensor, in runs of 37 elements -> (p, g, m, v, regime index per element)"""
    names = list(REGIMES)
    which = (np.arange(n) // run) % len(names)
    out = [np.zeros(n, F32) for _ in range(4)]
    for k, name in enumerate(names):
        sel = which == k
        for o, x in zip(out, make_state(int(sel.sum()), name, wd, rng)):
            o[sel] = x
    return (*out, which)


# ---- Adam: float64 reference with its running-error bound ---------------------------------------------------------------------------
def adam_ref(p, g, m, v, h, f64_slot=False):
    """-> (p', m', v', E_p, E_m, E_v): one step in float64 (np.longdouble for an fp64 slot) and the bound on what adam_one<T> may return.
    An element whose gradient is not finite keeps p, m, v with a bound of 0."""
    wide, u, d = (np.longdouble, U64, D64) if f64_slot else (F64, U32, D32)
    g = np.asarray(g)
    keep = ~np.isfinite(g)
    p0, m0, v0 = (np.asarray(x).astype(wide) for x in (p, m, v))
    p, m, v, g = p0, m0, v0, np.where(keep, 0, g).astype(wide)
    wd, omb1, b2, omb2 = wide(h.weight_decay), wide(1.0 - h.beta1), wide(h.beta2), wide(1.0 - h.beta2)
    step, bc2, eps = wide(h.step_size), wide(h.bc2_sqrt), wide(h.eps)
    mag = lambda x: np.abs(x).astype(F64)            # noqa: E731
    rnd = lambda x: u * mag(x) + d                    # noqa: E731  (one rounded operation with result x)
    if h.weight_decay != 0:
        t = wd * p
        g = g + t
        E_g = u * mag(t) + rnd(t) + rnd(g)            # the cast of wd, the product, the sum
    else:
        E_g = np.zeros(g.shape, F64)
    diff = g - m
    E_diff = E_g + rnd(diff)
    low = (omb1 if f64_slot else F32(omb1)) < 0.5     # at::lerp's branch, taken in T
    m1 = m + omb1 * diff
    if low:                                           # m + w * diff
        pr = omb1 * diff
        E_m = float(omb1) * E_diff + u * mag(pr) + rnd(pr) + rnd(m1)
    else:                                             # g - diff * (1 - w)
        w = 1 - omb1
        E_w = u * float(omb1) + u * abs(float(w)) + d
        pr = diff * w
        E_m = E_g + abs(float(w)) * E_diff + mag(diff) * E_w + rnd(pr) + rnd(m1)
    a = v * b2
    E_a = u * mag(a) + rnd(a)
    c1 = omb2 * g
    E_c1 = float(omb2) * E_g + u * mag(c1) + rnd(c1)
    c2 = c1 * g
    E_c2 = mag(g) * E_c1 + mag(c1) * E_g + rnd(c2)   # (g * g: 2 |g| E_g)
    v1 = a + c2
    E_v = E_a + E_c2 + rnd(v1)
    s = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        E_s = np.where(s > 0, E_v / (2 * mag(s)), np.inf)
    E_s = np.minimum(E_s, np.sqrt(E_v)) + rnd(s)     # correctly rounded sqrt: one rounding
    q = s / bc2
    E_q = E_s / float(bc2) + u * mag(q) + rnd(q)     # the cast of bc2_sqrt, the (correctly rounded) quotient
    den = q + eps
    E_den = E_q + u * float(eps) + rnd(den)
    r = m1 / den
    E_r = E_m / mag(den) + mag(r) * E_den / mag(den) + rnd(r)
    t = step * r
    E_t = float(step) * E_r + u * mag(t) + rnd(t)
    p1 = p - t
    E_p = E_t + rnd(p1)
    z = lambda new, old: np.where(keep, old, new)    # noqa: E731
    return z(p1, p0), z(m1, m0), z(v1, v0), z(E_p, 0.0), z(E_m, 0.0), z(E_v, 0.0)


def adam_f32(p, g, m, v, h, T=F32, mutant=None):
    """adam_one<T> one rounded operation at a time (numpy, no fma) -> (p', m', v'); mutant: one of MUTANTS"""
    p, g, m, v = (np.asarray(x, T) for x in (p, g, m, v))
    keep, p0, m0, v0 = ~np.isfinite(g), p, m, v
    g = np.where(keep, T(0), g)
    wd, omb1, b2, omb2 = T(h.weight_decay), T(1.0 - h.beta1), T(h.beta2), T(1.0 - h.beta2)
    step, bc2, eps = T(h.step_size), T(h.bc2_sqrt), T(h.eps)
    if wd != 0 and mutant != "wd_after_moments":
        g = g + wd * p
    diff = g - m
    if mutant == "beta1_as_weight":
        m = m + T(h.beta1) * diff
    else:
        m = m + omb1 * diff if omb1 < T(0.5) else g - diff * (T(1) - omb1)
    v = v * b2 + (omb2 * g if mutant == "v_from_g" else omb2 * g * g)
    with np.errstate(invalid="ignore"):                  # (v_from_g takes the root of a negative v: NaN, which is outside every bound)
        s = np.sqrt(v)
    if mutant == "eps_before_bc2":
        den = (s + eps) / bc2
    elif mutant == "no_bc2":
        den = s + eps
    else:
        den = s / bc2 + eps
    upd = (-step) * (m / den)
    if mutant == "wd_after_moments" and wd != 0:
        upd = upd + (-step) * (wd * p)
    p = p + upd
    assert p.dtype == T and m.dtype == T and v.dtype == T
    return np.where(keep, p0, p), np.where(keep, m0, m), np.where(keep, v0, v)


def ratios(got, ref):
    """worst |got - ref| / E of (p, m, v); an element with E == 0 must be equal"""
    out = []
    for x, r, E in zip(got, ref[:3], ref[3:]):
        err = np.abs(np.asarray(x).astype(r.dtype) - r).astype(F64)
        assert not err[E == 0].any(), "an element that must keep its value changed"
        out.append(float((err[E > 0] / E[E > 0]).max()) if (E > 0).any() else 0.0)
    return dict(zip("pmv", out))


def outside(got, ref):
    """share of the elements with p, m or v outside the bound"""
    bad = np.zeros(ref[0].shape, bool)
    for x, r, E in zip(got, ref[:3], ref[3:]):
        bad |= ~(np.abs(np.asarray(x).astype(r.dtype) - r).astype(F64) <= E)          # (a NaN is outside)
    return float(bad.mean())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- reductions: float64 references, the summation shape in fp32, its bound ----------------------------------------------------------
def gamma(levels, u=U32):
    return levels * u / (1 - levels * u)


def blocks_for(biggest):                              # loss.hip: blocks_for() of the l1 / mix kernels
    return min(max(-(-max(biggest, 1) // 2048), 1), 256)


def sqerr_blocks(n):                                  # nmf_sqerr_fwd
    return min(-(-n // 1024), 256)


def clip01(x):
    """fminf(fmaxf(x, 0), 1): a NaN becomes 0"""
    return np.fmin(np.fmax(x, 0), 1)


def tree_levels(n, blocks):
    return -(-max(n, 1) // (blocks * 256)) + 6 + 4


def l1_ref(xs):
    """sum_i mean |x_i| in float64, its bound under k_l1_fwd's summation shape (0-element tensors add nothing: t == 0 is not added)"""
    blocks = blocks_for(max(x.size for x in xs))
    val = sum(float(np.abs(x.astype(F64)).mean()) for x in xs if x.size)
    levels = max(tree_levels(x.size, blocks) for x in xs) + 2 + blocks * len(xs)      # + cast of n, the division; the atomics of all tensors
    return val, gamma(levels) * val


def l1_grad_ref(xs, d_out):
    return [float(d_out) * np.sign(x.astype(F64)) / max(x.size, 1) for x in xs]


def mix_ref(xs, ws, scale):
    blocks = blocks_for(max(x.size for x in xs))
    val = sum(float(scale) * float(w) * float(x.astype(F64).sum()) for x, w in zip(xs, ws))
    mags = sum(abs(float(scale) * float(w)) * float(np.abs(x.astype(F64)).sum()) for x, w in zip(xs, ws))
    levels = max(tree_levels(x.size, blocks) for x in xs) + 4 + blocks * len(xs)      # + 2 casts, 2 products
    return val, gamma(levels) * mags


def sqerr_terms64(pred, gt):
    return (clip01(pred.astype(F64)) - clip01(gt.astype(F64))) ** 2


def sqerr_ref(pred, gt):
    """sum (clip(pred) - clip(gt))^2 over all floats, bound under k_sqerr_fwd's shape"""
    n = pred.size
    val = float(sqerr_terms64(pred, gt).sum())
    if n == 0:
        return 0.0, 0.0
    blocks = sqerr_blocks(n)
    return val, gamma(3 + tree_levels(n, blocks) + blocks) * val


def sqerr_grad_ref(pred, gt, d_out):
    p = pred.astype(F64)
    return np.where((p >= 0) & (p <= 1), 2 * (p - clip01(gt.astype(F64))) * float(d_out), 0.0)


def head_ref(pred, gt):
    """the loss of k_loss_head: one term per thread, tree + waves, then the fixed second pass over the blocks' partial sums"""
    n = pred.size
    val = float(sqerr_terms64(pred, gt).sum())
    blocks = max(-(-n // 256), 1)
    return val, gamma(3 + 6 + 4 + -(-blocks // 256) + 6 + 4) * val


def _block_sum(v):
    """block_sum of loss.hip on [blocks, 256] fp32: lane 0 of the shuffle tree of each wave, the 4 waves added in order"""
    v = v.reshape(-1, 4, 64).copy()
    for d in (32, 16, 8, 4, 2, 1):
        v[:, :, :d] = v[:, :, :d] + v[:, :, d:2 * d]
    t = np.zeros(v.shape[0], F32)
    for w in range(4):
        t = t + v[:, w, 0]
    return t


def block_partials(terms, blocks):
    """the per-block sums of a grid-stride loop over fp32 terms"""
    terms = np.asarray(terms, F32).reshape(-1)
    k = -(-terms.size // (blocks * 256))
    padded = np.zeros(k * blocks * 256, F32)
    padded[:terms.size] = terms
    a = np.zeros(blocks * 256, F32)
    for row in padded.reshape(k, blocks * 256):
        a = a + row
    return _block_sum(a.reshape(blocks, 256))


def atomic_orders(parts, rng):
    """fp32 sums of the parts added onto 0 one after the other: in order, reversed, shuffled"""
    outs = []
    for order in (np.arange(len(parts)), np.arange(len(parts))[::-1], rng.permutation(len(parts))):
        s = F32(0)
        for x in np.asarray(parts, F32)[order]:
            if x != 0:
                s = F32(s + x)
        outs.append(float(s))
    return outs


def l1_f32(xs, rng):
    blocks = blocks_for(max(x.size for x in xs))
    parts = [block_partials(np.abs(x), blocks) / F32(x.size) for x in xs if x.size]
    return atomic_orders(np.concatenate(parts), rng)


def mix_f32(xs, ws, scale, rng):
    blocks = blocks_for(max(x.size for x in xs))
    parts = [block_partials(x, blocks) * F32(w) * F32(scale) for x, w in zip(xs, ws) if x.size]
    return atomic_orders(np.concatenate(parts), rng)


def sqerr_terms32(pred, gt):
    d = (clip01(pred.astype(F32)) - clip01(gt.astype(F32))).astype(F32)
    return (d * d).astype(F32)


def sqerr_f32(pred, gt, rng):
    return atomic_orders(block_partials(sqerr_terms32(pred, gt), sqerr_blocks(pred.size)), rng)


def head_f32(pred, gt):
    t = sqerr_terms32(pred, gt).reshape(-1)
    blocks = max(-(-t.size // 256), 1)
    padded = np.zeros(blocks * 256, F32)
    padded[:t.size] = t
    partial = _block_sum(padded.reshape(blocks, 256))
    k = -(-blocks // 256)
    p2 = np.zeros(k * 256, F32)
    p2[:blocks] = partial
    a = np.zeros(256, F32)
    for row in p2.reshape(k, 256):
        a = a + row
    return float(_block_sum(a.reshape(1, 256))[0])


# ---- backward kernels: the kernels' bits ---------------------------------------------------------------------------------------------
def l1_bwd_f32(x, d_out, before=None):
    """k_l1_bwd: +-fp32(d_out / fp32(n)), 0 for +-0.0 (and NaN); before: the gradient it is added to (one fp32 add)"""
    with np.errstate(divide="ignore"):                   # (an empty tensor: nothing is written)
        s = F32(F32(d_out) / F32(x.size))
    gv = np.where(x > 0, s, np.where(x < 0, -s, F32(0))).astype(F32)
    return gv if before is None else (before + gv).astype(F32)


def sqerr_bwd_f32(pred, gt, s):
    """k_sqerr_bwd and the d_pred of k_loss_head: 2 (p - clip(gt)) s inside [0, 1], 0 outside (and for NaN)"""
    p, c = pred.astype(F32), clip01(gt.astype(F32)).astype(F32)
    with np.errstate(invalid="ignore"):
        d = (F32(2) * (p - c)).astype(F32) * F32(s)
        return np.where((p >= 0) & (p <= 1), d, F32(0)).astype(F32)


def head_const_f32(d_out, scale, w):
    """d_out * scale * w of k_loss_head / k_mix_bwd, left to right in fp32"""
    return F32(F32(F32(d_out) * F32(scale)) * F32(w))


def l1_inputs(n, rng):
    """30 % exact zeros, some -0.0"""
    x = rng.standard_normal(n).astype(F32)
    x[rng.random(n) < 0.3] = 0.0
    x[rng.random(n) < 0.02] = -0.0
    return x


L1_SETS = ((524288, 1, 5, 0), (524289, 5, 1), (1440000, 0, 1, 5))
SQERR_RAYS = (87381, 87382, 200001)
HEAD_RAYS = (33001, 1, 0, 33001, 70000)


def sqerr_inputs(B, rng):
    pred = (rng.random((B, 3)) * 1.6 - 0.3).astype(F32)
    gt = (rng.random((B, 3)) * 1.4 - 0.2).astype(F32)          # below 0 and above 1 too
    return pred, gt


def prints(*a):
    print(*a, flush=True)


# ---- tests -------------------------------------------------------------------------------------------------------------------------
N_CPU = 20000


def _chain(h0, rng, step_fn):
    """4 steps from zero moments: one gradient, then three zero gradients; every step is checked from the restatement's own fp32 state"""
    p, g, m, v = make_state(N_CPU, "ordinary", h0.weight_decay, rng)
    m, v = np.zeros_like(m), np.zeros_like(v)
    worst = dict.fromkeys("pmv", 0.0)
    for t in range(1, 5):
        h = hyper(h0.beta1, h0.beta2, h0.weight_decay, t)
        gt = g if t == 1 else np.zeros_like(g)
        ref = adam_ref(p, gt, m, v, h)
        p, m, v = step_fn(p, gt, m, v, h)
        for k, r in ratios((p, m, v), ref).items():
            worst[k] = max(worst[k], r)
    return worst


def test_adam_restatement_stays_inside_the_bound_in_every_regime():
    for regime in REGIMES:
        worst = dict.fromkeys("pmv", 0.0)
        for i, h in enumerate(HYPERS):
            rng = np.random.default_rng([3, i, list(REGIMES).index(regime)])
            p, g, m, v = make_state(N_CPU, regime, h.weight_decay, rng)
            ref = adam_ref(p, g, m, v, h)
            got = adam_f32(p, g, m, v, h)
            for k, r in ratios(got, ref).items():
                worst[k] = max(worst[k], r)
            if regime == "all_zero":
                assert all(same_bits(a, b) for a, b in zip(got, (p, m, v)))
        prints(f"adam restatement / bound, {regime}: m {worst['m']:.3f} v {worst['v']:.3f} p {worst['p']:.3f}")
        assert max(worst.values()) <= 1.0, (regime, worst)
    worst = dict.fromkeys("pmv", 0.0)
    for i, h in enumerate(HYPERS):
        if h.t == 1:
            for k, r in _chain(h, np.random.default_rng([4, i]), adam_f32).items():
                worst[k] = max(worst[k], r)
    prints(f"adam restatement / bound, chained: m {worst['m']:.3f} v {worst['v']:.3f} p {worst['p']:.3f}")
    assert max(worst.values()) <= 1.0, worst


def test_adam_restatement_in_an_fp64_slot_and_a_mixed_tensor():
    rng = np.random.default_rng(5)
    for h in HYPERS[::5]:
        p, g, m, v = make_state(2000, "ordinary", h.weight_decay, rng, dtype=F64)
        r = ratios(adam_f32(p, g, m, v, h, T=F64), adam_ref(p, g, m, v, h, f64_slot=True))
        assert max(r.values()) <= 1.0, r
        p, g, m, v, which = make_mixed(5000, h.weight_decay, rng)
        got, ref = adam_f32(p, g, m, v, h), adam_ref(p, g, m, v, h)
        assert max(ratios(got, ref).values()) <= 1.0
        z = which == list(REGIMES).index("all_zero")
        assert all(same_bits(a[z], b[z]) for a, b in zip(got, (p, m, v)))
    g[:8] = [np.inf, -np.inf, np.nan, 1.0, np.nan, 2.0, np.inf, 3.0]
    got, ref = adam_f32(p, g, m, v, h), adam_ref(p, g, m, v, h)
    bad = ~np.isfinite(g)
    assert all(same_bits(a[bad], b[bad]) for a, b in zip(got, (p, m, v))) and max(ratios(got, ref).values()) <= 1.0


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_bound_catches_a_wrong_adam(mutant):
    share = {}
    for regime in REGIMES:
        worst = 0.0
        for i, h in enumerate(HYPERS):
            if mutant == "beta1_as_weight" and h.beta1 == 0.5:
                continue                                 # beta1 == 1 - beta1
            rng = np.random.default_rng([6, i, list(REGIMES).index(regime)])
            p, g, m, v = make_state(4000, regime, h.weight_decay, rng)
            worst = max(worst, outside(adam_f32(p, g, m, v, h, mutant=mutant), adam_ref(p, g, m, v, h)))
        share[regime] = worst
    prints(f"mutant {mutant}: share outside the bound (worst hyperparameter set) " +
           ", ".join(f"{k} {100 * s:.1f} %" for k, s in share.items()))
    assert max(share.values()) > 0.0
    assert share["all_zero"] == 0.0                      # nothing to get wrong there


def test_reduction_restatements_stay_inside_their_bounds():
    rng = np.random.default_rng(7)
    worst = dict(l1=0.0, mix=0.0, sqerr=0.0, head=0.0)
    for sizes in L1_SETS:
        xs = [l1_inputs(n, rng) for n in sizes]
        val, bound = l1_ref(xs)
        worst["l1"] = max(worst["l1"], max(abs(s - val) for s in l1_f32(xs, rng)) / bound)
        xs = [rng.standard_normal(n).astype(F32) + F32(0.25) for n in sizes]
        ws = [0.37, -1.3, 0.013, 2.0][:len(xs)]
        val, bound = mix_ref(xs, ws, 1.0 / 7.0)
        worst["mix"] = max(worst["mix"], max(abs(s - val) for s in mix_f32(xs, ws, 1.0 / 7.0, rng)) / bound)
    for B in SQERR_RAYS:
        pred, gt = sqerr_inputs(B, rng)
        val, bound = sqerr_ref(pred, gt)
        worst["sqerr"] = max(worst["sqerr"], max(abs(s - val) for s in sqerr_f32(pred, gt, rng)) / bound)
    for B in HEAD_RAYS:
        pred, gt = sqerr_inputs(B, rng)
        val, bound = head_ref(pred, gt)
        got = head_f32(pred, gt)
        if B == 0:
            assert got == 0.0 and val == 0.0
        else:
            worst["head"] = max(worst["head"], abs(got - val) / bound)
    prints("reduction restatement / bound: " + ", ".join(f"{k} {r:.4f}" for k, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_what_the_reduction_bounds_catch():
    """A worst-case bound over ~300 levels is about 2e-5 of the sum: a sum that drops one workgroup's share of a pass is outside it, one
    that drops a single element of half a million is not.  So the GPU tests also sum ONE-HOT tensors (one_hot_positions), where a
    dropped or doubled element changes an exactly known result."""
    rng = np.random.default_rng(8)
    x = l1_inputs(524289, rng)
    val, bound = l1_ref([x])
    a = np.abs(x.astype(F64))
    assert abs(a[256:].sum() / x.size - val) > bound            # one workgroup's first 256
    assert abs(a[:-1].sum() / x.size - val) < bound             # the one element of the second pass: the bound cannot see it
    pred, gt = sqerr_inputs(SQERR_RAYS[1], rng)
    val, bound = sqerr_ref(pred, gt)
    terms = sqerr_terms64(pred, gt).reshape(-1)
    assert terms[256:].sum() < val - bound
    assert one_hot_positions(524289, 524288) == [0, 524287, 524288] and one_hot_positions(5, 524288) == [0, 4]


def one_hot_positions(n, per_pass):
    """the first element, the last of the first pass, the first of every later pass, the last element"""
    pos = {0, n - 1} | {k for k in range(per_pass, n, per_pass)} | ({per_pass - 1} if n > per_pass else set())
    return sorted(pos)


def test_backward_restatements_equal_float64_to_rounding():
    rng = np.random.default_rng(9)
    x = l1_inputs(1001, rng)
    g = l1_bwd_f32(x, 3.0)
    assert np.allclose(g, l1_grad_ref([x], 3.0)[0], rtol=2e-7, atol=0) and not g[x == 0].any()
    pred, gt = sqerr_inputs(1001, rng)
    pred.reshape(-1)[:6] = [0.0, -0.0, 1.0, np.nextafter(F32(1), F32(2)), np.nextafter(F32(0), F32(-1)), np.nan]
    d = sqerr_bwd_f32(pred, gt, 0.5)
    ref = sqerr_grad_ref(pred, gt, 0.5)
    assert np.allclose(d, ref, rtol=3e-7, atol=0) and not d.reshape(-1)[3:6].any() and d.reshape(-1)[2] != 0
