"""The VM field (csrc/vm.hip) on the CPU: inputs, a float64 reference, an fp32 restatement and the margins that tests/test_hip_vm.py holds
the kernels to -- and the proof that those margins mean something.

FOOTPRINTS.  normalized / make_tap1 / make_tap2 / brick_of are restated in numpy float32 one rounded operation at a time (the kernel
compiles them with contraction off, so texel indices, weights and bricks are the kernel's bits).  The fp32 weights are INPUTS of the
float64 reference: the rounding of the texel coordinate (~ G 2^-24) is not the error under test.

REFERENCE (float64).  forward(): sigma_feat, sigma, grad, normal, app, coef from the packed tables and the weights.  pack_tables() /
unpack_grads(): the 5x5 stencil of hip.derivative_stencil_rows() with zero padding 2 and its transpose (+ the l1 term, sign(0) = 0).
backward(): the per-sample adjoints of sample_adjoint_finish, then the scatter  weight x adjoint x other factor  into g_dpk (48 ch),
g_dlk (32), the appearance planes and lines (24) and g_basis = d_app^T coef, summed with np.bincount in float64.  Next to every
gradient entry e it returns S(e), the float64 sum of the ABSOLUTE values of everything that is added up for e -- the same expressions
evaluated on |weights|, |tables|, |adjoints|, so a cancellation inside one sample's factor counts as the separate terms it is -- and
the entries nothing reaches (S == 0): these must be exactly 0.0 on the device.  test_reference_agrees_with_the_float64_oracle
checks this hand-written reference (given float64 weights) against oracle/nmf_oracle.py and autograd in float64.

RESTATEMENT (fp32).  The same sums in float32: the density forward with the kernel's fmaf chains in tap and channel order (an fma is
emulated as the float64 product and sum rounded once), everything the source leaves to the compiler or to atomics / the MFMA
accumulator as plain float32 operations, the scatter sums added one after the other (np.add.at) in three sample orders -- as given,
brick-sorted, reversed -- and the worst of the three taken.

METRICS.  Gradient tables: |got - ref64| / S(e) over the entries with S(e) > 0, maximised per table kind; sigma_feat, grad, app, coef,
pack and unpack: |err| / the float64 sum of absolute terms of that output; sigma and normal: absolute error.  MARGINS: the project's
rule, max(8 x the restatement's error, 2^-23 x scale) (scale = 1 for the relative metrics), computed here per case, nothing hard-coded.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nmf_amd import hip
from oracle import nmf_oracle as O
from test_shading_rows_cpu import FLOOR, _big

F32, F64 = np.float32, np.float64
CD, CA, AD, DP, DL, BR = 16, 24, 24, 48, 32, 4
MAT0, MAT1, VEC = (0, 0, 1), (1, 2, 2), (2, 1, 0)
AABB = np.array([[-1.5, -1.0, -2.0], [1.5, 1.25, 1.0]], dtype=F32)          # not a cube: three different inv_size
INV = (F32(2.0) / (AABB[1] - AABB[0])).astype(F32)
SHIFT = F32(-4.0)
EPS = F32(1.1920929e-07)
GRIDS = (16, 17, 19, 57, 104, 129)
LADDER = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700)
ITEM = 128                                   # samples per work item up to 400 000 samples, 256 above (plan_layout)
GRAD_FLOOR = 0.01                            # float64 |g| of every sample of the standard tables over the norm of its sums of |terms|: no
                                             # gradient is the remainder of a cancellation (a sample that only just reaches the grid has a
                                             # small |g| with small terms, which the unit normal takes as well as any other)
SHAPES = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257)
EDGE_CLASSES = ("integer", "zero", "last", "below0", "out_low", "out_high", "brick_below", "brick_on", "brick_above")


# ---- footprints: the kernel's bits -------------------------------------------------------------------------------------------------
def normalized(x):
    return ((x[:, :3] - AABB[0]) * INV - F32(1.0)).astype(F32)


def texel_coord(xn, G):
    return (((xn + F32(1.0)) * F32(0.5)) * F32(G - 1)).astype(F32)


def half_coord(xn):
    return ((xn + F32(1.0)) * F32(0.5)).astype(F32)


def _frac(xn, G, weights):
    """(x0, w): floor and fractional part of the texel coordinate.  weights: "f32" the kernel's bits; "fused" the fraction taken from
    the UNROUNDED product (what an fma(t, G - 1, -floor) returns); "f64" everything in float64 (for the comparison with the oracle)"""
    if weights == "f64":
        ix = ((xn.astype(F64) + 1.0) * 0.5) * (G - 1)
        f = np.floor(ix)
        return f.astype(np.int64), ix - f
    ix = texel_coord(xn, G)
    f = np.floor(ix)
    if weights == "fused":
        return f.astype(np.int64), (half_coord(xn).astype(F64) * F64(G - 1) - f.astype(F64)).astype(F32)
    return f.astype(np.int64), (ix - f).astype(F32)


def brick_of(xn, G):
    nbx = (G + BR - 1) // BR
    b = np.clip(np.floor(texel_coord(xn, G)).astype(np.int64), 0, G - 1) // BR
    return (b[:, 2] * nbx + b[:, 1]) * nbx + b[:, 0]


def footprints(x, G, weights="f32"):
    """PI [3,M,4] texel (y G + x, -1 outside) and PW [3,M,4] weights in the order nw, ne, sw, se; LI [3,M,2], LW [3,M,2]"""
    xn = normalized(x) if weights != "f64" else (x[:, :3].astype(F64) - AABB[0].astype(F64)) * INV.astype(F64) - 1.0
    x0, w = _frac(xn, G, weights)
    one = w.dtype.type(1.0)
    e = one - w
    ins0, ins1 = (x0 >= 0) & (x0 < G), (x0 + 1 >= 0) & (x0 + 1 < G)
    M = len(x)
    PI, PW = np.full((3, M, 4), -1, np.int64), np.zeros((3, M, 4), w.dtype)
    LI, LW = np.full((3, M, 2), -1, np.int64), np.zeros((3, M, 2), w.dtype)
    for i in range(3):
        a, b, c = MAT0[i], MAT1[i], VEC[i]
        taps = ((ins0[:, a] & ins0[:, b], x0[:, b] * G + x0[:, a], e[:, a] * e[:, b]),
                (ins1[:, a] & ins0[:, b], x0[:, b] * G + x0[:, a] + 1, w[:, a] * e[:, b]),
                (ins0[:, a] & ins1[:, b], (x0[:, b] + 1) * G + x0[:, a], e[:, a] * w[:, b]),
                (ins1[:, a] & ins1[:, b], (x0[:, b] + 1) * G + x0[:, a] + 1, w[:, a] * w[:, b]))
        for t, (ok, idx, wt) in enumerate(taps):
            PI[i, :, t] = np.where(ok, idx, -1)
            PW[i, :, t] = np.where(ok, wt, 0)
        LI[i, :, 0], LW[i, :, 0] = np.where(ins0[:, c], x0[:, c], -1), np.where(ins0[:, c], e[:, c], 0)
        LI[i, :, 1], LW[i, :, 1] = np.where(ins1[:, c], x0[:, c] + 1, -1), np.where(ins1[:, c], w[:, c], 0)
    xn32 = normalized(x)
    return SimpleNamespace(G=G, M=M, PI=PI, PW=PW, LI=LI, LW=LW, x0=x0, ix=texel_coord(xn32, G), brick=brick_of(xn32, G))


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def stencil():
    """the 5x5 x-stencil kx (rows 0 and 4 and column 2 are zero); ky = kx^T"""
    c, o = hip.derivative_stencil_rows()
    k = np.zeros((5, 5), F32)
    k[1], k[2], k[3] = o, c, o
    return k


def bf16_round(a):
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)


def pack_tables(planes, lines, dt=F64, absolute=False):
    """-> (dpk [3][G*G,48], dlk [3][G,32]) = (P | corr_x P | corr_y P), (L | corr L), zero padding 2.  absolute: the sums of |terms|"""
    k = stencil().astype(dt, copy=False)
    if absolute:
        k, planes, lines = np.abs(k), [np.abs(p) for p in planes], [np.abs(ln) for ln in lines]
    dpk, dlk = [], []
    for P, L in zip(planes, lines):
        G = P.shape[0]
        pad = np.zeros((G + 4, G + 4, CD), dt)
        pad[2:-2, 2:-2] = P
        dx, dy = np.zeros((G, G, CD), dt), np.zeros((G, G, CD), dt)
        for i in (1, 2, 3):
            for j in (0, 1, 3, 4):
                dx = dx + k[i, j] * pad[i:i + G, j:j + G]
                dy = dy + k[i, j] * pad[j:j + G, i:i + G]
        dpk.append(np.concatenate([P.astype(dt, copy=False), dx, dy], axis=2).reshape(G * G, DP))
        lp = np.zeros((G + 4, CD), dt)
        lp[2:-2] = L
        d = np.zeros((G, CD), dt)
        for i in (0, 1, 3, 4):
            d = d + k[2, i] * lp[i:i + G]
        dlk.append(np.concatenate([L.astype(dt, copy=False), d], axis=1))
    return dpk, dlk


def unpack_grads(g_dpk, g_dlk, G, dt=F64, absolute=False, x=None, l1=None):
    """transpose of pack_tables: -> (gP [3][G,G,16], gL [3][G,16]); x = (planes, lines), l1: + l1 / n * sign(x)"""
    k = stencil().astype(dt, copy=False)
    if absolute:
        k, g_dpk, g_dlk = np.abs(k), [np.abs(g) for g in g_dpk], [np.abs(g) for g in g_dlk]
    gP, gL = [], []
    for n, (gp, gl) in enumerate(zip(g_dpk, g_dlk)):
        gp = np.asarray(gp, dt).reshape(G, G, DP)
        pad = np.zeros((G + 4, G + 4, DP), dt)
        pad[2:-2, 2:-2] = gp
        acc = gp[:, :, :CD].copy()
        for i in (1, 2, 3):
            for j in (0, 1, 3, 4):
                acc = acc + k[i, j] * pad[4 - i:4 - i + G, 4 - j:4 - j + G, CD:2 * CD]
                acc = acc + k[i, j] * pad[4 - j:4 - j + G, 4 - i:4 - i + G, 2 * CD:]
        lp = np.zeros((G + 4, DL), dt)
        lp[2:-2] = gl
        al = np.asarray(gl, dt)[:, :CD].copy()
        for i in (0, 1, 3, 4):
            al = al + k[2, i] * lp[4 - i:4 - i + G, CD:]
        if x is not None:
            xp, xl = np.asarray(x[0][n], dt), np.asarray(x[1][n], dt)
            sp, sl = dt(l1) / dt(xp.size), dt(l1) / dt(xl.size)
            acc = acc + (np.abs(np.sign(xp)) if absolute else np.sign(xp)) * sp
            al = al + (np.abs(np.sign(xl)) if absolute else np.sign(xl)) * sl
        gP.append(acc)
        gL.append(al)
    return gP, gL


@functools.lru_cache(maxsize=None)
def tables(G, kind="std"):
    """the field's tables at grid G: raw density factors, the packed tables (float64 pack rounded to fp32: GIVEN values for every query),
    appearance factors, basis -- and the bf16 copy of each (fp32 values rounded to bf16).  kind "std": random values + a unit offset on
    channel 0 of the planes and a linear ramp (0.25 per texel, centred) on channel 0 of the lines, which keeps |g| of every sample away
    from 0 and spreads sigma_feat over the clamp at -15 and the softplus threshold; kind "special": a patch of plane 0 scaled so that
    sigma_feat passes 1e3, and an all-zero corner of every plane (|g|^2 <= eps)"""
    rng = np.random.default_rng([5, G])
    r = lambda *s: rng.standard_normal(s).astype(F32)      # noqa: E731
    planes = [F32(0.1) * r(G, G, CD) for _ in range(3)]
    lines = [F32(0.1) * r(G, CD) for _ in range(3)]
    ramp = (F32(0.25) * (np.arange(G, dtype=F32) - F32(0.5 * (G - 1)))).astype(F32)
    for i in range(3):
        planes[i][:, :, 0] += F32(1.0)
        lines[i][:, 0] += ramp
    if kind == "special":
        planes[0][:4, :4, 0] = F32(900.0)
        for i in range(3):
            planes[i][G - 8:, G - 8:, :] = F32(0.0)
    apl = [F32(0.3) * r(G, G, CA) for _ in range(3)]
    ali = [F32(0.3) * r(G, CA) for _ in range(3)]
    basis = F32(0.2) * r(AD, 3 * CA)
    d64, l64 = pack_tables(planes, lines)
    dpk, dlk = [t.astype(F32) for t in d64], [t.astype(F32) for t in l64]
    apl = [a.reshape(G * G, CA) for a in apl]
    fp32 = SimpleNamespace(dpk=dpk, dlk=dlk, apl=apl, ali=ali, basis=basis)
    bf16 = SimpleNamespace(dpk=[bf16_round(t) for t in dpk], dlk=[bf16_round(t) for t in dlk], apl=[bf16_round(t) for t in apl],
                           ali=[bf16_round(t) for t in ali], basis=basis)
    raw = SimpleNamespace(dpk=[p.reshape(G * G, CD) for p in planes], dlk=lines)
    raw16 = SimpleNamespace(dpk=[bf16_round(t) for t in raw.dpk], dlk=[bf16_round(t) for t in raw.dlk])
    out = SimpleNamespace(G=G, planes=planes, lines=lines, fp32=fp32, bf16=bf16, raw=raw, raw16=raw16)
    for ns in (fp32, bf16, raw, raw16):
        for v in vars(ns).values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
    return out


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _gather(tab, idx):
    return tab[np.maximum(idx, 0)]


def _interp(tab, idx, w, dt, absolute=False):
    """sum_t w[:, t] tab[idx[:, t]] in tap order (weights are 0 outside)"""
    acc = 0
    for t in range(idx.shape[1]):
        v = _gather(tab, idx[:, t]).astype(dt, copy=False)
        acc = acc + w[:, t, None].astype(dt, copy=False) * (np.abs(v) if absolute else v)
    return acc


def forward(fp, T, dt=F64, absolute=False, value_only=False, app=True):
    """dt F64: the reference (absolute: the sums of |terms| of sigma_feat, grad, app, coef instead); dt F32: the restatement"""
    M, out = fp.M, {}
    inv = INV.astype(dt, copy=False)
    PW, LW = (np.abs(fp.PW), np.abs(fp.LW)) if absolute else (fp.PW, fp.LW)
    ab = np.abs if absolute else (lambda v: v)
    if T.dpk is not None:
        sf, g = np.zeros(M, dt), np.zeros((M, 3), dt)
        for i in range(3):
            nl = CD if value_only else DL
            if dt is F64:
                Lf = _interp(T.dlk[i][:, :nl], fp.LI[i], LW[i], F64, absolute)
                Lc = Lf[:, :CD]
                s = np.zeros((4, M))
                for t in range(4):
                    run = ab(_gather(T.dpk[i], fp.PI[i][:, t]).astype(F64))
                    w = PW[i][:, t].astype(F64)
                    s[0] += w * (run[:, :CD] * Lc).sum(1)
                    if not value_only:
                        s[1] += w * (run[:, CD:2 * CD] * Lc).sum(1)
                        s[2] += w * (run[:, 2 * CD:] * Lc).sum(1)
                        s[3] += w * (run[:, :CD] * Lf[:, CD:]).sum(1)
            else:                                          # the kernel's fmaf chains: taps in order, channels in order
                Lf = np.zeros((M, nl), F32)
                for t in range(2):
                    run = _gather(T.dlk[i][:, :nl], fp.LI[i][:, t])
                    Lf = _fma(np.broadcast_to(LW[i][:, t, None], run.shape), run, Lf)
                s = np.zeros((4, M), F32)
                for t in range(4):
                    run = _gather(T.dpk[i], fp.PI[i][:, t])
                    a = np.zeros((4, M), F32)
                    for c in range(CD):
                        a[0] = _fma(run[:, c], Lf[:, c], a[0])
                        if not value_only:
                            a[3] = _fma(run[:, c], Lf[:, CD + c], a[3])
                            a[1] = _fma(run[:, CD + c], Lf[:, c], a[1])
                            a[2] = _fma(run[:, 2 * CD + c], Lf[:, c], a[2])
                    for q in range(4):
                        s[q] = _fma(PW[i][:, t], a[q], s[q])
            sf = sf + s[0]
            g[:, MAT0[i]] += s[1]
            g[:, MAT1[i]] += s[2]
            g[:, VEC[i]] += s[3]
        out["sigma_feat"] = sf
        if not absolute:
            xx = np.minimum(np.maximum(sf, dt(-15.0)), dt(1e3)) + dt(SHIFT)
            with np.errstate(over="ignore"):
                out["sigma"] = np.where(xx > 20, xx, np.log1p(np.exp(np.minimum(xx, dt(30.0)))))
        if not value_only:
            g = g * inv
            out["grad"] = g
            if not absolute:
                n2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
                out["normal"] = -g * (dt(1.0) / np.sqrt(np.maximum(n2, dt(EPS))))[:, None]
    if app and getattr(T, "apl", None) is not None:
        coef = []
        for i in range(3):
            La = _interp(T.ali[i], fp.LI[i], LW[i], dt, absolute)
            Pa = _interp(T.apl[i], fp.PI[i], PW[i], dt, absolute)
            coef.append(Pa * La)
        out["coef"] = np.concatenate(coef, axis=1)
        B = ab(T.basis.astype(dt, copy=False))
        ap = np.zeros((M, AD), dt)
        for i in range(3):
            if dt is F64:
                ap = ap + coef[i] @ B[:, i * CA:(i + 1) * CA].T
            else:
                a = np.zeros((M, AD), F32)
                for c in range(CA):
                    a = a + coef[i][:, c, None] * B[None, :, i * CA + c]
                ap = ap + a
        out["app"] = ap
    return out


FWD_REL = ("sigma_feat", "grad", "app", "coef")          # |err| / sum of |terms|
FWD_ABS = ("sigma", "normal")                            # absolute error


def fwd_errors(got, ref, S):
    """metric -> largest error; an output whose sum of |terms| is 0 (every tap outside) must be exactly 0"""
    out = {}
    for m in got:
        g, r = np.asarray(got[m], F64).reshape(ref[m].shape), ref[m]
        if m in FWD_REL:
            live = S[m] > 0
            assert not g[~live].any(), f"{m}: a value where every tap is outside the grid"
            out[m] = _big((g - r)[live] / S[m][live])
        else:
            out[m] = _big(g - r)
    return out


def fwd_margins(own, ref):
    """relative metrics and the unit normal: scale 1; sigma: its largest value"""
    return {m: max(8 * own[m], FLOOR * (_big(ref[m]) if m == "sigma" else 1.0)) for m in own}


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def sample_adjoints(sf, grad, adj, dt, absolute=False):
    """sample_adjoint_finish: (dsf [M], dg [M,3]) in raw (texel) units.  absolute: the sums of |terms|"""
    M = len(adj.x)
    ab = np.abs if absolute else (lambda v: v)
    dsf = np.zeros(M, dt)
    if adj.d_sigma_feat is not None:
        dsf = dsf + ab(adj.d_sigma_feat.astype(dt, copy=False))
    if adj.d_sigma is not None:
        f = np.asarray(sf).astype(dt, copy=False)
        xx = np.minimum(np.maximum(f, dt(-15.0)), dt(1e3)) + dt(SHIFT)
        with np.errstate(over="ignore"):
            ds = np.where(xx > 20, dt(1.0), dt(1.0) / (dt(1.0) + np.exp(-xx)))
        ds = np.where((f < -15) | (f > 1e3), dt(0.0), ds)
        dsf = dsf + ab(adj.d_sigma.astype(dt, copy=False)) * ds
    dg = np.zeros((M, 3), dt)
    if adj.d_normal is not None:
        g, dn = np.asarray(grad).astype(dt, copy=False), adj.d_normal.astype(dt, copy=False)
        n2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        inv = dt(1.0) / np.sqrt(np.maximum(n2, dt(EPS)))
        if absolute:
            dot = (np.abs(dn) * np.abs(g)).sum(1)
            kk = np.where(n2 > dt(EPS), dot * inv * inv * inv, dt(0.0))
            dg = (np.abs(dn) * inv[:, None] + kk[:, None] * np.abs(g)) * INV.astype(dt, copy=False)
        else:
            dot = (dn[:, 0] * g[:, 0] + dn[:, 1] * g[:, 1]) + dn[:, 2] * g[:, 2]
            kk = np.where(n2 > dt(EPS), dot * inv * inv * inv, dt(0.0))
            dg = (-dn * inv[:, None] + kk[:, None] * g) * INV.astype(dt, copy=False)
    return dsf.astype(dt, copy=False), dg.astype(dt, copy=False)


def density_terms(fp, T, A, dt, absolute=False, with_normal=True):
    """per plane i: (PI, PW, B [M,48 or 16]) for g_dpk[i] and (LI, LW, B [M,32 or 16]) for g_dlk[i]: entry += weight x B"""
    dsf, dg = A
    PW, LW = (np.abs(fp.PW), np.abs(fp.LW)) if absolute else (fp.PW, fp.LW)
    planes, lines = [], []
    for i in range(3):
        nl, npl = (DL, DP) if with_normal else (CD, CD)
        Lf = _interp(T.dlk[i][:, :nl], fp.LI[i], LW[i], dt, absolute)
        Pf = _interp(T.dpk[i][:, :npl], fp.PI[i], PW[i], dt, absolute)
        Lc, Pq = Lf[:, :CD], Pf[:, :CD]
        d = dsf[:, None]
        if with_normal:
            da, db, dw = dg[:, MAT0[i], None], dg[:, MAT1[i], None], dg[:, VEC[i], None]
            bP = d * Lc + dw * Lf[:, CD:]
            bL = (d * Pq + da * Pf[:, CD:2 * CD]) + db * Pf[:, 2 * CD:]
            planes.append((fp.PI[i], PW[i].astype(dt, copy=False), np.concatenate([bP, da * Lc, db * Lc], axis=1)))
            lines.append((fp.LI[i], LW[i].astype(dt, copy=False), np.concatenate([bL, dw * Pq], axis=1)))
        else:
            planes.append((fp.PI[i], PW[i].astype(dt, copy=False), d * Lc))
            lines.append((fp.LI[i], LW[i].astype(dt, copy=False), d * Pq))
    return planes, lines


def dcoef_of(d_app, basis, dt, absolute=False):
    """k_dcoef: d_app x basis_mat, the 24 terms in order"""
    da, B = d_app.astype(dt, copy=False), basis.astype(dt, copy=False)
    if absolute:
        da, B = np.abs(da), np.abs(B)
    if dt is F64:
        return da @ B
    v = np.zeros((len(da), 3 * CA), F32)
    for q in range(AD):
        v = v + B[None, q] * da[:, q, None]
    return v


def app_terms(fp, T, d_app, dt, absolute=False):
    PW, LW = (np.abs(fp.PW), np.abs(fp.LW)) if absolute else (fp.PW, fp.LW)
    dc = dcoef_of(d_app, T.basis, dt, absolute)
    planes, lines, coef = [], [], []
    for i in range(3):
        La = _interp(T.ali[i], fp.LI[i], LW[i], dt, absolute)
        Pa = _interp(T.apl[i], fp.PI[i], PW[i], dt, absolute)
        planes.append((fp.PI[i], PW[i].astype(dt, copy=False), dc[:, i * CA:(i + 1) * CA] * La))
        lines.append((fp.LI[i], LW[i].astype(dt, copy=False), dc[:, i * CA:(i + 1) * CA] * Pa))
        coef.append(Pa * La)
    return planes, lines, np.concatenate(coef, axis=1)


def slots_of(idx):
    """-> (tex: the sorted texels any tap names, slot [M,T]: position of each tap in tex, -1 outside)"""
    ok = idx >= 0
    tex, inv = np.unique(idx[ok], return_inverse=True)
    slot = np.full(idx.shape, -1, np.int64)
    slot[ok] = inv.reshape(-1)
    return tex, slot


def accumulate(slot, nU, w, B, dt, order=None, init=None):
    """acc[slot[m, t], c] += w[m, t] B[m, c], one addition after the other in sample order (index_add_ on the CPU walks its index
    front to back), in float64 or float32; taps outside the grid (weight 0) go to a spare row"""
    if order is not None:
        slot, w, B = slot[order], w[order], B[order]
    C = B.shape[1]
    tw, tB = (torch.from_numpy(np.ascontiguousarray(a, dtype=dt)) for a in (w, B))
    acc = torch.zeros((nU + 1, C), dtype=tw.dtype)
    if init is not None:
        acc[:nU] += torch.from_numpy(np.ascontiguousarray(init, dtype=dt).reshape(nU, C))
    acc.index_add_(0, torch.from_numpy(np.where(slot >= 0, slot, nU).reshape(-1)), (tw[:, :, None] * tB[:, None, :]).reshape(-1, C))
    return acc[:nU].numpy()


def sum_rows(rows, dt, order=None):
    """sum over samples of rows [M, ...]: float32 one after the other"""
    if dt is F64:
        return rows.sum(0)
    acc = np.zeros((1,) + rows.shape[1:], F32)
    for s in range(0, len(rows), 4096):
        sel = slice(s, s + 4096) if order is None else order[s:s + 4096]
        acc = np.cumsum(np.concatenate([acc, rows[sel]]), axis=0, dtype=F32)[-1:]
    return acc[0]


def sample_orders(fp):
    return (None, np.argsort(fp.brick, kind="stable"), np.arange(fp.M)[::-1].copy())


def _scatter_case(terms_ref, terms_abs, terms_f32, orders, init=None):
    """one table: -> SimpleNamespace(tex, ref [U,C], S [U,C], own: the restatement's worst |err| / S over the sample orders)"""
    idx = terms_ref[0]
    tex, slot = slots_of(idx)
    nU = len(tex)
    i64 = None if init is None else init[tex].astype(F64)
    ref = accumulate(slot, nU, terms_ref[1], terms_ref[2], F64, init=i64)
    S = accumulate(slot, nU, terms_abs[1], terms_abs[2], F64, init=None if init is None else np.abs(i64))
    own = 0.0
    live = S > 0
    for o in orders:
        r = accumulate(slot, nU, terms_f32[1], terms_f32[2], F32, order=o, init=None if init is None else init[tex])
        assert not r[~live].any()
        own = max(own, _big((r.astype(F64) - ref)[live] / S[live]))
    return SimpleNamespace(tex=tex, ref=ref, S=S, own=own)


def adjoints(x, sf=None, grad=None, d_sigma=None, d_sigma_feat=None, d_normal=None, d_app=None):
    return SimpleNamespace(x=x, sf=sf, grad=grad, d_sigma=d_sigma, d_sigma_feat=d_sigma_feat, d_normal=d_normal, d_app=d_app)


def backward_density(fp, T, adj, init=None, fp_kernel=None):
    """-> {"g_dpk": [3 cases], "g_dlk": [3 cases]}; with_normal follows adj.d_normal.  init = (g_dpk, g_dlk) values already in the tables.
    fp_kernel: other footprints for the 'got' side of a broken variant (see variants())"""
    wn = adj.d_normal is not None
    A64 = sample_adjoints(adj.sf, adj.grad, adj, F64)
    Aab = sample_adjoints(adj.sf, adj.grad, adj, F64, absolute=True)
    A32 = sample_adjoints(adj.sf, adj.grad, adj, F32)
    t64 = density_terms(fp, T, A64, F64, with_normal=wn)
    tab = density_terms(fp, T, Aab, F64, absolute=True, with_normal=wn)
    t32 = density_terms(fp, T, A32, F32, with_normal=wn)
    orders = sample_orders(fp)
    out = {}
    for k, name in enumerate(("g_dpk", "g_dlk")):
        out[name] = [_scatter_case(t64[k][i], tab[k][i], t32[k][i], orders, None if init is None else init[k][i]) for i in range(3)]
    return out


def backward_app(fp, T, d_app, init=None):
    """-> {"g_apl": [3], "g_ali": [3], "g_basis": SimpleNamespace(ref, S, own)}"""
    t64, tab, t32 = app_terms(fp, T, d_app, F64), app_terms(fp, T, d_app, F64, absolute=True), app_terms(fp, T, d_app, F32)
    orders = sample_orders(fp)
    out = {}
    for k, name in enumerate(("g_apl", "g_ali")):
        out[name] = [_scatter_case(t64[k][i], tab[k][i], t32[k][i], orders, None if init is None else init[k][i]) for i in range(3)]
    ref = d_app.astype(F64).T @ t64[2]
    S = np.abs(d_app).astype(F64).T @ tab[2]
    rows32 = d_app[:, :, None] * t32[2][:, None, :]
    live = S > 0
    own = max(_big((sum_rows(rows32, F32, o).astype(F64) - ref)[live] / S[live]) for o in orders) if live.any() else 0.0
    out["g_basis"] = SimpleNamespace(ref=ref, S=S, own=own)
    return out


def table_error(got, case, init=None):
    """got [n, C] (or [n, C'] with C' > the channels of the case: the rest must be zero): the largest |got - ref| / S over the entries
    something is added to; every other entry must be EXACTLY what it was (0.0 without init)"""
    got = np.asarray(got, F64)
    C = case.ref.shape[1]
    rest = np.ones(len(got), bool)
    rest[case.tex] = False
    base = np.zeros_like(got) if init is None else np.asarray(init, F64).reshape(got.shape)
    assert np.array_equal(got[rest], base[rest]), "an entry that no sample touches was written"
    assert np.array_equal(got[:, C:], base[:, C:]), "a channel block that this walk does not have was written"
    g = got[case.tex][:, :C]
    live = case.S > 0
    assert np.array_equal(g[~live], base[case.tex][:, :C][~live]), "an entry whose every contribution is zero was changed"
    return _big((g - case.ref)[live] / case.S[live]) if live.any() else 0.0


def margin_of(cases, own=None):
    """(the restatement's error, the margin) of one table kind: the three planes / lines of a walk share them"""
    own = max(c.own for c in cases) if own is None else own
    return own, max(8 * own, FLOOR)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def world_of(ix, G):
    """fp32 positions whose texel coordinates are near ix [M,3] (float64)"""
    xn = ix / (G - 1) * 2.0 - 1.0
    return ((xn + 1.0) / INV.astype(F64) + AABB[0].astype(F64)).astype(F32)


def _axis_coord(x_axis, a, G):
    x = np.zeros((len(x_axis), 3), F32)
    x[:, a] = x_axis
    return texel_coord(normalized(x), G)[:, a]


def _hit(target, a, G):
    """an fp32 coordinate on axis a whose restated texel coordinate is exactly `target`, or None"""
    x0 = world_of(np.full((1, 3), float(target)), G)[0, a]
    c = np.array([x0], F32)
    lo, hi = c.copy(), c.copy()
    for _ in range(256):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        c = np.concatenate([lo, c, hi])
    ix = _axis_coord(c, a, G)
    ok = np.nonzero(ix == F32(target))[0]
    return None if len(ok) == 0 else c[ok[len(ok) // 2]]


def _step(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf if n > 0 else -np.inf))
    return x


@functools.lru_cache(maxsize=None)
def axis_candidates(G, a):
    """fp32 coordinates on axis a for every edge class (classified afterwards by the restated texel coordinate)"""
    nbx = (G + BR - 1) // BR
    out = []
    mult = sorted({4 * b for b in (1, 2, nbx - 2, nbx - 1) if 0 < 4 * b <= G - 1})
    for t in [0, G - 1, 1, G // 2, G - 2, G - 3, G - 6, G - 7] + mult:
        h = _hit(t, a, G)
        if h is None:              # not every integer is the rounded image of an fp32 position: the nearest one then
            h = world_of(np.full((1, 3), float(t)), G)[0, a]
        out += [h, _step(h, -6), _step(h, 6)]
    for t in (-0.5, -0.01, -1.0, -1.5, -3.0, G - 0.5, float(G), G + 0.6, G + 2.5, 0.37, G - 1.4):
        out.append(world_of(np.full((1, 3), t), G)[0, a])
    return np.array(out, F32)


def classify(ix, G):
    """edge class -> bool [M,3], from the restated texel coordinate alone"""
    f = np.floor(ix)
    integer = (ix == f) & (ix >= 0) & (ix <= G - 1)
    nbx = (G + BR - 1) // BR
    mult = np.array(sorted({4.0 * b for b in (1, 2, nbx - 2, nbx - 1) if 0 < 4 * b <= G - 1}))
    near = lambda d: np.isin(f + d, mult)       # noqa: E731
    return {"integer": integer, "zero": ix == 0, "last": ix == G - 1, "below0": (ix > -1) & (ix < 0), "out_low": ix <= -1,
            "out_high": ix >= G, "brick_on": integer & np.isin(ix, mult), "brick_below": (ix != f) & near(1) & (ix - f > 0.5),
            "brick_above": (ix != f) & near(0) & (ix - f < 0.5)}


@functools.lru_cache(maxsize=None)
def batch(G, kind):
    """kind "edge": every candidate on each axis with the other axes random, on two and on three axes at once, and all triples of a
    short list; "ladder": one named brick per population of LADDER, the rest filled sparsely (G = 104: every brick holds a sample);
    "big": 400 001 random samples (item size 256); "special" (tables(G, "special")): sigma_feat beyond 1e3 and the all-zero corner"""
    rng = np.random.default_rng([7, G, sum(map(ord, kind))])
    inside = lambda n: world_of(rng.uniform(0.05, G - 1.05, (n, 3)), G)       # noqa: E731
    if kind == "edge":
        cand = [axis_candidates(G, a) for a in range(3)]
        n = min(len(c) for c in cand)
        rows = []
        for a in range(3):
            for rep in range(2):
                x = inside(n)
                x[:, a] = cand[a][:n]
                rows.append(x)
            x = inside(n)
            x[:, a], x[:, (a + 1) % 3] = cand[a][:n], cand[(a + 1) % 3][:n]
            rows.append(x)
        rows.append(np.stack([cand[a][:n] for a in range(3)], axis=1))
        short = [0, 3, 6, 9, n - 11, n - 8, n - 6, n - 5]   # (positions in axis_candidates)              # ix = 0 and G - 1 with a neighbour, in (-1,0), <= -1, >= G
        tri = np.array([(i, j, k) for i in short for j in short for k in short])
        rows.append(np.stack([cand[a][tri[:, a]] for a in range(3)], axis=1))
        x = np.concatenate(rows)
    elif kind == "ladder":
        nbx = (G + BR - 1) // BR
        named = ladder_bricks(G)
        rows = []
        for (bx, by, bz), n in zip(named, LADDER):
            lo = np.array([bx, by, bz]) * BR
            hi = np.minimum(lo + BR, G) - 1e-3
            while True:
                x = world_of(rng.uniform(lo + 1e-3, hi, (2 * n + 8, 3)), G)
                x = x[brick_of(normalized(x), G) == (bz * nbx + by) * nbx + bx][:n]
                if len(x) == n:
                    break
            rows.append(x)
        if G == 104:
            c = np.stack(np.meshgrid(*[np.arange(nbx)] * 3, indexing="ij"), -1).reshape(-1, 3) * BR
            fill = world_of(c + rng.uniform(0.2, 3.8, c.shape), G)
        else:
            fill = world_of(rng.uniform(-0.7, G - 0.3, (1500, 3)), G)
        ids = {(bz * nbx + by) * nbx + bx for bx, by, bz in named}
        fill = fill[~np.isin(brick_of(normalized(fill), G), list(ids))]
        x = np.concatenate(rows + [fill])
        x = x[rng.permutation(len(x))]
    elif kind == "big":
        x = world_of(rng.uniform(-0.4, G - 0.6, (400001, 3)), G)
    elif kind == "special":
        x = np.concatenate([world_of(rng.uniform(0.2, 2.8, (12, 3)) + np.array([0, 0, G - 4.0]), G),      # plane 0 patch x the top of the ramp
                            world_of(rng.uniform(0.2, 2.8, (8, 3)) + np.array([0, 0, 0.5 * (G - 1) + 1.0]), G),      # the same patch lower on the ramp: x > 20
                            world_of(rng.uniform(0.2, 2.8, (8, 3)), G),                                   # ... and at its negative end: below -15
                            world_of(rng.uniform(G - 5.5, G - 1.2, (12, 3)), G),                          # the all-zero corner
                            inside(40)])
    else:
        raise KeyError(kind)
    x = np.concatenate([x, rng.uniform(0, 1, (len(x), 1)).astype(F32)], axis=1)
    x.setflags(write=False)
    return x


def ladder_bricks(G):
    """14 bricks (bx, by, bz) for the populations of LADDER: the first and the last brick of the grid and others spread between"""
    nbx = (G + BR - 1) // BR
    rng = np.random.default_rng([9, G])
    seen, out = set(), [(0, 0, 0), (nbx - 1, nbx - 1, nbx - 1), (nbx - 1, 0, nbx - 2), (0, nbx - 1, 1)]
    seen.update(out)
    while len(out) < len(LADDER):
        b = tuple(int(v) for v in rng.integers(0, nbx, 3))
        if b not in seen:
            seen.add(b)
            out.append(b)
    order = rng.permutation(len(LADDER))
    return [out[k] for k in order]


@functools.lru_cache(maxsize=None)
def prints(G, kind):
    return footprints(batch(G, kind), G)


def table_kind(kind):
    return "special" if kind == "special" else "std"


@functools.lru_cache(maxsize=None)
def fwd_case(G, kind, bf16=False, source="packed"):
    """-> (ref, S, own, margins) of the forward on batch(G, kind); source "raw": value only from the density factors themselves"""
    fp, tb = prints(G, kind), tables(G, table_kind(kind))
    if source == "raw":
        T = SimpleNamespace(dpk=(tb.raw16 if bf16 else tb.raw).dpk, dlk=(tb.raw16 if bf16 else tb.raw).dlk, apl=None)
    else:
        T = tb.bf16 if bf16 else tb.fp32
    vo = source == "raw"
    ref = forward(fp, T, value_only=vo)
    S = forward(fp, T, absolute=True, value_only=vo)
    own = fwd_errors(forward(fp, T, F32, value_only=vo), ref, S)
    return ref, S, own, fwd_margins(own, ref)


@functools.lru_cache(maxsize=None)
def saved(G, kind):
    """sigma_feat and grad as the backward gets them: the restatement's outputs (given arrays, independent of the forward kernel)"""
    fp, tb = prints(G, kind), tables(G, table_kind(kind))
    out = forward(fp, tb.fp32, F32, app=False, value_only=(kind == "big"))
    return out["sigma_feat"], out.get("grad")


@functools.lru_cache(maxsize=None)
def adjoint_set(G, kind, hot=None):
    """random adjoints with exact zeros; hot = a sample index: that sample alone has adjoints (every other row is exactly zero)"""
    M = len(batch(G, kind))
    rng = np.random.default_rng([13, G, sum(map(ord, kind))])
    r = lambda *s: rng.standard_normal(s).astype(F32)      # noqa: E731
    d = dict(d_sigma=r(M), d_sigma_feat=r(M), d_normal=r(M, 3), d_app=r(M, AD))
    zero = rng.uniform(size=M) < 0.1
    for v in d.values():
        v[zero] = 0
        if hot is not None:
            keep = v[hot].copy()
            v[:] = 0
            v[hot] = keep if np.any(keep) else 1
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def bwd_case(G, kind, mode, hot=None):
    """mode "full": d_sigma, d_sigma_feat, d_normal (the <true> walks); "value": d_sigma and d_sigma_feat; "feat": d_sigma_feat alone;
    "app": the appearance tables and g_basis.  -> the dict of backward_density / backward_app"""
    fp, tb = prints(G, kind), tables(G, table_kind(kind))
    d = adjoint_set(G, kind, hot)
    x = batch(G, kind)
    if hot is not None:                                   # a row with zero adjoints adds nothing: the reference of one sample
        fp = footprints(x[hot:hot + 1], G)
        d = {k: v[hot:hot + 1] for k, v in d.items()}
        sf, gr = (v[hot:hot + 1] for v in saved(G, kind))
        x = x[hot:hot + 1]
    else:
        sf, gr = saved(G, kind)
    if mode == "app":
        return backward_app(fp, tb.fp32, d["d_app"])
    adj = adjoints(x, sf, gr, d_sigma=None if mode == "feat" else d["d_sigma"], d_sigma_feat=d["d_sigma_feat"],
                   d_normal=d["d_normal"] if mode == "full" else None)
    return backward_density(fp, tb.fp32, adj)


def one_hot_samples(G):
    """for every edge class and axis the first sample of the edge batch in it, other axes inside where there is one"""
    fp = prints(G, "edge")
    cl = classify(fp.ix, G)
    inside = (fp.ix > 0) & (fp.ix < G - 1)
    out = {}
    for name in EDGE_CLASSES:
        for a in range(3):
            others = inside[:, (a + 1) % 3] & inside[:, (a + 2) % 3]
            hit = np.nonzero(cl[name][:, a] & others)[0]
            if len(hit) == 0:
                hit = np.nonzero(cl[name][:, a])[0]
            if len(hit):
                out[(name, a)] = int(hit[0])
    return out


# ---- broken variants ----------------------------------------------------------------------------------------------------------------
def _variant_error(fp_ref, fp_got, T, adj, keep=None):
    """-> (worst |got - ref| / S over the entries of all density tables that something is added to, over the margin; whether an entry
    that nothing is added to was written), got = the float64 sums of a broken walk"""
    wn = adj.d_normal is not None
    case = backward_density(fp_ref, T, adj)
    A64 = sample_adjoints(adj.sf, adj.grad, adj, F64)
    if keep is not None:
        A64 = (A64[0] * keep, A64[1] * keep[:, None])
    got = density_terms(fp_got, T, A64, F64, with_normal=wn)
    n = (fp_ref.G * fp_ref.G, fp_ref.G)
    worst, stray = 0.0, False
    for k, name in enumerate(("g_dpk", "g_dlk")):
        _, mg = margin_of(case[name])
        for i in range(3):
            idx, w, B = got[k][i]
            dense = np.bincount(((np.maximum(idx, 0) * B.shape[1])[:, :, None] + np.arange(B.shape[1])).reshape(-1),
                                weights=((idx >= 0)[:, :, None] * w[:, :, None] * B[:, None, :]).reshape(-1),
                                minlength=n[k] * B.shape[1]).reshape(n[k], B.shape[1])
            c = case[name][i]
            full = np.zeros_like(dense)
            full[c.tex] = c.ref
            err = np.abs(dense - full)
            Sfull = np.zeros_like(dense)
            Sfull[c.tex] = c.S
            worst = max(worst, float((err / np.where(Sfull > 0, Sfull, 1))[Sfull > 0].max()) / mg)
            stray = stray or bool(err[Sfull == 0].any())
    return worst, stray


def _copy_fp(fp):
    return SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(fp).items()})


def variants(G):
    """name -> (the factor by which the broken walk misses the margin, whether it also writes an entry that must stay zero)"""
    tb = tables(G)
    out = {}
    for kind in ("edge", "ladder"):
        fp, x = prints(G, kind), batch(G, kind)
        sf, gr = saved(G, kind)
        d = adjoint_set(G, kind)
        adj = adjoints(x, sf, gr, d["d_sigma"], d["d_sigma_feat"], d["d_normal"])
        if kind == "edge":
            # (a) the halo column of the tile dropped: the east taps that land on tile column 4
            a = _copy_fp(fp)
            for i in range(3):
                xa = fp.x0[:, MAT0[i]]
                halo = (xa + 1) - BR * (np.clip(xa, 0, G - 1) // BR) == BR
                a.PW[i][halo, 1] = 0
                a.PW[i][halo, 3] = 0
            out["halo column dropped"] = _variant_error(fp, a, tb.fp32, adj)
            # (c) tile cell c00 one row off at x0 = -1
            c = _copy_fp(fp)
            for i in range(3):
                row = fp.x0[:, MAT0[i]] == -1
                moved = np.where(c.PI[i] >= 0, c.PI[i] + G, -1)
                moved[moved >= G * G] = -1
                c.PI[i][row] = moved[row]
                c.PW[i][row] = np.where(c.PI[i][row] >= 0, c.PW[i][row], 0)
            out["c00 one row off at x0 = -1"] = _variant_error(fp, c, tb.fp32, adj)
            # (d) the fraction from the unrounded product
            out["weights from the fused product"] = _variant_error(fp, footprints(x, G, "fused"), tb.fp32, adj)
        else:
            # (b) the last (e - s) mod 4 samples of every work item skipped
            order = np.argsort(fp.brick, kind="stable")
            b = fp.brick[order]
            start = np.r_[0, np.nonzero(np.diff(b))[0] + 1]
            cnt = np.diff(np.r_[start, len(b)])
            r = np.arange(len(b)) - np.repeat(start, cnt)
            length = np.minimum(ITEM, np.repeat(cnt, cnt) - (r // ITEM) * ITEM)
            keep = np.ones(len(b))
            keep[order[(r % ITEM) >= length - length % 4]] = 0
            assert (keep == 0).any()
            out["item tail skipped"] = _variant_error(fp, fp, tb.fp32, adj, keep=keep)
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GRIDS)
def test_inputs_hold_every_edge_class_and_ladder_population(G):
    fp = prints(G, "edge")
    cl = classify(fp.ix, G)
    for name in EDGE_CLASSES:
        for a in range(3):
            assert cl[name][:, a].any(), (G, name, a)
    assert (cl["out_low"].any(1) | cl["out_high"].any(1)).sum() > 20
    assert (cl["integer"].sum(1) == 3).any() and (cl["zero"].sum(1) == 3).any() and (cl["last"].sum(1) == 3).any()
    assert len(one_hot_samples(G)) == 3 * len(EDGE_CLASSES)
    lad = prints(G, "ladder")
    nbx = (G + BR - 1) // BR
    counts = np.bincount(lad.brick, minlength=nbx ** 3)
    for (bx, by, bz), n in zip(ladder_bricks(G), LADDER):
        assert counts[(bz * nbx + by) * nbx + bx] == n, (G, n)
    items = int(((counts + ITEM - 1) // ITEM).sum())
    if G == 104:
        assert counts.min() >= 1 and items > 16384          # the persistent loop of the walk has to stride
    if G == 129:
        assert nbx ** 3 > 32768                             # one counter copy per brick, several scan chunks
    assert len(batch(16, "big")) == 400001                  # above 400 000: work items of 256 samples


@pytest.mark.parametrize("G", GRIDS)
def test_gradient_of_every_random_sample_is_clear_of_zero(G):
    for kind in ("edge", "ladder"):
        ref, S = fwd_case(G, kind)[:2]
        fp = prints(G, kind)
        gn, sn = np.linalg.norm(ref["grad"], axis=1), np.linalg.norm(S["grad"], axis=1)
        live = sn > 0
        print(f"G {G} {kind}: smallest |g| / |sum of |terms|| = {(gn[live] / sn[live]).min():.3e}")
        assert (gn[live] / sn[live]).min() > GRAD_FLOOR, (G, kind)
        assert all(np.isfinite(v).all() for v in ref.values())
        outd = ((fp.ix <= -1) | (fp.ix >= G)).all(1)
        assert (outd.any() or kind != "edge") and not ref["sigma_feat"][outd].any() and not ref["app"][outd].any()


def test_special_samples_reach_the_remaining_branches():
    ref = fwd_case(17, "special")[0]
    sf = ref["sigma_feat"]
    assert (sf > 1e3).any() and ((sf + SHIFT > 20) & (sf <= 1e3)).any() and (sf < -15).any()
    g2 = (ref["grad"] ** 2).sum(1)
    assert (g2 == 0).sum() >= 4 and (g2 > 1e-4).any()
    std = fwd_case(129, "ladder")[0]["sigma_feat"]           # the ramps of the standard tables reach every branch on the large grids
    assert (std < -15).any() and (std + SHIFT > 20).any() and ((std > -15) & (std + SHIFT < 20)).any()


@pytest.mark.parametrize("G", (17, 19, 57))
def test_restatement_and_fp32_oracle_stay_inside_half_of_every_margin(G):
    for kind in ("edge", "ladder"):
        for bf in (False, True):
            ref, S, own, mg = fwd_case(G, kind, bf)
            for m in own:
                print(f"G {G} {kind} bf16={bf} forward {m}: restatement {own[m]:.3e}, margin {mg[m]:.3e}")
                assert own[m] <= 0.5 * mg[m]
        for mode in ("full", "value", "app"):
            for name, cases in bwd_case(G, kind, mode).items():
                own, mg = margin_of(cases if isinstance(cases, list) else [cases])
                print(f"G {G} {kind} backward {mode} {name}: restatement {own:.3e}, margin {mg:.3e}")
                assert own <= 0.5 * mg
    # the fp32 torch oracle (its own coordinate arithmetic and sum order) on the samples of the ladder batch that sit clear of a texel
    x, tb = batch(G, "ladder"), tables(G)
    ref, S, own, mg = fwd_case(G, "ladder")
    sd, cfg = _oracle_inputs(tb, torch.float32, G)
    sf = O.density_feature(sd, cfg, torch.from_numpy(x.copy())).detach().numpy().astype(F64)
    ix = prints(G, "ladder").ix
    far = (np.abs(ix - np.round(ix)) > 1e-3).all(1) & (S["sigma_feat"] > 0)      # (its rounding of the coordinate may cross a texel)
    e = np.abs(sf - ref["sigma_feat"])[far] / S["sigma_feat"][far]
    print(f"G {G} fp32 oracle sigma_feat: {e.max():.3e} of the sum of |terms|, margin {mg['sigma_feat']:.3e}")
    assert e.max() <= 0.5 * mg["sigma_feat"]


def _oracle_inputs(tb, dtype, G):
    sd = {}
    for i in range(3):
        sd[f"rf.density_rf.app_plane.{i}"] = torch.tensor(tb.planes[i]).to(dtype).permute(2, 0, 1)[None].clone().requires_grad_(True)
        sd[f"rf.density_rf.app_line.{i}"] = torch.tensor(tb.lines[i]).to(dtype).t()[None, :, :, None].clone().requires_grad_(True)
        sd[f"rf.app_rf.app_plane.{i}"] = torch.tensor(tb.fp32.apl[i]).to(dtype).reshape(G, G, CA).permute(2, 0, 1)[None].clone().requires_grad_(True)
        sd[f"rf.app_rf.app_line.{i}"] = torch.tensor(tb.fp32.ali[i]).to(dtype).t()[None, :, :, None].clone().requires_grad_(True)
    sd["rf.basis_mat.weight"] = torch.tensor(tb.fp32.basis).to(dtype).requires_grad_(True)
    return sd, O.Cfg(aabb=torch.tensor(AABB), grid=G, density_shift=float(SHIFT))


@pytest.mark.parametrize("G", (17, 19))
def test_reference_agrees_with_the_float64_oracle(G, monkeypatch):
    """the numpy reference with FLOAT64 weights and float64 tables (pack included) against oracle/nmf_oracle.py and autograd in float64"""
    tb = tables(G)
    rng = np.random.default_rng([3, G])
    x = np.concatenate([world_of(rng.uniform(-0.6, G - 0.4, (600, 3)), G), np.zeros((600, 1), F32)], axis=1)
    k = torch.tensor(stencil().astype(F64))[None, None]
    monkeypatch.setattr(O, "derivative_stencils", lambda: (k, k.transpose(2, 3)))
    sd, cfg = _oracle_inputs(tb, torch.float64, G)
    xt = torch.tensor(x.astype(F64))
    o_sf, o_sg = O.density_feature(sd, cfg, xt), O.density(sd, cfg, xt)
    o_g, o_n, o_app = O.density_gradient(sd, cfg, xt), O.normals(sd, cfg, xt), O.app_feature(sd, cfg, xt)
    fp = footprints(x, G, "f64")
    d64, l64 = pack_tables(tb.planes, tb.lines)
    T = SimpleNamespace(dpk=d64, dlk=l64, apl=tb.fp32.apl, ali=tb.fp32.ali, basis=tb.fp32.basis)
    ref = forward(fp, T)
    rel = lambda a, b: _big(a - b.detach().numpy()) / _big(b.detach().numpy())      # noqa: E731
    agree = {"sigma_feat": rel(ref["sigma_feat"], o_sf), "sigma": rel(ref["sigma"], o_sg), "grad": rel(ref["grad"], o_g),
             "normal": rel(ref["normal"], o_n), "app": rel(ref["app"], o_app)}
    r = lambda *s: rng.standard_normal(s)      # noqa: E731
    ca, cd, cc, cb = r(600), r(600), r(600, 3), r(600, AD)
    loss = (o_sg * torch.tensor(ca)).sum() + (o_sf * torch.tensor(cd)).sum() + (o_n * torch.tensor(cc)).sum() + (o_app * torch.tensor(cb)).sum()
    names = list(sd)
    auto = dict(zip(names, torch.autograd.grad(loss, [sd[n] for n in names])))
    adj = adjoints(x, ref["sigma_feat"], ref["grad"], ca, cd, cc)
    A = sample_adjoints(adj.sf, adj.grad, adj, F64)
    planes, lines = density_terms(fp, T, A, F64)
    dense = lambda t, n: np.bincount(((np.maximum(t[0], 0) * t[2].shape[1])[:, :, None] + np.arange(t[2].shape[1])).reshape(-1),      # noqa: E731
                                     weights=((t[0] >= 0)[:, :, None] * t[1][:, :, None] * t[2][:, None, :]).reshape(-1),
                                     minlength=n * t[2].shape[1]).reshape(n, t[2].shape[1])
    gP, gL = unpack_grads([dense(t, G * G) for t in planes], [dense(t, G) for t in lines], G)
    ap, al, coef = app_terms(fp, T, cb, F64)
    for i in range(3):
        agree[f"d plane {i}"] = rel(gP[i], auto[f"rf.density_rf.app_plane.{i}"][0].permute(1, 2, 0))
        agree[f"d line {i}"] = rel(gL[i], auto[f"rf.density_rf.app_line.{i}"][0, :, :, 0].t())
        agree[f"d app plane {i}"] = rel(dense(ap[i], G * G).reshape(G, G, CA), auto[f"rf.app_rf.app_plane.{i}"][0].permute(1, 2, 0))
        agree[f"d app line {i}"] = rel(dense(al[i], G), auto[f"rf.app_rf.app_line.{i}"][0, :, :, 0].t())
    agree["d basis"] = rel(cb.T @ coef, auto["rf.basis_mat.weight"])
    for kk, v in agree.items():
        print(f"G {G} numpy reference vs float64 oracle, {kk}: {v:.2e} of the largest entry")
        assert v < 1e-11, kk


def test_pack_and_unpack_restatements():
    for G in (5, 6, 17, 19):
        rng = np.random.default_rng([17, G])
        planes = [rng.standard_normal((G, G, CD)).astype(F32) for _ in range(3)]
        lines = [rng.standard_normal((G, CD)).astype(F32) for _ in range(3)]
        own, mg = pack_margin(planes, lines)
        print(f"G {G} pack: restatement {own:.3e} of the sum of |terms|, margin {mg:.3e}")
        assert own <= 0.5 * mg


def pack_margin(planes, lines):
    ref, S, r32 = pack_tables(planes, lines), pack_tables(planes, lines, absolute=True), pack_tables(planes, lines, F32)
    own = max(_big((a.astype(F64) - b) / np.where(s > 0, s, 1)) for k in range(2) for a, b, s in zip(r32[k], ref[k], S[k]))
    return own, max(8 * own, FLOOR)


def unpack_case(g_dpk, g_dlk, G, x=None, l1=None):
    """-> (ref (gP, gL), S, own, margin)"""
    ref, S = unpack_grads(g_dpk, g_dlk, G, x=x, l1=l1), unpack_grads(g_dpk, g_dlk, G, absolute=True, x=x, l1=l1)
    r32 = unpack_grads(g_dpk, g_dlk, G, F32, x=x, l1=None if l1 is None else F32(l1))
    own = max(_big((a.astype(F64) - b)[s > 0] / s[s > 0]) if (s > 0).any() else 0.0 for k in range(2) for a, b, s in zip(r32[k], ref[k], S[k]))
    return ref, S, own, max(8 * own, FLOOR)


def test_broken_variants_miss_the_margins_by_a_wide_factor():
    v19, v17 = variants(19), variants(17)
    for k in v19:
        print(f"broken variant '{k}': misses the margin {v19[k][0]:.3g}-fold at G = 19 (stray entries: {v19[k][1]}), "
              f"{v17[k][0]:.3g}-fold at G = 17 (stray entries: {v17[k][1]})")
    for k in ("halo column dropped", "item tail skipped", "c00 one row off at x0 = -1"):
        assert v19[k][0] > 1e5 and v17[k][0] > 1e5, k
    assert v19["c00 one row off at x0 = -1"][1] and v17["c00 one row off at x0 = -1"][1]
    # the fused fraction: half an ulp of the texel coordinate in every weight at G = 19; the same bits where G - 1 is a power of two
    assert v19["weights from the fused product"][0] > 100
    a, b = footprints(batch(17, "edge"), 17), footprints(batch(17, "edge"), 17, "fused")
    assert np.array_equal(a.PW, b.PW) and np.array_equal(a.LW, b.LW) and v17["weights from the fused product"] == (0.0, False)
    a, b = footprints(batch(19, "edge"), 19), footprints(batch(19, "edge"), 19, "fused")
    assert not np.array_equal(a.PW, b.PW)


def test_big_case_margins():
    out = bwd_case(16, "big", "feat")
    for name, cases in out.items():
        own, mg = margin_of(cases)
        print(f"G 16 M 400001 value-only {name}: restatement {own:.3e}, margin {mg:.3e}")
        assert own <= 0.5 * mg
