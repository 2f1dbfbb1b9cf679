"""The VM field on the GPU (csrc/vm.hip through the wrappers of nmf_amd/hip.py) against the float64 references of tests/test_vm_cpu.py, on
its inputs, within its margins: nmf_vm_pack_density, nmf_vm_unpack_density_grad, the four forward kernels (k_vm_fwd, k_vm_sigma,
k_vm_rows_dn, k_vm_app_rows) with fp32 and bf16 tables, and all five launches of nmf_vm_query_bwd_segments.  The backward is checked
PER ENTRY of the packed gradient tables g_dpk / g_dlk, of the appearance tables and of g_basis: |got - ref64| over the float64 sum of
the absolute terms of that entry, and every entry that nothing is added to must be exactly 0.0 (or what it held before the walk).
Every test prints the kernel's error, its ratio to the fp32 restatement's and the margin (8 x the restatement's error, at least
2^-23), then holds every element to it.

What these tests found: fp_prologue, the footprint of both backward walks, was compiled with `ix - floor(ix)` fused into one fma, so
wherever G - 1 is not a power of two the walks scattered with weights half an ulp of ix away from the forward's (errors up to 2e-2 of
S(e) at G = 57, non-zero values in entries whose only tap has weight exactly 0); it now carries contract(off) like make_tap2.

The queries run on the tables that the CPU module packs, not on the kernel's own pack: the float64 references are then computed once,
and the pack is tested on its own below.  Still uncovered: the two-launch scan (k_bins_partial + k_bins_final) of grids beyond about
500^3, whose tables are too large for a quick test.
"""
import functools

import numpy as np
import pytest
import torch

from nmf_amd import hip
from test_vm_cpu import (AABB, AD, CA, CD, DL, DP, GRIDS, INV, SHAPES, SHIFT, adjoint_set, batch, bwd_case, fwd_case, fwd_errors,
                         margin_of, one_hot_samples, pack_margin, pack_tables, prints, saved, table_error, table_kind, tables,
                         unpack_case, backward_app, backward_density, adjoints)
from test_shading_rows_cpu import _big

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64
# launch -> (the adjoints of the density half, whether the appearance half runs)
LAUNCHES = {"k_vm_bwd_density<false>": ("value", False), "k_vm_bwd_density<true>": ("full", False),
            "k_vm_bwd_brick<false,2>": ("value", True), "k_vm_bwd_brick<true,2>": ("full", True),
            "k_vm_bwd_brick<false,1>": (None, True)}


def _dev(a, dtype=None):
    t = torch.tensor(np.ascontiguousarray(a)).to(DEV)                # (a copy: the shared inputs are read-only)
    return t if dtype is None else t.to(dtype)


def _params(G):
    return hip.vm_params(AABB, INV, float(SHIFT), G)


@functools.lru_cache(maxsize=None)
def _tabs(G, kind="std", bf16=False):
    tb = tables(G, kind)
    T = tb.bf16 if bf16 else tb.fp32
    dt = torch.bfloat16 if bf16 else None
    return dict(dpk=[_dev(t.reshape(G, G, DP), dt) for t in T.dpk], dlk=[_dev(t, dt) for t in T.dlk],
                apl=[_dev(t.reshape(G, G, CA), dt) for t in T.apl], ali=[_dev(t, dt) for t in T.ali], basis=_dev(T.basis))


def _report(what, err, own, mg):
    """prints the largest error of every metric next to the restatement's, then holds it to the margin"""
    for m in err:
        ratio = f" = {err[m] / own[m]:.2f} x restatement" if own.get(m, 0) > 0 else ""
        print(f"{what} {m}: {err[m]:.3e}{ratio}, margin {mg[m]:.3e}")
    for m in err:
        assert err[m] <= mg[m], f"{what} {m}: {err[m]:.3e} > margin {mg[m]:.3e}"


# ---- pack and unpack --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (5, 6, 17, 19))
def test_pack_density_against_float64(G):
    rng = np.random.default_rng([17, G])
    planes = [rng.standard_normal((G, G, CD)).astype(F32) for _ in range(3)]
    lines = [rng.standard_normal((G, CD)).astype(F32) for _ in range(3)]
    dpk, dlk = hip.vm_pack_density(_params(G), [_dev(p) for p in planes], [_dev(ln) for ln in lines])
    ref, S = pack_tables(planes, lines), pack_tables(planes, lines, absolute=True)
    own, mg = pack_margin(planes, lines)
    err = 0.0
    for got, r, s in zip(dpk + dlk, ref[0] + ref[1], S[0] + S[1]):
        g = got.cpu().numpy().astype(F64).reshape(r.shape)
        assert np.array_equal(g[:, :CD], r[:, :CD])                  # the value block is a copy
        err = max(err, _big((g - r) / np.where(s > 0, s, 1)))
    _report(f"pack G {G}", {"tables": err}, {"tables": own}, {"tables": mg})


def _unpack(G, g_dpk, g_dlk, x=None, l1=None):
    p = _params(G)
    a, b = [_dev(g.reshape(G, G, DP)) for g in g_dpk], [_dev(g) for g in g_dlk]
    arg = None
    if x is not None:
        arg = ([_dev(t) for t in x[0]] + [_dev(t) for t in x[1]], torch.full((), float(l1), dtype=torch.float32, device=DEV))
    gp, gl = hip.vm_unpack_density_grad(p, a, b, l1=arg)
    got = [t[0].permute(1, 2, 0).cpu().numpy() for t in gp] + [t[0, :, :, 0].t().cpu().numpy() for t in gl]
    ref, S, own, mg = unpack_case(g_dpk, g_dlk, G, x=x, l1=l1)
    err = 0.0
    for g, r, s in zip(got, ref[0] + ref[1], S[0] + S[1]):
        assert g.shape == r.shape and not g[s == 0].any()
        err = max(err, _big((g.astype(F64) - r)[s > 0] / s[s > 0]) if (s > 0).any() else 0.0)
    return err, own, mg


@pytest.mark.parametrize("G", (5, 6, 17, 19))
def test_unpack_density_grad_against_the_transposed_stencil(G):
    rng = np.random.default_rng([19, G])
    r = lambda *s: rng.standard_normal(s).astype(F32)      # noqa: E731
    g_dpk, g_dlk = [r(G * G, DP) for _ in range(3)], [r(G, DL) for _ in range(3)]
    err, own, mg = _unpack(G, g_dpk, g_dlk)
    _report(f"unpack G {G} random", {"tables": err}, {"tables": own}, {"tables": mg})
    x = ([r(G, G, CD) for _ in range(3)], [r(G, CD) for _ in range(3)])
    for t in x[0] + x[1]:
        t.reshape(-1)[::7] = 0.0                                     # parameters that are exactly 0: sign(0) = 0
    err, own, mg = _unpack(G, g_dpk, g_dlk, x=x, l1=F32(3e-4))
    _report(f"unpack G {G} random + l1", {"tables": err}, {"tables": own}, {"tables": mg})
    # one-hot packed gradients: corners, edges, the middle; every channel block
    worst, own_w = 0.0, 0.0
    for (y, xx) in ((0, 0), (0, G - 1), (G - 1, 0), (G - 1, G - 1), (0, G // 2), (G // 2, 0), (G - 1, 1), (1, G - 1), (G // 2, G // 2)):
        for ch in (3, CD + 5, 2 * CD + 11):
            hp = [np.zeros((G * G, DP), F32) for _ in range(3)]
            hl = [np.zeros((G, DL), F32) for _ in range(3)]
            hp[ch % 3][y * G + xx, ch] = F32(1.5)
            hl[(ch + 1) % 3][y, ch % DL] = F32(-0.75)
            err, own, mg = _unpack(G, hp, hl)
            assert err <= mg, (G, y, xx, ch, err, mg)
            worst, own_w = max(worst, err), max(own_w, own)
    print(f"unpack G {G} one-hot: {worst:.3e}, restatement {own_w:.3e}")


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def _cut(d, n):
    return {k: v[:n] for k, v in d.items()}


def _fwd_all(what, G, kind, bf16, n):
    """every forward path on the first n samples of batch(G, kind)"""
    p, T = _params(G), _tabs(G, table_kind(kind), bf16)
    ref, S, own, mg = fwd_case(G, kind, bf16)
    n = len(batch(G, kind)) if n is None else n
    x = _dev(batch(G, kind)[:n])
    ref, S = _cut(ref, n), _cut(S, n)
    num = lambda t: t.cpu().numpy()      # noqa: E731
    dpk, dlk, apl, ali, basis = T["dpk"], T["dlk"], T["apl"], T["ali"], T["basis"]
    out = {}
    sf, sg, gr, nr, ap, cf = hip.vm_query_fwd(p, x, dpk, dlk, apl, ali, basis, want_coef=True)
    out["k_vm_fwd all"] = dict(sigma_feat=num(sf), sigma=num(sg), grad=num(gr), normal=num(nr), app=num(ap), coef=num(cf))
    sf, sg, gr, nr, ap, cf = hip.vm_query_fwd(p, x, dpk, dlk, apl, ali, basis, want_normal=False)
    assert gr is None and nr is None and cf is None
    out["k_vm_fwd value + app"] = dict(sigma_feat=num(sf), sigma=num(sg), app=num(ap))
    sf, sg, gr, nr, ap, cf = hip.vm_query_fwd(p, x, dpk, dlk, apl, ali, basis, want_density=False, want_app=False, want_coef=True)
    assert sf is None and ap is None
    out["k_vm_fwd normal + coef"] = dict(grad=num(gr), normal=num(nr), coef=num(cf))
    sf, sg, *_ = hip.vm_query_fwd(p, x, dpk, dlk, None, None, None, want_normal=False, want_app=False)
    out["k_vm_sigma packed"] = dict(sigma_feat=num(sf), sigma=num(sg))
    sf, gr, nr = hip.vm_query_rows(p, x, dpk, dlk)
    out["k_vm_rows_dn"] = dict(sigma_feat=num(sf), grad=num(gr), normal=num(nr))
    *_, ap, cf = hip.vm_query_fwd(p, x, None, None, apl, ali, basis, want_density=False, want_normal=False)
    out["k_vm_app_rows"] = dict(app=num(ap))
    for name, got in out.items():
        err = fwd_errors(got, ref, S)
        if n == len(batch(G, kind)):
            _report(f"{what} {name}", err, own, mg)
        for m in err:
            assert err[m] <= mg[m], f"{what} first {n} {name} {m}: {err[m]:.3e} > margin {mg[m]:.3e}"
    # the value from the density factors themselves (a third of the bytes)
    tb = tables(G, table_kind(kind))
    raw = tb.raw16 if bf16 else tb.raw
    dt = torch.bfloat16 if bf16 else None
    sf, sg = hip.vm_query_sigma(p, x, [_dev(t.reshape(G, G, CD), dt) for t in raw.dpk], [_dev(t, dt) for t in raw.dlk])
    ref, S, own, mg = fwd_case(G, kind, bf16, "raw")
    err = fwd_errors(dict(sigma_feat=num(sf), sigma=num(sg)), _cut(ref, n), _cut(S, n))
    if n == len(batch(G, kind)):
        _report(f"{what} k_vm_sigma raw factors", err, own, mg)
    for m in err:
        assert err[m] <= mg[m], f"{what} first {n} raw {m}: {err[m]:.3e} > margin {mg[m]:.3e}"


@pytest.mark.parametrize("bf16", (False, True), ids=("fp32", "bf16"))
@pytest.mark.parametrize("G", (17, 19, 129))
def test_forward_against_float64(G, bf16):
    """the full edge batch and its first 1 ... 257 samples (16 lanes per row, 32 rows per workgroup, 256 threads); the ladder batch"""
    tag = "bf16" if bf16 else "fp32"
    _fwd_all(f"G {G} {tag} edge", G, "edge", bf16, None)
    for n in SHAPES:
        _fwd_all(f"G {G} {tag} edge", G, "edge", bf16, n)
    _fwd_all(f"G {G} {tag} ladder", G, "ladder", bf16, None)


@pytest.mark.parametrize("bf16", (False, True), ids=("fp32", "bf16"))
def test_forward_hand_placed_branches(bf16):
    """sigma_feat below -15 and above 1e3, x > 20, |g|^2 <= eps on the all-zero corner"""
    _fwd_all(f"G 17 special {'bf16' if bf16 else 'fp32'}", 17, "special", bf16, None)


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def _grad_tables(G, init=None):
    shapes = dict(g_dpk=(G, G, DP), g_dlk=(G, DL), g_apl=(G, G, CA), g_ali=(G, CA))
    if init is None:
        return {k: [torch.zeros(s, dtype=torch.float32, device=DEV) for _ in range(3)] for k, s in shapes.items()}
    return {k: [_dev(init[k][i].reshape(s)) for i in range(3)] for k, s in shapes.items()}


def _walk(G, kind, launch, basis=True, hot=None, bounds=None, clean=None, out=None, g_basis=None, x=None, d=None, sv=None):
    """one call of vm_query_bwd_segments on batch(G, kind); bounds: the segment boundaries (equal neighbours = an empty segment)"""
    p, T = _params(G), _tabs(G, table_kind(kind))
    mode, app = LAUNCHES[launch]
    x = batch(G, kind) if x is None else x
    d = adjoint_set(G, kind, hot) if d is None else d
    sf, gr = saved(G, kind) if sv is None else sv
    M = len(x)
    cols = [x, sf if mode else None, gr if mode == "full" else None, d["d_sigma"] if mode in ("value", "full") else None,
            d["d_sigma_feat"] if mode else None, d["d_normal"] if mode == "full" else None, d["d_app"] if app else None]
    edges = [0] + list(bounds or []) + [M]
    segs = [tuple(None if c is None else _dev(c[a:b]) for c in cols) for a, b in zip(edges[:-1], edges[1:])]
    out = _grad_tables(G) if out is None else out
    if app and basis and g_basis is None:
        g_basis = torch.zeros((AD, 3 * CA), dtype=torch.float32, device=DEV)
    hip.vm_query_bwd_segments(p, segs, T["dpk"], T["dlk"], T["apl"], T["ali"], T["basis"], out["g_dpk"], out["g_dlk"], out["g_apl"],
                              out["g_ali"], g_basis if (app and basis) else None, clean)
    return out, g_basis


def _check(what, G, got, g_basis, launch, dens, appc, basis=True, init=None, show=True, pooled=None):
    """every table of the walk per entry; the tables of a half that did not run must be untouched.  pooled: table -> the restatement's
    error over a family of cases (the one-hot rows), in place of this case's own"""
    mode, app = LAUNCHES[launch]
    n = {"g_dpk": G * G, "g_dlk": G, "g_apl": G * G, "g_ali": G}
    err, own, mg = {}, {}, {}
    for name in ("g_dpk", "g_dlk", "g_apl", "g_ali"):
        cases = (dens if name in ("g_dpk", "g_dlk") else appc)
        ran = mode is not None if name in ("g_dpk", "g_dlk") else app
        for i in range(3):
            g = got[name][i].cpu().numpy().reshape(n[name], -1)
            base = None if init is None else init[name][i].reshape(g.shape)
            if not ran:
                assert np.array_equal(g, np.zeros_like(g) if base is None else base), f"{what} {name}[{i}] written by a walk without it"
                continue
            err[name] = max(err.get(name, 0.0), table_error(g, cases[name][i], base))
        if ran:
            own[name], mg[name] = margin_of(cases[name], pooled and pooled[name])
    if app and basis:
        c = appc["g_basis"]
        g = g_basis.cpu().numpy().astype(F64)
        base = np.zeros_like(g) if init is None else init["g_basis"].astype(F64)
        live = c.S > 0
        assert np.array_equal(g[~live], base[~live])
        err["g_basis"] = _big((g - c.ref)[live] / c.S[live]) if live.any() else 0.0
        own["g_basis"], mg["g_basis"] = margin_of([c], pooled and pooled["g_basis"])
    if show:
        _report(what, err, own, mg)
    for m in err:
        assert err[m] <= mg[m], f"{what} {m}: {err[m]:.3e} > margin {mg[m]:.3e}"
    return err


def _cases(G, kind, launch, hot=None):
    mode, app = LAUNCHES[launch]
    return (bwd_case(G, kind, mode, hot) if mode else None), (bwd_case(G, kind, "app", hot) if app else None)


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("G", GRIDS)
def test_backward_ladder_per_entry(G, launch):
    """brick populations 1 ... 700 (odd pipeline tails, several items of one brick), sparse bricks elsewhere; G = 104: more work items
    than workgroups; G = 129: one counter copy per brick and several scan chunks"""
    dens, appc = _cases(G, "ladder", launch)
    got, gb = _walk(G, "ladder", launch)
    _check(f"G {G} ladder {launch}", G, got, gb, launch, dens, appc)
    if LAUNCHES[launch][1]:
        got, gb = _walk(G, "ladder", launch, basis=False)
        assert gb is None
        _check(f"G {G} ladder {launch} without g_basis", G, got, gb, launch, dens, appc, basis=False, show=False)


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("G", GRIDS)
def test_backward_edge_batch_per_entry(G, launch):
    dens, appc = _cases(G, "edge", launch)
    got, gb = _walk(G, "edge", launch)
    _check(f"G {G} edge {launch}", G, got, gb, launch, dens, appc)


@pytest.mark.parametrize("launch", ("k_vm_bwd_brick<true,2>", "k_vm_bwd_density<false>"))
@pytest.mark.parametrize("G", GRIDS)
def test_backward_one_hot_rows(G, launch):
    """the edge batch with the adjoints of ONE sample: S(e) is a single term, a wrong cell or weight is an error of order one.  The
    margin of a table is the largest over the one-hot samples of this grid (one sample's restatement is a handful of roundings)"""
    hots = one_hot_samples(G)
    cases = {k: _cases(G, "edge", launch, h) for k, h in hots.items()}
    pooled = {}
    for dens, appc in cases.values():
        for c in (dens, appc):
            for name, v in (c or {}).items():
                pooled[name] = max(pooled.get(name, 0.0), margin_of(v if isinstance(v, list) else [v])[0])
    worst = {}
    for key, h in hots.items():
        dens, appc = cases[key]
        got, gb = _walk(G, "edge", launch, hot=h)
        err = _check(f"G {G} one-hot {key} {launch}", G, got, gb, launch, dens, appc, show=False, pooled=pooled)
        for m, e in err.items():
            worst[m] = max(worst.get(m, 0.0), e)
    for m, e in worst.items():
        print(f"G {G} one-hot rows {launch} {m}: {e:.3e} = {e / pooled[m]:.2f} x restatement, margin {margin_of([], pooled[m])[1]:.3e}")


@pytest.mark.parametrize("launch", ("k_vm_bwd_density<true>", "k_vm_bwd_brick<true,2>"))
def test_backward_hand_placed_branches(launch):
    """clamp' = 0 beyond [-15, 1e3], softplus' = 1 above the threshold, and the normalize adjoint on the all-zero corner (n2 <= eps)"""
    dens, appc = _cases(17, "special", launch)
    got, gb = _walk(17, "special", launch)
    _check(f"G 17 special {launch}", 17, got, gb, launch, dens, appc)


def test_backward_item_size_256():
    """M = 400 001 at G = 16: the item size of 256; d_sigma_feat alone"""
    G, kind = 16, "big"
    dens = bwd_case(G, kind, "feat")
    p, T = _params(G), _tabs(G)
    out = _grad_tables(G)
    d = adjoint_set(G, kind)
    hip.vm_query_bwd_segments(p, [(_dev(batch(G, kind)), None, None, None, _dev(d["d_sigma_feat"]), None, None)], T["dpk"], T["dlk"],
                              T["apl"], T["ali"], T["basis"], out["g_dpk"], out["g_dlk"], out["g_apl"], out["g_ali"], None, None)
    _check(f"G {G} M 400001 k_vm_bwd_density<false>", G, out, None, "k_vm_bwd_density<false>", dens, None)


@pytest.mark.parametrize("G", (17, 19, 57))
def test_backward_segments_equal_the_concatenation(G):
    """two, three and four segments with an empty one between them, boundaries off every multiple of 64"""
    launch = "k_vm_bwd_brick<true,2>"
    dens, appc = _cases(G, "ladder", launch)
    M = len(batch(G, "ladder"))
    for bounds in ([M // 3 + 5], [97, 97, M - 33], [1, 1, 1], [M // 2 + 7, M // 2 + 7], [131, 131, 131 + 257]):
        got, gb = _walk(G, "ladder", launch, bounds=bounds)
        _check(f"G {G} ladder segments at {bounds}", G, got, gb, launch, dens, appc, show=(bounds == [97, 97, M - 33]))


@pytest.mark.parametrize("G", (19, 57, 129))
def test_backward_twice_on_one_kept_scratch(G):
    launch = "k_vm_bwd_brick<true,2>"
    dens, appc = _cases(G, "ladder", launch)
    clean = hip.vm_bwd_clean_scratch(_params(G), DEV)
    for rep in range(2):
        got, gb = _walk(G, "ladder", launch, clean=clean)
        _check(f"G {G} ladder kept scratch, walk {rep + 1}", G, got, gb, launch, dens, appc, show=(rep == 1))
    assert not clean.any()                                           # handed back zero


@pytest.mark.parametrize("G", (17, 19))
def test_backward_adds_to_what_the_tables_hold(G):
    """adding is the contract: the tables and g_basis hold values before the walk; an entry that nothing is added to keeps its bits"""
    launch = "k_vm_bwd_brick<true,2>"
    rng = np.random.default_rng([23, G])
    r = lambda *s: rng.standard_normal(s).astype(F32)      # noqa: E731
    init = dict(g_dpk=[r(G * G, DP) for _ in range(3)], g_dlk=[r(G, DL) for _ in range(3)], g_apl=[r(G * G, CA) for _ in range(3)],
                g_ali=[r(G, CA) for _ in range(3)], g_basis=r(AD, 3 * CA))
    fp, tb, x, d = prints(G, "ladder"), tables(G), batch(G, "ladder"), adjoint_set(G, "ladder")
    sf, gr = saved(G, "ladder")
    dens = backward_density(fp, tb.fp32, adjoints(x, sf, gr, d["d_sigma"], d["d_sigma_feat"], d["d_normal"]),
                            init=(init["g_dpk"], init["g_dlk"]))
    appc = backward_app(fp, tb.fp32, d["d_app"], init=(init["g_apl"], init["g_ali"]))
    plain = bwd_case(G, "ladder", "app")["g_basis"]                   # g_basis: the held value is one more term of every entry
    appc["g_basis"].ref, appc["g_basis"].S = plain.ref + init["g_basis"], plain.S + np.abs(init["g_basis"])
    got, gb = _walk(G, "ladder", launch, out=_grad_tables(G, init), g_basis=_dev(init["g_basis"]))
    _check(f"G {G} ladder into held values", G, got, gb, launch, dens, appc, init=init)
