"""Multi-sample frames without a GPU (nmf_amd/multisample.py, csrc/accum.hip): the numpy fp32 restatements of the
four kernels that tests/test_hip_multisample.py compares bit for bit (camera_rays_at_np, accum_update_np, accum_active_np,
accum_resolve_np) against float64, the pixel hash, the pass offsets, the refusals of the entry points, the command line's argument
errors, and the control flow of render_frame driven through its seam: a numpy accumulator behind FrameAccumulator's interface and a
stub in place of render_images."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from test_camera_path_cpu import camera_rays_np, random_pose  # noqa: E402

F = np.float32
U = 2.0 ** -24                                   # half an ulp of 1: the relative error of one fp32 rounding
PLANES, TILE = 15, 256                           # NMF_ACCUM_PLANES, NMF_ACCUM_TILE
PL_COUNT, PL_LIN, PL_ACC, PL_DEPTH, PL_NORMAL, PL_MAP, PL_M2 = 0, 1, 4, 5, 6, 9, 12
SRGB_LIMIT = F(0.0031308)


# ---- the restatements the GPU tests use --------------------------------------------------------------------------------------------
def mix32_np(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def pixel_rotation_np(p, seed):
    """the per-pixel rotation of nmf_camera_rays_at in [0, 1)^2, exact in fp32 (24 bits): uint32 arithmetic as the header states it"""
    p = np.asarray(p, dtype=np.int64).astype(np.uint32)
    h0 = mix32_np(p * np.uint32(0x9E3779B1) + np.uint32((int(seed) * 0x85EBCA77) & 0xFFFFFFFF))
    h1 = mix32_np(h0 + np.uint32(0x9E3779B9))
    return (h0 >> np.uint32(8)).astype(F) * F(2.0 ** -24), (h1 >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def pixel_offsets_np(p, jx, jy, seed, dtype=F):
    """(ox, oy) of the pixels p: (jx, jy) for seed 0, otherwise the rotation added and wrapped, one rounding per operation in dtype"""
    T = dtype
    p = np.asarray(p, dtype=np.int64)
    ox, oy = np.full(p.shape, T(F(jx)), dtype=T), np.full(p.shape, T(F(jy)), dtype=T)
    if int(seed) != 0:
        u0, u1 = pixel_rotation_np(p, seed)
        ox, oy = ox + u0.astype(T), oy + u1.astype(T)
        ox, oy = np.where(ox >= 1, ox - T(1), ox), np.where(oy >= 1, oy - T(1), oy)
    assert ox.dtype == T
    return ox, oy


def camera_rays_at_np(c2w, fx, fy, cx, cy, H, W, jx=0.5, jy=0.5, seed=0, pix=None, out=None, dtype=F, offsets=None):
    """nmf_camera_rays_at in the kernel's order, one rounding per operation in `dtype` -> [n, 6]; rows of list entries outside
    [0, H W) keep what `out` holds (zeros without one).  offsets: (ox, oy) to use instead of the hash's (the float64 comparison)"""
    T = dtype
    P = H * W
    ids = np.arange(P, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64)
    res = np.zeros((len(ids), 6), dtype=T) if out is None else np.array(out, dtype=T)
    ok = (ids >= 0) & (ids < P)
    p = ids[ok]
    m = np.asarray(c2w, dtype=F).astype(T)
    fx, fy, cx, cy = (T(F(v)) for v in (fx, fy, cx, cy))
    ox, oy = pixel_offsets_np(p, jx, jy, seed, T) if offsets is None else (offsets[0][ok].astype(T), offsets[1][ok].astype(T))
    row, col = (p // W).astype(T), (p % W).astype(T)
    x = ((col + ox) - cx) / fx
    y = ((row + oy) - cy) / fy
    n = np.sqrt((x * x + y * y) + T(1))
    dx, dy, dz = x / n, y / n, T(1) / n
    world = [(m[i, 0] * dx + m[i, 1] * dy) + m[i, 2] * dz for i in range(3)]
    origin = [np.full(p.shape, m[i, 3], dtype=T) for i in range(3)]
    res[ok] = np.stack(origin + world, -1)
    assert res.dtype == T
    return res


def state_np(P, dtype=F):
    """a zeroed state: dict(count int32 [P], planes dtype [14, P]: rows PL_* - 1)"""
    return dict(count=np.zeros(P, dtype=np.int32), planes=np.zeros((PLANES - 1, P), dtype=dtype))


def state_words(st, P):
    """the uint32 words of the device state for a numpy state (tile scratch zero)"""
    w = np.zeros(PLANES * P + -(-P // TILE), dtype=np.uint32)
    w[:P] = st["count"].view(np.uint32)
    w[P:PLANES * P] = st["planes"].astype(F).reshape(-1).view(np.uint32)
    return w


def state_from_words(w, P):
    w = np.asarray(w).view(np.uint32)
    return dict(count=w[:P].view(np.int32).copy(), planes=w[P:PLANES * P].view(F).reshape(PLANES - 1, P).copy())


def _nan0(v, T):
    v = np.asarray(v).astype(T)
    return np.where(np.isnan(v), T(0), v)


def accum_update_np(st, rgb_lin, acc, rgb_map, depth=None, normal=None, pix=None):
    """nmf_accum_update in place on a numpy state, in the state's dtype: Welford's update, one rounding per operation"""
    T = st["planes"].dtype.type
    P = st["count"].shape[0]
    ids = np.arange(P, dtype=np.int64) if pix is None else np.asarray(pix, dtype=np.int64)
    ok = (ids >= 0) & (ids < P)
    p = ids[ok]
    st["count"][p] += 1
    c = st["count"][p].astype(T)
    pl = st["planes"]

    def fold(k, x):
        old = pl[k - 1, p]
        d = x - old
        pl[k - 1, p] = old + d / c
        return d

    lin, mp = _nan0(rgb_lin, T).reshape(-1, 3)[ok], _nan0(rgb_map, T).reshape(-1, 3)[ok]
    for k in range(3):
        fold(PL_LIN + k, lin[:, k])
    fold(PL_ACC, _nan0(acc, T).reshape(-1)[ok])
    if depth is not None:
        fold(PL_DEPTH, _nan0(depth, T).reshape(-1)[ok])
    if normal is not None:
        nm = _nan0(normal, T).reshape(-1, 3)[ok]
        for k in range(3):
            fold(PL_NORMAL + k, nm[:, k])
    for k in range(3):
        x = mp[:, k]
        d = fold(PL_MAP + k, x)
        pl[PL_M2 + k - 1, p] = pl[PL_M2 + k - 1, p] + d * (x - pl[PL_MAP + k - 1, p])
    return st


def std_err_np(st):
    """max_c sqrt(M2_c / ((float)count (float)(count - 1))), 0 below two samples, in the state's dtype"""
    T = st["planes"].dtype.type
    n = st["count"]
    cc = n.astype(T) * (n - 1).astype(T)
    se = np.zeros(n.shape, dtype=T)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            v = np.sqrt(st["planes"][PL_M2 + k - 1] / cc)
            se = np.where(np.isnan(v), se, np.maximum(se, v))                       # fmaxf drops a NaN operand
    return np.where(n >= 2, se, T(0)).astype(T)


def accum_active_mask_np(st, min_spp, max_spp, tol):
    n = st["count"]
    T = st["planes"].dtype.type
    return (n < min_spp) | ((n < max_spp) & (std_err_np(st) > T(F(tol))))


def accum_active_np(st, min_spp, max_spp, tol):
    """nmf_accum_active: np.flatnonzero of the predicate -> int32 [n]"""
    return np.flatnonzero(accum_active_mask_np(st, min_spp, max_spp, tol)).astype(np.int32)


def srgb_np(x, noclip, T):
    """nmf_accum_resolve's tonemap: the formula of nmf_ray_compose_fwd with the kernel's fp32 constants; the power in double,
    rounded to `T` once"""
    with np.errstate(invalid="ignore"):
        p = np.power(np.maximum(x, T(SRGB_LIMIT)).astype(np.float64), 1.0 / 2.4).astype(T)
        o = np.where(x > T(SRGB_LIMIT), T(F(1.055)) * p - T(F(0.055)), T(F(12.92)) * x).astype(T)
    return o if noclip else np.minimum(np.maximum(o, T(0)), T(1))


def accum_resolve_np(st, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False):
    """nmf_accum_resolve -> dict(rgb_map [P, 3], acc, depth [P], normal [P, 3], se [P], count [P] float) in the state's dtype"""
    T = st["planes"].dtype.type
    pl = st["planes"]
    a = pl[PL_ACC - 1]
    t = T(1) - a
    rgb = np.stack([(srgb_np(pl[PL_LIN + k - 1], noclip, T) if tonemap else pl[PL_LIN + k - 1]) + t * T(F(bg[k])) for k in range(3)], -1)
    assert rgb.dtype == T
    return dict(rgb_map=rgb, acc=a.copy(), depth=pl[PL_DEPTH - 1].copy(), normal=np.stack([pl[PL_NORMAL + k - 1] for k in range(3)], -1),
                se=std_err_np(st), count=st["count"].astype(T))


def random_pass(rng, n, nan_every=0):
    """the inputs of one pass for n list entries: radiance up to 1.2, acc in [0, 1], the displayed colour in [0, 1], depth 2..6, unit
    normals; nan_every > 0 plants NaNs"""
    lin = rng.uniform(0, 1.2, size=(n, 3)).astype(F)
    acc = rng.uniform(0, 1, size=n).astype(F)
    mp = rng.uniform(0, 1, size=(n, 3)).astype(F)
    depth = rng.uniform(2, 6, size=n).astype(F)
    nm = rng.normal(size=(n, 3))
    nm = (nm / np.linalg.norm(nm, axis=-1, keepdims=True)).astype(F)
    if nan_every and n:
        lin[::nan_every, 1] = np.nan
        mp[1::nan_every, 0] = np.nan
        acc[2::nan_every] = np.nan
    return lin, acc, mp, depth, nm


def random_sublist(rng, P, kind):
    if kind == "full":
        return np.arange(P, dtype=np.int32)
    if kind == "empty":
        return np.zeros(0, dtype=np.int32)
    return np.flatnonzero(rng.random(P) < rng.uniform(0.05, 0.9)).astype(np.int32)


def run_passes(P, n_pass, seed, dtype=F, with_maps=True, record=None):
    """n_pass updates of a P-pixel state with a different random ascending sub-list each (pass 3 empty, pass 5 full, pass 0 full so
    that every pixel has a sample) -> the state; record(k, pix, inputs) sees every pass"""
    rng = np.random.default_rng(seed)
    st = state_np(P, dtype)
    for k in range(n_pass):
        pix = random_sublist(rng, P, "full" if k in (0, 5) else "empty" if k == 3 else "random")
        inputs = random_pass(rng, len(pix), nan_every=7 if k == 2 else 0)
        if record is not None:
            record(k, pix, inputs)
        lin, acc, mp, depth, nm = inputs
        accum_update_np(st, lin, acc, mp, depth if with_maps else None, nm if with_maps else None, pix)
    return st


# ---- restatements against float64 --------------------------------------------------------------------------------------------------
def test_hash_rotation_range_and_seeds():
    p = np.arange(200000)
    seen = []
    for seed in (1, 2, 3, 0xFFFFFFFF):
        u0, u1 = pixel_rotation_np(p, seed)
        assert u0.dtype == F and u0.min() >= 0 and u0.max() < 1 and u1.min() >= 0 and u1.max() < 1
        # 24-bit values: exact in fp32; both coordinates fill the interval evenly (200000 draws: mean within 5 sigma of 1/2)
        assert abs(float(u0.mean()) - 0.5) <= 5 * (1 / 12 / len(p)) ** 0.5 and abs(float(u1.mean()) - 0.5) <= 5 * (1 / 12 / len(p)) ** 0.5
        assert abs(float(np.corrcoef(u0, u1)[0, 1])) <= 5 / len(p) ** 0.5
        seen.append((u0, u1))
    for a in range(len(seen)):
        for b in range(a + 1, len(seen)):
            assert (seen[a][0] != seen[b][0]).mean() > 0.99 and (seen[a][1] != seen[b][1]).mean() > 0.99
    # seed 0 is no rotation; with a seed the offsets stay in [0, 1), also at the ends of the allowed jitter
    ox, oy = pixel_offsets_np(p, 0.25, 0.75, 0)
    assert (ox == F(0.25)).all() and (oy == F(0.75)).all()
    for jx, jy in ((0.0, 1.0), (1.0, 0.0), (0.5, 0.99999994)):
        ox, oy = pixel_offsets_np(p, jx, jy, 7)
        assert ox.min() >= 0 and ox.max() < 1 and oy.min() >= 0 and oy.max() < 1
    # a value written down: the hash of pixel 12345 under seed 3 by Python integers
    def mix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    h0 = mix((12345 * 0x9E3779B1 + 3 * 0x85EBCA77) & 0xFFFFFFFF)
    h1 = mix((h0 + 0x9E3779B9) & 0xFFFFFFFF)
    u0, u1 = pixel_rotation_np([12345], 3)
    assert float(u0[0]) == (h0 >> 8) / 2 ** 24 and float(u1[0]) == (h1 >> 8) / 2 ** 24


def test_pass_offsets():
    from nmf_amd.multisample import PLASTIC, pass_offset
    assert pass_offset(0) == (0.5, 0.5)
    pts = np.array([pass_offset(k) for k in range(4096)])
    assert pts.min() >= 0.0 and pts.max() < 1.0
    assert np.array_equal(pts.astype(F).astype(np.float64), pts)                         # fp32 values
    k = np.arange(4096, dtype=np.float64)
    for c in range(2):
        want = np.mod(0.5 + k * PLASTIC[c], 1.0)
        d = np.abs(pts[:, c] - want)
        assert np.minimum(d, 1 - d).max() <= U                                           # float64, then one fp32 rounding (circular)
    assert len({tuple(p) for p in pts[:64]}) == 64
    with pytest.raises(ValueError):
        pass_offset(-1)


def test_ray_restatement_against_float64_and_the_anchor():
    """Bound (not fitted): every direction component within 2^-20 of float64 -- tests/test_camera_path_cpu.py's bound for the same
    chain; the offset adds no rounding to it (col + ox is one rounding either way).  The float64 run takes the fp32 offsets: the wrap
    of a sum that rounds to 1 is a jump in the offset, not an error of the ray."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for H, W in ((5, 7), (37, 53)):
        c2w = random_pose(rng)
        fx, fy, cx, cy = 111.25, 97.5, W / 2 + 1.75, H / 2 - 2.25
        anchor = camera_rays_at_np(c2w, fx, fy, cx, cy, H, W)
        assert np.array_equal(anchor.view(np.uint32), camera_rays_np(c2w, fx, fy, cx, cy, H, W).view(np.uint32))
        for seed, (jx, jy) in ((0, (0.25, 0.75)), (1, (0.5, 0.5)), (9, (0.0, 1.0))):
            pix = np.flatnonzero(rng.random(H * W) < 0.5).astype(np.int32)
            got = camera_rays_at_np(c2w, fx, fy, cx, cy, H, W, jx, jy, seed, pix)
            off = pixel_offsets_np(pix, jx, jy, seed)
            ref = camera_rays_at_np(c2w, fx, fy, cx, cy, H, W, jx, jy, seed, pix, dtype=np.float64, offsets=off)
            worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
            # the offsets themselves: float64 and fp32 agree on the circle to one rounding
            o64 = pixel_offsets_np(pix, jx, jy, seed, np.float64)
            for a, b in zip(off, o64):
                d = np.abs(a.astype(np.float64) - b)
                assert np.minimum(d, 1 - d).max() <= U
            # a jittered ray differs from the centre ray and stays inside its pixel's cone
            if seed:
                centre = camera_rays_at_np(c2w, fx, fy, cx, cy, H, W, pix=pix)
                assert (got[:, 3:] != centre[:, 3:]).any(axis=1).mean() > 0.99
                assert np.abs(got[:, 3:] - centre[:, 3:]).max() <= 1.0 / min(fx, fy)
    print("camera_rays_at_np - float64, units of 2^-24:", worst / U, "(margin for a non-identical comparison: 4 x)")
    assert worst <= 2.0 ** -20
    # list entries outside the frame keep the buffer
    out = np.full((4, 6), 7.0, dtype=F)
    got = camera_rays_at_np(np.eye(4), 50.0, 50.0, 3.5, 2.5, 5, 7, pix=[-1, 3, 35, 34], out=out)
    assert (got[[0, 2]] == 7.0).all() and (got[[1, 3]] != 7.0).any(axis=1).all()


def test_update_restatement_against_float64():
    """Bounds from the roundings (u = 2^-24, R = the largest |x| of a quantity, n passes): a mean's error contracts by 1 - 1 / count
    per step and gains at most 2 u R / c + 2 u R / c + u R <= 5 u R, so at most 5 n u R; M2 gains per step t at most
    2 R (e_mean(t - 1) + e_mean(t) + 4 u R) + 4 u R^2 (the product) + 4 u R^2 t (the sum): in all (12 n^2 + 24 n) u R^2."""
    P, n = 37 * 53, 17
    st32 = run_passes(P, n, seed=11)
    st64 = run_passes(P, n, seed=11, dtype=np.float64)
    assert np.array_equal(st32["count"], st64["count"]) and st32["count"].min() >= 2 and st32["count"].max() <= n - 1
    dev = np.abs(st32["planes"].astype(np.float64) - st64["planes"])
    R = dict(lin=1.2, acc=1.0, depth=6.0, normal=1.0, map=1.0)
    rows = dict(lin=slice(0, 3), acc=slice(3, 4), depth=slice(4, 5), normal=slice(5, 8), map=slice(8, 11))
    for name, sl in rows.items():
        print(f"mean {name}: |fp32 - float64| = {dev[sl].max() / U:.2f} u (bound {5 * n * R[name]:.0f} u)")
        assert dev[sl].max() <= 5 * n * U * R[name]
    print(f"M2: |fp32 - float64| = {dev[11:14].max() / U:.2f} u (bound {12 * n * n + 24 * n} u)")
    assert dev[11:14].max() <= (12 * n * n + 24 * n) * U
    # after exactly one full pass the means are the inputs' bits and M2 is 0
    rng = np.random.default_rng(3)
    lin, acc, mp, depth, nm = random_pass(rng, P)
    st = accum_update_np(state_np(P), lin, acc, mp, depth, nm)
    pl = st["planes"]
    for got, want in ((pl[0:3].T, lin), (pl[3], acc), (pl[4], depth), (pl[5:8].T, nm), (pl[8:11].T, mp)):
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert not pl[11:14].any() and (st["count"] == 1).all()
    # a NaN counts as 0; entries outside the frame are skipped; without depth / normal those means stay
    st = accum_update_np(state_np(4), [[np.nan, 1, 2]] * 3, [np.nan, 1, 1], [[0.5, np.nan, 1]] * 3, pix=[-1, 2, 4])
    assert st["count"].tolist() == [0, 0, 1, 0] and st["planes"][:, 2].tolist() == [0, 1, 2, 1, 0, 0, 0, 0, 0.5, 0, 1, 0, 0, 0]
    # Welford against the two-pass definition in float64
    x = np.random.default_rng(0).uniform(0, 1, size=(9, 5, 3))
    st = state_np(5, np.float64)
    for k in range(9):
        accum_update_np(st, x[k], x[k, :, 0], x[k])
    assert np.abs(st["planes"][8:11].T - x.mean(0)).max() <= 1e-15
    assert np.abs(st["planes"][11:14].T - ((x - x.mean(0)) ** 2).sum(0)).max() <= 1e-14
    assert np.abs(std_err_np(st) - (x.std(0, ddof=1) / 3.0).max(-1)).max() <= 1e-15


def test_active_and_resolve_restatements_against_float64():
    """Given the same state (the fp32 state's values), se is two roundings (the quotient, the root; count (count - 1) is exact):
    within 3 u relative.  The lists agree wherever float64's se is further than that from tol.  rgb_map is the correctly rounded power
    (u p), its product with 1.055 (u), the subtraction (u), 1 - acc (u), its product with bg (u) and the sum (u |rgb|): values up to
    ~1.2 here, so within 8 u; acc, depth, normal and count are copies."""
    P, n = 37 * 53, 17
    st32 = run_passes(P, n, seed=13)
    st64 = dict(count=st32["count"].copy(), planes=st32["planes"].astype(np.float64))
    se32, se64 = std_err_np(st32), std_err_np(st64)
    assert se32.dtype == F and (se64 > 0).all()
    rel = np.abs(se32.astype(np.float64) - se64) / se64
    print(f"se: |fp32 - float64| / se = {rel.max() / U:.2f} u (bound 3 u)")
    assert rel.max() <= 3 * U
    tol = float(np.median(se64))
    for min_spp, max_spp in ((4, 16), (1, 8), (12, 12)):
        a32, a64 = accum_active_mask_np(st32, min_spp, max_spp, tol), accum_active_mask_np(st64, min_spp, max_spp, tol)
        clear = np.abs(se64 - float(F(tol))) > 3 * U * se64
        assert np.array_equal(a32[clear], a64[clear]) and 0 < a32.sum() < P
        lst = accum_active_np(st32, min_spp, max_spp, tol)
        assert lst.dtype == np.int32 and np.array_equal(lst, np.flatnonzero(a32)) and (np.diff(lst) > 0).all()
    # the predicate's corners: below min_spp always, at max_spp never, tol 0 / inf
    st = state_np(6)
    st["count"][:] = [0, 3, 4, 4, 16, 1]
    st["planes"][PL_M2 - 1] = [0, 0, 0, 2.0, 2.0, 5.0]
    assert accum_active_np(st, 4, 16, 0.0).tolist() == [0, 1, 3, 5]
    assert accum_active_np(st, 4, 16, np.inf).tolist() == [0, 1, 5]
    assert accum_active_np(st, 1, 16, 0.0).tolist() == [0, 3] and std_err_np(st).tolist()[5] == 0.0
    assert std_err_np(st)[3] == np.sqrt(F(2.0) / F(12.0))
    worst = 0.0
    for tonemap in (True, False):
        for noclip in (True, False):
            r32 = accum_resolve_np(st32, (1.0, 0.5, 0.25), tonemap, noclip)
            r64 = accum_resolve_np(st64, (1.0, 0.5, 0.25), tonemap, noclip)
            worst = max(worst, float(np.abs(r32["rgb_map"].astype(np.float64) - r64["rgb_map"]).max()))
            for k in ("acc", "depth", "normal", "count"):
                assert np.array_equal(r32[k].astype(np.float64), r64[k])
            assert r32["rgb_map"].dtype == F and r32["se"].dtype == F
    print(f"rgb_map: |fp32 - float64| = {worst / U:.2f} u (bound 8 u)")
    assert worst <= 8 * U
    # srgb at its knee and its clip, fp32: the linear branch on the knee, the power branch one float above; clipped unless noclip
    x = np.array([0.0, SRGB_LIMIT, np.nextafter(SRGB_LIMIT, F(1)), 1.0, 1.2, -0.5], dtype=F)
    o = srgb_np(x, True, F)
    assert o[1] == F(12.92) * SRGB_LIMIT and abs(float(o[2]) - float(o[1])) <= 1e-4 and o[3] == F(1.055) - F(0.055)
    assert o[4] > 1 and o[5] < 0 and srgb_np(x, False, F)[4] == 1 and srgb_np(x, False, F)[5] == 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
POSE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.5, 0.25, 2.0]
NAMES = ("nmf_accum_state_bytes", "nmf_camera_rays_at", "nmf_accum_update", "nmf_accum_active", "nmf_accum_resolve")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    f, i, p = C.c_float, C.c_int32, C.c_void_p
    lib.nmf_accum_state_bytes.argtypes, lib.nmf_accum_state_bytes.restype = [i, i], C.c_int64
    lib.nmf_camera_rays_at.argtypes = [f] * 16 + [i, i, f, f, C.c_uint32, p, C.c_int64, p, p]
    lib.nmf_accum_update.argtypes = [p, i, i, p, C.c_int64, p, p, p, p, p, p]
    lib.nmf_accum_active.argtypes = [p, i, i, i, i, f, p, p, p]
    lib.nmf_accum_resolve.argtypes = [p, i, i, f, f, f, i, i, p, p, p, p, p, p, p]
    return lib, hip


def test_symbols_are_declared_exported_and_bound():
    lib, hip = _lib()
    hdr = open(os.path.join(ROOT, "include", "nmf_hip.h")).read()
    for name in NAMES:
        assert f" {name}(" in hdr and hasattr(lib, name) and name in hip.EXPORTS
    assert "#define NMF_ACCUM_PLANES %d" % PLANES in hdr and "#define NMF_ACCUM_TILE %d" % TILE in hdr
    assert (hip.ACCUM_PLANES, hip.ACCUM_TILE) == (PLANES, TILE)
    assert "#define NMF_ABI_VERSION %d" % hip.version() in hdr
    build = open(os.path.join(ROOT, "nmf_amd", "csrc", "build.sh")).read()
    assert "accum.hip" in [ln for ln in build.splitlines() if "-ffp-contract=off" in ln and "camera.hip" in ln][0]
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "nmf_amd", "csrc", "accum.hip")).read()


def test_state_size_is_host_arithmetic():
    lib, hip = _lib()
    for H, W in ((1, 1), (5, 7), (37, 53), (16, 16), (800, 800), (1, 70001)):
        P = H * W
        assert lib.nmf_accum_state_bytes(H, W) == 4 * (PLANES * P + -(-P // TILE)) == hip.accum_state_bytes(H, W)
        assert len(state_words(state_np(P), P)) * 4 == hip.accum_state_bytes(H, W)
    for H, W in ((0, 5), (5, -1), (46341, 46341)):
        assert lib.nmf_accum_state_bytes(H, W) == 0
        with pytest.raises(hip.NmfHipError):
            hip.accum_state_bytes(H, W)


def test_refusals_name_the_function():
    """every refusal with NULL device pointers: nothing can be launched, and the argument checks come before the pointers'"""
    lib, _ = _lib()
    inf, nan = float("inf"), float("nan")

    def rays_at(pose=POSE, fx=100.0, fy=90.0, cx=3.0, cy=4.0, H=5, W=7, jx=0.5, jy=0.5, seed=0, n=0):
        return lib.nmf_camera_rays_at(*pose, fx, fy, cx, cy, H, W, jx, jy, seed, None, n, None, None)
    cases = [(dict(), -1, b"null pointer"), (dict(H=0), -1, b"below 1"), (dict(W=-3), -1, b"below 1"), (dict(fx=0.0), -1, b"fx and fy"),
             (dict(fy=inf), -1, b"fx and fy"), (dict(cx=nan), -1, b"finite"), (dict(n=-1), -1, b"n below 0"),
             (dict(jx=-0.001), -1, b"offset"), (dict(jy=1.001), -1, b"offset"), (dict(jx=nan), -1, b"offset"), (dict(jy=inf), -1, b"offset"),
             (dict(H=46341, W=46341), -2, b"2^31 - 1"), (dict(n=2 ** 31), -2, b"2^31 - 1")]
    for k in (0, 5, 11):
        cases.append((dict(pose=POSE[:k] + [nan] + POSE[k + 1:]), -1, b"finite"))
    for kw, code, word in cases:
        assert rays_at(**kw) == code, kw
        msg = lib.nmf_last_error_string()
        assert b"nmf_camera_rays_at" in msg and word in msg, (kw, msg)
    assert rays_at(jx=0.0, jy=1.0) == -1 and b"null pointer" in lib.nmf_last_error_string()          # the ends of [0, 1] are allowed

    def update(H=5, W=7, n=0):
        return lib.nmf_accum_update(None, H, W, None, n, None, None, None, None, None, None)
    for kw, code, word in [(dict(), -1, b"null pointer"), (dict(H=0), -1, b"below 1"), (dict(W=0), -1, b"below 1"), (dict(n=-2), -1, b"n below 0"),
                           (dict(H=46341, W=46341), -2, b"2^31 - 1"), (dict(n=2 ** 31), -2, b"2^31 - 1")]:
        assert update(**kw) == code, kw
        msg = lib.nmf_last_error_string()
        assert b"nmf_accum_update" in msg and word in msg, (kw, msg)

    def active(H=5, W=7, lo=4, hi=16, tol=0.01):
        return lib.nmf_accum_active(None, H, W, lo, hi, tol, None, None, None)
    for kw, code, word in [(dict(), -1, b"null pointer"), (dict(H=0), -1, b"below 1"), (dict(lo=-1), -1, b"min_spp"), (dict(lo=5, hi=4), -1, b"min_spp"),
                           (dict(tol=-1.0), -1, b"tol"), (dict(tol=nan), -1, b"tol"), (dict(H=46341, W=46341), -2, b"2^31 - 1")]:
        assert active(**kw) == code, kw
        msg = lib.nmf_last_error_string()
        assert b"nmf_accum_active" in msg and word in msg, (kw, msg)
    assert active(tol=inf) == -1 and b"null pointer" in lib.nmf_last_error_string()                    # +inf is a tolerance

    def resolve(H=5, W=7, bg=(1.0, 1.0, 1.0)):
        return lib.nmf_accum_resolve(None, H, W, *bg, 1, 0, None, None, None, None, None, None, None)
    for kw, code, word in [(dict(), -1, b"null state"), (dict(W=0), -1, b"below 1"), (dict(bg=(1.0, nan, 1.0)), -1, b"bg"),
                           (dict(bg=(inf, 0.0, 1.0)), -1, b"bg"), (dict(H=46341, W=46341), -2, b"2^31 - 1")]:
        assert resolve(**kw) == code, kw
        msg = lib.nmf_last_error_string()
        assert b"nmf_accum_resolve" in msg and word in msg, (kw, msg)


def test_wrappers_refuse_host_tensors():
    _, hip = _lib()
    from nmf_amd.multisample import FrameAccumulator
    state = torch.zeros(hip.accum_state_bytes(4, 4) // 4, dtype=torch.int32)
    z = torch.zeros
    with pytest.raises(hip.NmfHipError):
        hip.camera_rays_at(np.eye(4), 100.0, 100.0, 4.0, 4.0, 8, 8, device="cpu")
    with pytest.raises(hip.NmfHipError):
        hip.camera_rays_at(np.eye(4), 100.0, 100.0, 4.0, 4.0, 8, 8, pix=z(3, dtype=torch.int32))
    with pytest.raises(hip.NmfHipError):
        hip.accum_update(state, 4, 4, z(16, 3), z(16), z(16, 3))
    with pytest.raises(hip.NmfHipError):
        hip.accum_active(state, 4, 4, 4, 16, 0.01)
    with pytest.raises(hip.NmfHipError):
        hip.accum_resolve(state, 4, 4)
    with pytest.raises(hip.NmfHipError):
        FrameAccumulator(4, 4, "cpu")


def test_render_argument_errors(capsys):
    from nmf_amd import render as R
    base = ["--ckpt", "none.th"]
    for extra, word in ((["--datadir", "d", "--eval-dir", "e", "--material-maps", "--spp", "4"], "not accumulated"),
                        (["--adaptive", "1"], "--adaptive needs --spp"), (["--adaptive"], "--adaptive needs --spp"),
                        (["--spp", "4", "--min-spp", "5"], "--min-spp"), (["--spp", "4", "--min-spp", "0"], "--min-spp"),
                        (["--spp", "0"], "--spp is at least 1"), (["--spp", "4", "--adaptive", "-1"], "--adaptive takes")):
        with pytest.raises(SystemExit) as e:
            R.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra


# ---- render_frame's loop -----------------------------------------------------------------------------------------------------------
class NumpyAccumulator:
    """FrameAccumulator's interface over the numpy restatements: the seam of render_frame(accumulator=)"""

    def __init__(self, H, W):
        self.H, self.W, self.device = H, W, torch.device("cpu")
        self.reset()
        self.resets = 0

    def reset(self):
        self.st = state_np(self.H * self.W)
        self.resets = getattr(self, "resets", 0) + 1

    def update(self, ims, pix=None):
        g = lambda k: None if ims.get(k) is None else ims[k].numpy()      # noqa: E731
        accum_update_np(self.st, g("rgb_lin"), g("acc_map"), g("rgb_map"), g("depth"), g("world_normal"), None if pix is None else pix.numpy())

    def active(self, min_spp, max_spp, tol):
        lst = accum_active_np(self.st, min_spp, max_spp, tol)
        return torch.from_numpy(lst), len(lst)

    def resolve(self, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False, keys=()):
        r = accum_resolve_np(self.st, bg, tonemap, noclip)
        names = dict(rgb_map="rgb_map", acc_map="acc", depth="depth", world_normal="normal", se="se", count="count")
        return {k: torch.from_numpy(r[v]) for k, v in names.items() if k in keys or k in ("se", "count")}


class StubRender:
    """stands in for render_images: the pixel id travels in the ray's first component.  Pixels with id % 3 == 0 get a constant colour,
    the others alternate between two displayed colours from call to call (0.2 / 0.6: a standard error far above 1 / 255)"""

    def __init__(self):
        self.calls = []

    def __call__(self, nerf, rays, focal, chunk=None, noise=None, keys=("rgb_map",)):
        ids = rays[:, 0].long()
        k = len(self.calls)
        self.calls.append((ids.clone(), tuple(keys)))
        noisy = (ids % 3 != 0).float()
        v = 0.4 + noisy * (0.2 if k % 2 else -0.2)
        rgb = v[:, None].repeat(1, 3)
        out = dict(rgb_map=rgb, rgb_lin=rgb * 0.5, acc_map=torch.ones_like(v))
        if "depth" in keys:
            out["depth"] = ids.float()
        if "world_normal" in keys:
            out["world_normal"] = rgb.clone()
        return out


def _stub_rays(P):
    rays = torch.zeros(P, 6)
    rays[:, 0] = torch.arange(P)
    return rays


def test_render_frame_control_flow_with_a_stub():
    from nmf_amd.multisample import render_frame
    P, spp, min_spp = 300, 16, 4
    rays = _stub_rays(P)
    ids = np.arange(P)
    # adaptive: constant pixels end at min_spp, the others at spp; the work is the sum of the counts
    stub, acc = StubRender(), NumpyAccumulator(1, P)
    ims, stats = render_frame(None, rays, 50.0, spp=spp, min_spp=min_spp, tol=1 / 255, jitter=False, keys=("rgb_map", "depth"),
                              accumulator=acc, render=stub)
    count = ims["count"].numpy()
    assert (count[ids % 3 == 0] == min_spp).all() and (count[ids % 3 != 0] == spp).all()
    assert stats == dict(passes=spp, rays_rendered=int(count.sum())) and acc.resets == 1
    assert (ims["se"].numpy()[ids % 3 == 0] == 0).all() and (ims["se"].numpy()[ids % 3 != 0] > 1 / 255).all()
    assert set(ims) == {"rgb_map", "depth", "se", "count"} and np.array_equal(ims["depth"].numpy(), ids.astype(F))
    for k, (got, keys) in enumerate(stub.calls):
        assert set(keys) == {"rgb_map", "acc_map", "rgb_lin", "depth"}
        assert np.array_equal(got.numpy(), ids if k < min_spp else ids[ids % 3 != 0])              # all pixels first, then the ascending list
    # the mean is taken on rgb_lin and tonemapped afterwards: srgb(mean of 0.1 and 0.3) for a noisy pixel, not the mean of the colours
    # (bound: the mean's 5 n u R of test_update_restatement_against_float64 times the tonemap's slope there, below 1.2)
    want = srgb_np(np.array([F(0.2)]), False, F)[0]
    assert abs(float(ims["rgb_map"][1, 0]) - float(want)) <= 1.2 * 5 * spp * U and abs(float(ims["rgb_map"][1, 0]) - 0.4) > 0.05
    # fixed count: every pixel gets spp samples, no list is asked for
    stub, acc = StubRender(), NumpyAccumulator(1, P)
    acc.active = None
    ims, stats = render_frame(None, rays, 50.0, spp=spp, min_spp=min_spp, tol=None, jitter=False, accumulator=acc, render=stub)
    assert (ims["count"].numpy() == spp).all() and stats == dict(passes=spp, rays_rendered=spp * P) and set(ims) == {"rgb_map", "se", "count"}
    # a huge tolerance ends after min_spp passes; tol 0 keeps every pixel with M2 > 0 to the end; min_spp above spp is spp
    stub = StubRender()
    ims, stats = render_frame(None, rays, 50.0, spp=spp, min_spp=min_spp, tol=float("inf"), jitter=False, accumulator=NumpyAccumulator(1, P),
                              render=stub)
    assert stats == dict(passes=min_spp, rays_rendered=min_spp * P) and len(stub.calls) == min_spp
    ims, stats = render_frame(None, rays, 50.0, spp=spp, min_spp=min_spp, tol=0.0, jitter=False, accumulator=NumpyAccumulator(1, P),
                              render=StubRender())
    assert (ims["count"].numpy()[ids % 3 != 0] == spp).all() and (ims["count"].numpy()[ids % 3 == 0] == min_spp).all()
    ims, stats = render_frame(None, rays, 50.0, spp=2, min_spp=4, tol=1 / 255, jitter=False, accumulator=NumpyAccumulator(1, P),
                              render=StubRender())
    assert (ims["count"].numpy() == 2).all() and stats["passes"] == 2
    # refusals of the loop itself
    for kw in (dict(spp=0), dict(spp=4, min_spp=0), dict(spp=4, tol=-1.0), dict(spp=4, tol=float("nan")), dict(spp=4, keys=("albedo",)),
               dict(spp=4, jitter=True), dict(spp=4, accumulator=NumpyAccumulator(1, P + 1))):
        args = dict(jitter=False, accumulator=NumpyAccumulator(1, P), render=StubRender())
        args.update(kw)
        with pytest.raises(ValueError):
            render_frame(None, rays, 50.0, **args)
