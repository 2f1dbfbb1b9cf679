"""Relighting without a GPU: the float64 numpy restatement of csrc/envmap_resample.hip (the definition the kernel is held to), the
conventions it rests on pinned against the CPU oracle's lookup, the error of a resampled map against analytic radiance, argument
validation through the C ABI, and the fp32-vs-float64 margin the GPU tests (tests/test_hip_relight.py) use as their tolerance."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

H, W = 32, 64                      # destination grid
PANO = (96, 192)                   # panorama
PANO_ODD = (50, 101)               # an odd one: Wp is neither 2 Hp nor a power of two
SA = math.log(1e-5)                # the sharpest footprint (pano2env.fit's)


# ---- the shared analytic input ------------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(0)
A = _rng.normal(size=(3, 3))
B = 0.5 * _rng.normal(size=(3, 3, 3))


def radiance(d):
    """L_c(d) = exp(0.4 A_c . d + 0.4 d^T B_c d); d [...,3] -> [...,3]"""
    d = np.asarray(d, dtype=np.float64)
    return np.exp(0.4 * np.einsum("ck,...k->...c", A, d) + 0.4 * np.einsum("...k,ckl,...l->...c", d, B, d))


def rotations():
    from nmf_amd import relight
    return {"identity": np.eye(3), "yaw90": relight.rotation(yaw=90), "x90": relight.axis_angle((1, 0, 0), math.pi / 2),
            "axis": relight.axis_angle((1, 2, 0.5), 0.9)}


def dir_to_coords(d):
    a, b, c = d[..., 0], d[..., 1], d[..., 2]
    return (np.mod(np.arctan2(b, a), 2 * np.pi) - np.pi) / np.pi, -2 * np.arctan2(c, np.hypot(a, b)) / np.pi


def coords_to_dir(cx, cy):
    phi, theta = np.broadcast_arrays(np.pi * (np.asarray(cx) + 1), -np.pi * np.asarray(cy) / 2)
    return np.stack([np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi), np.sin(theta)], axis=-1)


def texel_centres(h, w):
    """directions of the texel centres of an h x w module map: cx_j = (j - 1/2) 2 / (w - 1) - 1, cy_i likewise (row 0 clamps to the pole)"""
    cx = (np.arange(w) - 0.5) * 2 / (w - 1) - 1
    cy = np.clip((np.arange(h) - 0.5) * 2 / (h - 1) - 1, -1, 1)
    return coords_to_dir(cx[None, :], cy[:, None])


def pano_directions(hp, wp):
    """pano2env.pixel_directions restated in float64: [hp, wp, 3]"""
    theta = (np.arange(hp) / (hp - 1) * np.pi - np.pi / 2)[:, None]
    phi = (-np.arange(wp) / (wp - 1) * 2 * np.pi - np.pi)[None, :]
    return np.stack([np.cos(phi) * np.cos(theta), np.sin(phi) * np.cos(theta), -np.sin(theta) + 0 * phi], axis=-1)


def module_source(h, w, R=None):
    """planar [3,h,w] LINEAR radiance at the texel centres (of the lighting rotated by R)"""
    d = texel_centres(h, w)
    return np.ascontiguousarray(np.moveaxis(radiance(d if R is None else d @ R), -1, 0))          # d @ R = rows (R^T d)^T


def pano_source(hp, wp):
    return radiance(pano_directions(hp, wp))


def lookup_bias(h, w):
    return (w - 1) * (h - 1) / (w * h)


def query_directions(R, h=H):
    """4000 default_rng(1) directions, those kept whose latitude coordinate is 0.15 clear of the pole rows for d and for R^T d"""
    d = np.random.default_rng(1).normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lim = 1 - 6 / h - 0.15
    keep = (np.abs(dir_to_coords(d)[1]) < lim) & (np.abs(dir_to_coords(d @ R)[1]) < lim)
    return d[keep]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def resample_np(src, kind, R, gain, S, h, w, dtype=np.float64):
    """csrc/envmap_resample.hip in numpy, IN THE KERNEL'S EXPRESSION ORDER, in `dtype` throughout: float64 is the definition, float32
    differs from the kernel by the transcendental functions only.  src: LINEAR radiance, planar [3,Hs,Ws] (kind 0) or interleaved
    [Hp,Wp,3] (kind 1).  -> the log map [3,h,w]"""
    f = dtype
    src = np.asarray(src, dtype=f)
    R = np.asarray(R, dtype=f)
    PI, TWO_PI = f(math.pi), f(2 * math.pi)
    hs, ws = src.shape[1:] if kind == 0 else src.shape[:2]
    sx, sy = f(2) / f(w - 1), f(2) / f(h - 1)
    hx, hy = f(ws - 1) * f(0.5), f(hs - 1) * f(0.5)
    im1 = (np.arange(h) - 1).astype(f)[:, None]
    jm1 = (np.arange(w) - 1).astype(f)[None, :]
    acc = np.zeros((3, h, w), dtype=f)
    for a in range(S):
        fa = (f(a) + f(0.5)) / f(S)
        cy = np.clip((im1 + fa) * sy - f(1), f(-1), f(1))
        th = (-PI * cy) * f(0.5)
        st, ct = np.sin(th), np.cos(th)
        for b in range(S):
            fb = (f(b) + f(0.5)) / f(S)
            cx = (jm1 + fb) * sx - f(1)
            ph = PI * (cx + f(1))
            sp, cp = np.sin(ph), np.cos(ph)
            d0, d1, d2 = ct * cp, ct * sp, st + f(0) * sp
            s0 = (R[0, 0] * d0 + R[1, 0] * d1) + R[2, 0] * d2
            s1 = (R[0, 1] * d0 + R[1, 1] * d1) + R[2, 1] * d2
            s2 = (R[0, 2] * d0 + R[1, 2] * d1) + R[2, 2] * d2
            phi = np.arctan2(s1, s0)
            m = np.where(phi < 0, phi + TWO_PI, phi)
            scx = (m - PI) / PI
            theta = np.arctan2(s2, np.sqrt(s0 * s0 + s1 * s1))
            scy = ((-theta) / PI) * f(2)
            if kind == 0:
                u = (scx + f(1)) * hx + f(0.5)
                v = (scy + f(1)) * hy + f(0.5)
                fu, fv = np.floor(u), np.floor(v)
                ju, iv = fu.astype(np.int64), fv.astype(np.int64)
                c0, c1 = np.mod(ju - 1, ws - 1) + 1, np.mod(ju, ws - 1) + 1
                r0, r1 = np.clip(iv, 1, hs - 1), np.clip(iv + 1, 1, hs - 1)
            else:
                u = (-scx * f(0.5)) * f(ws - 1)
                v = (scy + f(1)) * hy
                fu, fv = np.floor(u), np.floor(v)
                ju, iv = fu.astype(np.int64), fv.astype(np.int64)
                c0, c1 = np.mod(ju, ws - 1), np.mod(ju + 1, ws - 1)
                r0, r1 = np.clip(iv, 0, hs - 1), np.clip(iv + 1, 0, hs - 1)
            u, v = u - fu, v - fv
            e, s = f(1) - u, f(1) - v
            for c in range(3):
                p = src[c] if kind == 0 else src[:, :, c]
                acc[c] = acc[c] + (s * (e * p[r0, c0] + u * p[r0, c1]) + v * (e * p[r1, c0] + u * p[r1, c1]))
    val = (acc / f(S * S)) * f(gain)
    val = np.where(val >= f(1e-8), val, f(1e-8))          # fmaxf: a NaN becomes the floor
    out = np.log(val)
    assert out.dtype == f
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """every resampling the GPU test runs: name -> (src float32, kind, R, gain, S, h, w).  Sources are rounded to float32 first (what
    the kernel is handed), so the margins below hold no rounding of the input."""
    out = {}
    rots = rotations()
    mod = module_source(H, W).astype(np.float32)
    pano = pano_source(*PANO).astype(np.float32)
    for rn, R in rots.items():
        for S in (1, 4):
            out[f"module-{rn}-S{S}"] = (mod, 0, R, 1.0, S, H, W)
            out[f"pano-{rn}-S{S}"] = (pano, 1, R, 1.0 / lookup_bias(H, W), S, H, W)
    out["module-resize-axis-S4"] = (mod, 0, rots["axis"], lookup_bias(H, W) / lookup_bias(16, 32), 4, 16, 32)
    out["pano-odd-axis-S2"] = (pano_source(*PANO_ODD).astype(np.float32), 1, rots["axis"], 1.0 / lookup_bias(H, W), 2, H, W)
    out["module-yaw8-S1"] = (mod, 0, yaw_by_texels(8, W), 1.0, 1, H, W)
    return out


def yaw_by_texels(k, w):
    from nmf_amd import relight
    return relight.rotation(yaw=2 * math.pi * k / (w - 1), degrees=False)


@functools.lru_cache(maxsize=None)
def restatement(name):
    """the float64 definition of a case (computed once, shared by the CPU and GPU tests; callers must not write into it)"""
    src, kind, R, gain, S, h, w = cases()[name]
    out = resample_np(src, kind, R, gain, S, h, w, np.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restatement_margin():
    """the GPU tolerance in the log domain: 4 x the largest |numpy-fp32 restatement - float64| over rows 1..H-1 of every case (row 0
    is the exact pole, where the azimuth is undefined: it is compared by its mean).  fp32 in the kernel's expression order has the
    kernel's rounding of every coordinate; the factor covers its sincosf / atan2f / logf against numpy's."""
    worst = 0.0
    for name, (src, kind, R, gain, S, h, w) in cases().items():
        d = np.abs(resample_np(src, kind, R, gain, S, h, w, np.float32).astype(np.float64) - restatement(name))[:, 1:]
        worst = max(worst, float(d.max()))
    return 4 * worst


def oracle_lookup(bg_log, dirs, mipbias=0.0, brightness=0.0, mul=1.0):
    """oracle.nmf_oracle.env_lookup of the log map [3,h,w] (float64) along dirs at the sharpest footprint -> [n,3] numpy"""
    from oracle.nmf_oracle import env_lookup
    t = lambda v: torch.tensor(v, dtype=torch.float64)      # noqa: E731
    sd = {"bg_module.bg_mat": torch.as_tensor(np.array(bg_log, dtype=np.float64))[None], "bg_module.brightness": t(brightness),
          "bg_module.mul": t(mul), "bg_module.mipbias": t(mipbias)}
    dirs = torch.as_tensor(np.asarray(dirs, dtype=np.float64))
    return env_lookup(sd, dirs, torch.full((dirs.shape[0],), SA, dtype=torch.float64)).numpy()


def error_ratios(bg_log, R, lookup=oracle_lookup, target_bias=None):
    """(max, mean) of |lookup(map) - analytic x bias| over the query directions, relative to the same error of a map that HOLDS the
    analytic radiance of the rotated lighting at its texel centres (the best a map of this size can do)"""
    h, w = bg_log.shape[-2:]
    bias = lookup_bias(h, w)
    q = query_directions(R, h)
    want = radiance(q @ R)                                  # L'(d) = L(R^T d)
    got = lookup(bg_log, q)
    ideal = lookup(np.log(module_source(h, w, R)), q)
    e_got = np.abs(got - want * (bias if target_bias is None else target_bias))
    e_ideal = np.abs(ideal - want * bias)
    return e_got.max() / e_ideal.max(), e_got.mean() / e_ideal.mean(), len(q)


# ---- conventions against the oracle ------------------------------------------------------------------------------------------------
def test_direction_and_coordinate_conventions_round_trip():
    d = np.random.default_rng(3).normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cx, cy = dir_to_coords(d)
    assert np.abs(cx).max() <= 1 and np.abs(cy).max() <= 1
    assert np.abs(coords_to_dir(cx, cy) - d).max() < 1e-14
    # the panorama parameterisation is pano2env.pixel_directions'
    from nmf_amd import pano2env
    rows, cols = np.meshgrid(np.arange(PANO_ODD[0]), np.arange(PANO_ODD[1]), indexing="ij")
    t = pano2env.pixel_directions(torch.as_tensor(rows.reshape(-1), dtype=torch.float64),
                                  torch.as_tensor(cols.reshape(-1), dtype=torch.float64), *PANO_ODD).numpy()
    assert np.abs(t.reshape(*PANO_ODD, 3) - pano_directions(*PANO_ODD)).max() < 1e-14


def test_sharpest_lookup_at_texel_centres_returns_the_texel_times_the_bias():
    rng = np.random.default_rng(4)
    bg = rng.normal(size=(3, H, W)) * 0.5
    d = texel_centres(H, W)
    rows = [i for i in range(1, H) if abs((i - 0.5) * 2 / (H - 1) - 1) < 1 - 6 / H]          # off the pole rows
    got = oracle_lookup(bg, d[rows].reshape(-1, 3)).reshape(len(rows), W, 3)
    ratio = got[:, 1:] / np.exp(bg)[:, rows, 1:].transpose(1, 2, 0)
    print("centre-lookup ratio", ratio.min(), ratio.max())
    assert lookup_bias(H, W) == 0.95361328125
    assert np.abs(ratio - 0.95361328125).max() < 1e-11
    # half a texel to the side a lookup straddles two texels: no single ratio
    side = coords_to_dir(((np.arange(1, W) - 1.0) * 2 / (W - 1) - 1)[None, :], ((np.array(rows) - 0.5) * 2 / (H - 1) - 1)[:, None])
    r2 = oracle_lookup(bg, side.reshape(-1, 3)).reshape(len(rows), W - 1, 3) / np.exp(bg)[:, rows, 1:].transpose(1, 2, 0)
    assert np.abs(r2 - 0.95361328125).max() > 1e-2


def test_restatement_identity_and_yaw_equal_the_source_rows_and_a_roll():
    src = module_source(H, W)
    same = resample_np(src, 0, np.eye(3), 1.0, 1, H, W)
    err_id = np.abs(same[:, 1:] - np.log(src)[:, 1:]).max()
    # float64 rounds the source coordinate to ~W 2^-52 texels, times a texel contrast of order 1
    print("identity", err_id)
    assert err_id < 1e-12
    for k in (1, 8, 37):
        turned = resample_np(src, 0, yaw_by_texels(k, W), 1.0, 1, H, W)
        want = np.log(src).copy()
        want[:, :, 1:] = np.roll(want[:, :, 1:], k, axis=2)
        err = np.abs(turned[:, 1:, 1:] - want[:, 1:, 1:]).max()
        print("yaw", k, err)
        assert err < 1e-12
        assert np.abs(turned[:, 1:, 0] - turned[:, 1:, W - 1]).max() < 1e-12          # column 0 is column W-1 across the seam
    assert np.abs(restatement("module-yaw8-S1") - resample_np(cases()["module-yaw8-S1"][0], 0, yaw_by_texels(8, W), 1.0, 1, H, W)).max() == 0


def test_restatement_panorama_at_commensurate_sizes_picks_the_pixels_exactly():
    """Hp - 1 = 2 (H - 1), Wp - 1 = 2 (W - 1): a texel centre falls on pixel (2 i - 1, (W - 2 j) mod (Wp - 1)) exactly"""
    hp, wp = 2 * (H - 1) + 1, 2 * (W - 1) + 1
    pano = np.random.default_rng(5).uniform(0.1, 2.0, size=(hp, wp, 3))
    pano[:, -1] = pano[:, 0]
    got = resample_np(pano, 1, np.eye(3), 1.0, 1, H, W)
    i, j = np.arange(1, H), np.arange(W)
    want = np.log(pano[(2 * i - 1)[:, None], np.mod(W - 2 * j, wp - 1)[None, :]]).transpose(2, 0, 1)
    assert np.abs(got[:, 1:] - want).max() < 1e-11
    # and that pixel's direction IS the texel centre's
    pd = pano_directions(hp, wp)[(2 * i - 1)[:, None], np.mod(W - 2 * j, wp - 1)[None, :]]
    assert np.abs(pd - texel_centres(H, W)[1:]).max() < 1e-13


def test_restatement_floor_gain_nan_and_supersample_mean():
    src = module_source(H, W)
    assert np.abs(resample_np(src, 0, np.eye(3), 2.5, 1, H, W) - resample_np(src, 0, np.eye(3), 1.0, 1, H, W) - math.log(2.5)).max() < 1e-12
    bad = src.copy()
    bad[:, 5, 7] = np.nan
    bad[:, 9, 9] = 0.0
    out = resample_np(bad, 0, np.eye(3), 1.0, 1, H, W)
    assert np.isfinite(out).all() and out[0, 5, 7] == math.log(1e-8) and out[0, 9, 9] == math.log(1e-8)
    # a constant stays a constant whatever S, the rotation and the sizes
    for kind, s in ((0, np.full((3, 20, 33), 0.7)), (1, np.full((21, 47, 3), 0.7))):
        out = resample_np(s, kind, rotations()["axis"], 1.0, 3, 12, 24)
        assert np.abs(out - math.log(0.7)).max() < 1e-12


# ---- the resampled map against analytic radiance ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", ["identity", "yaw90", "x90", "axis"])
def test_resampled_maps_are_as_good_as_a_map_of_the_analytic_radiance(rot):
    R = rotations()[rot]
    mx, mean, n = error_ratios(restatement(f"module-{rot}-S4"), R)
    print("rotation", rot, "queries", n, "max ratio", mx, "mean ratio", mean)
    assert 2800 <= n <= 3500
    assert mx <= 1.5 and mean <= 1.25
    mx, mean, n = error_ratios(restatement(f"pano-{rot}-S4"), R, target_bias=1.0)      # gain 1 / bias: lookups return the radiance
    print("import", rot, "queries", n, "max ratio", mx, "mean ratio", mean)
    assert mx <= 1.5 and mean <= 1.25


def test_a_half_texel_convention_error_would_show():
    """the caps separate: the same resampling with the texel centres taken at ix = j fails both"""
    src = module_source(H, W)
    shifted = np.log(src)
    shifted[:, :, 1:] = 0.5 * (shifted[:, :, 1:] + np.roll(shifted[:, :, 1:], 1, axis=2))      # the map half a texel to the side
    mx, mean, _ = error_ratios(shifted, np.eye(3))
    print("half-texel shift", mx, mean)
    assert mx > 1.5 and mean > 1.25


# ---- the C ABI's argument checks (no GPU) ----------------------------------------------------------------------------------------
def _abi():
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    lib.nmf_version.restype = C.c_int
    return lib


def _call(lib, src=16, kind=0, hs=32, ws=64, R=None, gain=1.0, S=4, dst=32, h=32, w=64):
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731
    return lib.nmf_env_resample(p(src), C.c_int32(kind), C.c_int32(hs), C.c_int32(ws), *[C.c_float(v) for v in R.reshape(-1)],
                                C.c_float(gain), C.c_int32(S), p(dst), C.c_int32(h), C.c_int32(w), None)


def test_env_resample_arguments_are_checked_without_a_gpu():
    lib = _abi()
    assert lib.nmf_version() >= 121
    for kw in (dict(src=0), dict(dst=0)):
        assert _call(lib, **kw) == -1, kw
        assert b"nmf_env_resample" in lib.nmf_last_error_string() and b"null" in lib.nmf_last_error_string()
    for kw in (dict(hs=3), dict(ws=3), dict(h=3), dict(w=0), dict(h=-5)):
        assert _call(lib, **kw) == -1, kw
        assert b"size" in lib.nmf_last_error_string()
    for S in (0, 9, -1):
        assert _call(lib, S=S) == -2, S
        assert b"supersample" in lib.nmf_last_error_string()
    for kind in (2, -1):
        assert _call(lib, kind=kind) == -1, kind
        assert b"kind" in lib.nmf_last_error_string()
    for gain in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(lib, gain=gain) == -1, gain
        assert b"gain" in lib.nmf_last_error_string()
    skew = np.eye(3)
    skew[0, 1] = 3e-4
    nan = np.eye(3)
    nan[2, 2] = float("nan")
    for R in (2 * np.eye(3), skew, nan, np.zeros((3, 3))):
        assert _call(lib, R=R) == -1
        assert b"rotation" in lib.nmf_last_error_string()


def test_env_resample_has_no_cpu_path():
    from nmf_amd import hip
    with pytest.raises(hip.NmfHipError):
        hip.env_resample(torch.ones(3, 8, 16), hip.ENV_SRC_MODULE, np.eye(3), 1.0, 1, torch.zeros(3, 8, 16))


def test_rotation_helpers():
    from nmf_amd import relight
    for R in rotations().values():
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    assert np.abs(relight.rotation(yaw=90) @ [1, 0, 0] - [0, 1, 0]).max() < 1e-15          # +z up: a yaw turns x towards y
    assert np.abs(relight.rotation(pitch=90) @ [0, 0, 1] - [1, 0, 0]).max() < 1e-15
    assert np.abs(relight.rotation(roll=90) @ [0, 1, 0] - [0, 0, 1]).max() < 1e-15
    assert np.abs(relight.rotation(yaw=0.3, degrees=False) - relight.axis_angle((0, 0, 2), 0.3)).max() < 1e-15
    assert np.abs(relight.rotation(10, 20, 30) - relight.rotation(yaw=10) @ relight.rotation(pitch=20) @ relight.rotation(roll=30)).max() < 1e-15
    assert relight.lookup_bias(H, W) == lookup_bias(H, W)
    assert [relight.default_supersample(wp, 32) for wp in (64, 65, 192, 101, 4096)] == [1, 2, 3, 2, 8]


def test_restatement_margin_is_small_and_printed():
    m = restatement_margin()
    print("restatement margin (log domain)", m, "over", len(cases()), "cases")
    assert 0 < m < 1e-3
