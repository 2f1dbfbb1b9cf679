"""Scene composition without a GPU (nmf_amd/compose.py, csrc/compose.hip): the placement algebra, the numpy
restatements of the three kernels that tests/test_hip_compose.py compares the GPU against, the argument checks of the three entry
points, and the command line's refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- numpy restatements, in the kernels' expression order ------------------------------------------------------------------------
def rays_place_np(rays, R, c, s, inverse, dtype=np.float32):
    """nmf_rays_place: one rounding per operation in `dtype`; R = I, c = 0, s = 1 copies the rows"""
    R = np.asarray(R, dtype=np.float64).astype(np.float32).astype(dtype)
    c = np.asarray(c, dtype=np.float64).astype(np.float32).astype(dtype)
    s = dtype(np.float32(s))
    x = np.asarray(rays).astype(dtype)
    if np.array_equal(R, np.eye(3)) and not c.any() and s == 1:
        return x.copy()
    o, d = x[:, :3], x[:, 3:]
    out = np.empty_like(x)
    if inverse:
        t = o - c[None]
        for i in range(3):
            out[:, i] = ((R[0, i] * t[:, 0] + R[1, i] * t[:, 1]) + R[2, i] * t[:, 2]) / s
            out[:, 3 + i] = (R[0, i] * d[:, 0] + R[1, i] * d[:, 1]) + R[2, i] * d[:, 2]
    else:
        for i in range(3):
            out[:, i] = s * ((R[i, 0] * o[:, 0] + R[i, 1] * o[:, 1]) + R[i, 2] * o[:, 2]) + c[i]
            out[:, 3 + i] = (R[i, 0] * d[:, 0] + R[i, 1] * d[:, 1]) + R[i, 2] * d[:, 2]
    return out


def rays_place_margin(rays, R, c, s, inverse):
    """the project's restatement margin: 4 x the largest |fp32 restatement - float64 result|"""
    a = rays_place_np(rays, R, c, s, inverse, np.float32).astype(np.float64)
    return 4 * float(np.abs(a - rays_place_np(rays, R, c, s, inverse, np.float64)).max())


def merge_rank_np(offsets, zs, scales, B):
    """nmf_merge_rank by its definition: per ray, np.lexsort((original index, part, world depth)) -> (dst per list, offsets_m)"""
    K = len(offsets)
    offsets_m = np.sum([np.asarray(o[: B + 1], dtype=np.int64) for o in offsets], axis=0)
    dst = [np.empty(len(z), dtype=np.int64) for z in zs]
    for r in range(B):
        part, idx, zw = [], [], []
        for k in range(K):
            a, b = int(offsets[k][r]), int(offsets[k][r + 1])
            part += [k] * (b - a)
            idx += list(range(a, b))
            zw += list(np.float32(scales[k]) * np.asarray(zs[k][a:b], dtype=np.float32))
        order = np.lexsort((np.asarray(idx, dtype=np.int64), np.asarray(part, dtype=np.int64), np.asarray(zw, dtype=np.float32)))
        for place, j in enumerate(order):
            dst[part[j]][idx[j]] = offsets_m[r] + place
    return dst, offsets_m


def rotate_rows_np(n, R, dtype=np.float32):
    R = np.asarray(R, dtype=np.float64).astype(np.float32).astype(dtype)
    n = np.asarray(n).astype(dtype)
    return np.stack([(R[c, 0] * n[:, 0] + R[c, 1] * n[:, 1]) + R[c, 2] * n[:, 2] for c in range(3)], axis=1)


def merge_scatter_np(out, dst, part, sigma, dist, z, normal, ray_id, inv, sigma_ratio, scale, R, row_base):
    """nmf_merge_scatter of one list into the dict of merged numpy arrays `out` (every key present is written)"""
    f = np.float32
    if "sigma" in out:
        out["sigma"][dst] = np.asarray(sigma, dtype=f) * f(sigma_ratio)
    if "dist" in out:
        out["dist"][dst] = dist
    if "z" in out:
        out["z"][dst] = f(scale) * np.asarray(z, dtype=f)
    if "normal" in out:
        out["normal"][dst] = rotate_rows_np(normal, R)
    if "ray_id" in out:
        out["ray_id"][dst] = ray_id
    if "part" in out:
        out["part"][dst] = part
    if "src" in out:
        out["src"][dst] = np.arange(len(dst), dtype=np.int32)
    if "inv" in out:
        inv = np.asarray(inv, dtype=np.int32)
        out["inv"][dst] = np.where(inv >= 0, inv + np.int32(row_base), -1)
    return out


# ---- placement ----------------------------------------------------------------------------------------------------------------------
def test_placement_algebra_float64():
    from nmf_amd.compose import Placement
    from nmf_amd.relight import rotation
    rng = np.random.default_rng(0)
    P = Placement((40.0, -17.0, 63.0), (1.2, -0.4, 0.3), 0.7)
    Q = Placement(rotation(-110.0, 5.0, 0.0), (0.0, 2.0, -1.0), 1.9)
    for A in (P, Q, P @ Q, Placement.identity()):
        I = A @ A.inverse()
        assert np.abs(I.R - np.eye(3)).max() <= 1e-12 and np.abs(I.t).max() <= 1e-12 and abs(I.s - 1) <= 1e-12
        x = rng.normal(size=(50, 3))
        assert np.abs(A.inverse().apply(A.apply(x)) - x).max() <= 1e-12
    x = rng.normal(size=(20, 3))
    assert np.abs((P @ Q).apply(x) - P.apply(Q.apply(x))).max() <= 1e-12
    assert np.abs(P.apply(x) - (0.7 * x @ rotation(40.0, -17.0, 63.0).T + np.array([1.2, -0.4, 0.3]))).max() <= 1e-12
    assert Placement.identity().is_identity() and not P.is_identity()


def test_placement_refuses_what_is_not_a_similarity():
    from nmf_amd.compose import Placement
    shear = np.eye(3)
    shear[0, 1] = 2e-4
    for bad in (dict(rotation=shear), dict(rotation=np.diag([1.0, 1.0, -1.0])), dict(rotation=np.eye(4)), dict(scale=0.0),
                dict(scale=-1.0), dict(scale=float("nan")), dict(translation=(0.0, 1.0)), dict(translation=(0.0, np.inf, 0.0))):
        with pytest.raises(ValueError):
            Placement(**bad)
    ok = np.eye(3)
    ok[0, 1] = 5e-5                                      # inside the 1e-4 bound of nmf_env_resample
    Placement(ok)


def test_from_spec():
    from nmf_amd.compose import Placement
    from nmf_amd.relight import rotation
    P = Placement.from_spec("t=1.2,0,0;r=40,0,0;s=0.7")
    assert np.array_equal(P.t, [1.2, 0, 0]) and P.s == 0.7 and np.array_equal(P.R, rotation(40.0, 0.0, 0.0))
    Q = Placement.from_spec(" s=0.7 ; r=40,0,0 ;t=1.2,0,0;")                 # any order, blanks, a trailing separator
    assert np.array_equal(P.R, Q.R) and np.array_equal(P.t, Q.t) and P.s == Q.s
    assert Placement.from_spec("").is_identity() and Placement.from_spec("s=2").s == 2.0
    assert np.array_equal(Placement.from_spec("t=0,0,-3").t, [0, 0, -3])
    for text, field in (("q=1", "q"), ("t=1,2", "'t'"), ("r=1,2,3,4", "'r'"), ("s=0", "'s'"), ("s=-2", "'s'"), ("s=1,2", "'s'"),
                        ("r=a,b,c", "'r'"), ("t=1,2,nan", "'t'"), ("s=1;s=2", "'s'"), ("t", "t")):
        with pytest.raises(ValueError) as e:
            Placement.from_spec(text)
        assert field in str(e.value), (text, str(e.value))


# ---- restatements against their definitions -----------------------------------------------------------------------------------------
def test_rays_place_restatement():
    from nmf_amd.compose import Placement
    rng = np.random.default_rng(1)
    rays = rng.normal(size=(64, 6)).astype(np.float32)
    P = Placement((33.0, 12.0, -70.0), (0.5, -0.25, 0.125), 0.6)
    for inv in (0, 1):
        a = rays_place_np(rays, P.R, P.t, P.s, inv, np.float64)
        A = P.inverse() if inv else P
        Rf = P.R.astype(np.float32).astype(np.float64)                         # (the kernel's R is the float32 one)
        assert np.abs(a[:, 3:] - rays[:, 3:].astype(np.float64) @ (Rf if inv else Rf.T)).max() <= 1e-12
        assert np.abs(a[:, :3] - A.apply(rays[:, :3])).max() <= 2e-6
        assert rays_place_margin(rays, P.R, P.t, P.s, inv) <= 4e-6
        ident = rays_place_np(rays, np.eye(3), np.zeros(3), 1.0, inv)
        assert ident.tobytes() == rays.tobytes()
    # there and back
    back = rays_place_np(rays_place_np(rays, P.R, P.t, P.s, 1, np.float64), P.R, P.t, P.s, 0, np.float64)
    assert np.abs(back - rays).max() <= 1e-6


def test_merge_rank_restatement_is_the_stable_merge():
    offsets = [np.array([0, 2, 2, 4]), np.array([0, 1, 1, 3])]
    zs = [np.array([1.0, 2.0, 0.5, 0.5], np.float32), np.array([1.0, 1.0, 0.125], np.float32)]
    dst, off_m = merge_rank_np(offsets, zs, [1.0, 2.0], 3)
    assert off_m.tolist() == [0, 3, 3, 7]
    # ray 0: world depths list 0 = (1, 2), list 1 = (2): the tie at 2 goes to the lower list; ray 2: (.5, .5) and (2, .25)
    assert dst[0].tolist() == [0, 1, 4, 5] and dst[1].tolist() == [2, 6, 3]
    assert sorted(np.concatenate(dst).tolist()) == list(range(7))


# ---- the entry points' argument checks (no GPU: nothing is launched) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    for name in ("nmf_rays_place", "nmf_merge_rank", "nmf_merge_scatter"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = getattr(hip._lib, name).argtypes, C.c_int
    return lib


EINVAL, ERANGE = -1, -2
ONE = C.c_void_p(16)            # (never dereferenced: the calls fail on their arguments)


def test_abi_version_is_unchanged():
    from nmf_amd import hip
    assert hip.version() == 125
    assert {"nmf_rays_place", "nmf_merge_rank", "nmf_merge_scatter"} <= set(hip.EXPORTS)


def test_rays_place_refuses_bad_arguments(lib):
    I = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    sheared = (C.c_float * 9)(1, 2e-4, 0, 0, 1, 0, 0, 0, 1)
    zero = (C.c_float * 3)(0, 0, 0)
    nan3 = (C.c_float * 3)(0, float("nan"), 0)
    call = lib.nmf_rays_place
    assert call(None, I, zero, 1.0, 1, 4, ONE, None) == EINVAL and b"nmf_rays_place" in lib.nmf_last_error_string()
    assert call(ONE, I, zero, 1.0, 1, 4, None, None) == EINVAL
    assert call(ONE, None, zero, 1.0, 1, 4, ONE, None) == EINVAL
    assert call(ONE, I, None, 1.0, 1, 4, ONE, None) == EINVAL
    assert call(ONE, I, zero, 0.0, 1, 4, ONE, None) == EINVAL and b"s must be" in lib.nmf_last_error_string()
    assert call(ONE, I, zero, -1.0, 0, 4, ONE, None) == EINVAL
    assert call(ONE, I, zero, float("inf"), 0, 4, ONE, None) == EINVAL
    assert call(ONE, I, zero, float("nan"), 0, 4, ONE, None) == EINVAL
    assert call(ONE, I, nan3, 1.0, 0, 4, ONE, None) == EINVAL
    assert call(ONE, sheared, zero, 1.0, 0, 4, ONE, None) == EINVAL and b"not a rotation" in lib.nmf_last_error_string()
    assert call(ONE, I, zero, 1.0, 2, 4, ONE, None) == EINVAL
    assert call(ONE, I, zero, 1.0, 0, -1, ONE, None) == EINVAL
    assert call(None, I, zero, 1.0, 0, 0, None, None) == 0                      # no rays: fine, nothing launched


def test_merge_rank_refuses_bad_arguments(lib):
    from nmf_amd import hip
    L = hip.MergeLists()
    for k in range(8):
        L.offsets[k], L.z[k], L.dst[k], L.scale[k], L.M[k] = 16, 16, 16, 1.0, 5
    call = lib.nmf_merge_rank
    assert call(0, C.byref(L), 4, ONE, None) == ERANGE and b"nmf_merge_rank" in lib.nmf_last_error_string()
    assert call(9, C.byref(L), 4, ONE, None) == ERANGE
    assert call(-1, C.byref(L), 4, ONE, None) == ERANGE
    assert call(2, None, 4, ONE, None) == EINVAL
    assert call(2, C.byref(L), 4, None, None) == EINVAL
    assert call(2, C.byref(L), -1, ONE, None) == EINVAL
    for field in ("offsets", "z", "dst"):
        B = hip.MergeLists.from_buffer_copy(L)
        getattr(B, field)[1] = None
        assert call(2, C.byref(B), 4, ONE, None) == EINVAL, field
    B = hip.MergeLists.from_buffer_copy(L)
    B.z[1], B.dst[1], B.M[1] = None, None, 0                                    # an empty list needs neither
    B.scale[0] = 0.0
    assert call(2, C.byref(B), 4, ONE, None) == EINVAL and b"scale" in lib.nmf_last_error_string()
    B.scale[0], B.M[0] = 1.0, -3
    assert call(2, C.byref(B), 4, ONE, None) == EINVAL
    B.M[0] = 5
    assert call(2, C.byref(B), 0, ONE, None) == EINVAL                           # samples without rays


def test_merge_scatter_refuses_bad_arguments(lib):
    I = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    sheared = (C.c_float * 9)(1, 2e-4, 0, 0, 1, 0, 0, 0, 1)

    def call(M_k=4, M_total=8, dst=ONE, sigma=ONE, dist=ONE, z=ONE, normal=ONE, ray_id=ONE, inv=ONE, ratio=1.0, scale=1.0, R=I, part=0,
             row_base=0, outs=(ONE,) * 8):
        return lib.nmf_merge_scatter(M_k, M_total, dst, sigma, dist, z, normal, ray_id, inv, ratio, scale, R, part, row_base, *outs, None)

    assert call(M_k=-1) == EINVAL and b"nmf_merge_scatter" in lib.nmf_last_error_string()
    assert call(M_total=3) == EINVAL
    assert call(dst=None) == EINVAL
    assert call(part=8) == ERANGE and call(part=-1) == ERANGE
    assert call(row_base=-1) == ERANGE and call(row_base=2 ** 31) == ERANGE
    assert call(ratio=0.0) == EINVAL and call(scale=float("nan")) == EINVAL and call(scale=-2.0) == EINVAL
    assert call(R=sheared) == EINVAL and b"not a rotation" in lib.nmf_last_error_string()
    assert call(R=None) == EINVAL
    for name in ("sigma", "dist", "z", "normal", "ray_id", "inv"):
        assert call(**{name: None}) == EINVAL, name
        assert b"without its input" in lib.nmf_last_error_string()
    assert call(M_k=0, dst=None) == 0                                            # an empty list: fine, nothing launched


def test_wrappers_have_no_cpu_path():
    import torch
    from nmf_amd import hip
    with pytest.raises(hip.NmfHipError):
        hip.rays_place(torch.zeros(4, 6), np.eye(3), np.zeros(3), 1.0)
    with pytest.raises(hip.NmfHipError):
        hip.rays_place(torch.zeros(4, 5), np.eye(3), np.zeros(3), 1.0)
    with pytest.raises(hip.NmfHipError):
        hip.merge_rank([torch.zeros(5, dtype=torch.int64)], [torch.zeros(3)], [1.0], 4)


# ---- command line -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,flag", [(["--eval-dir", "x", "--datadir", "d"], "--eval-dir"),
                                         (["--relight-eval", "x", "--datadir", "d"], "--relight-eval"),
                                         (["--material-maps"], "--material-maps"), (["--edit", "roughness*0.4"], "--edit"),
                                         (["--edit-file", "edits.yaml"], "--edit")])
def test_render_refuses_insert_with_unsupported_flags(extra, flag, capsys):
    from nmf_amd import render
    for composed in (["--insert", "b.th@s=0.5"], ["--place", "t=1,0,0"]):
        with pytest.raises(SystemExit) as e:
            render.main(["--ckpt", "a.th"] + composed + extra)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert f"error: {flag} is not built for a composed scene" in err, err


def test_render_refuses_malformed_placements(capsys):
    from nmf_amd import render
    for argv, what in ((["--insert", "b.th@s=0"], "'s'"), (["--insert", "b.th@t=1,2"], "'t'"), (["--place", "w=3"], "w=3"),
                       (["--insert", "@s=2"], "no checkpoint"), (["--insert", "b.th"] * 8, "at most 8")):
        with pytest.raises(SystemExit) as e:
            render.main(["--ckpt", "a.th"] + argv)
        assert e.value.code == 2
        assert what in capsys.readouterr().err
