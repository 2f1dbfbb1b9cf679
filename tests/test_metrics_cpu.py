"""Evaluation metrics without a GPU: float64 NumPy restatements of SSIM (utils.py:90-136) and of the per-view normal error
(renderer.py:369-389) pinned against tests/golden/metrics.npz and closed-form cases; the host side of nmf_ssim /
nmf_normal_err (workspace arithmetic, argument checks); BlenderDataset's normal maps (dataLoader/blender.py:236-247).
The restatements are imported by tests/test_hip_metrics.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics.npz")


# ---- restatements ------------------------------------------------------------------------------------------------------
def gauss_taps(filter_size=11, filter_sigma=1.5):
    """utils.py:101-106"""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f = np.exp(-0.5 * ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2)
    return f / f.sum()


def _filter_valid(z, f):
    """utils.py:109-114: separable valid-mode convolution of [H, W, C] (vertical, then horizontal; f is symmetric)"""
    k = len(f)
    H, W = z.shape[:2]
    v = sum(f[t] * z[t:H - k + 1 + t] for t in range(k))
    return sum(f[t] * v[:, t:W - k + 1 + t] for t in range(k))


def ssim_np(img0, img1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """utils.py:90-136 in float64: filtered moments, variances clamped at 0, covariance limited to
    sign * min(sqrt(s00 s11), |s01|), c1 = (k1 max)^2, c2 = (k2 max)^2, mean of the map over pixels and channels"""
    a, b = np.asarray(img0, np.float64), np.asarray(img1, np.float64)
    f = gauss_taps(filter_size, filter_sigma)
    mu0, mu1 = _filter_valid(a, f), _filter_valid(b, f)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = np.maximum(0.0, _filter_valid(a * a, f) - mu00)
    s11 = np.maximum(0.0, _filter_valid(b * b, f) - mu11)
    s01 = _filter_valid(a * b, f) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    m = (2 * mu01 + c1) * (2 * s01 + c2) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return m if return_map else float(m.mean())


def normal_err_np(pred, gt, acc, return_map=False):
    """renderer.py:369-389 in float64: quantise (n * 127 + 128 truncated toward zero, then (q - 128) / 127), renormalise with
    sqrt(sum + 1e-6), dot clipped to [1e-8, 1 - 1e-8], degrees, NaN -> 0 (a non-finite normal counts as NaN), times alpha;
    the view's value sum(err * acc) / sum(acc) (NaN when sum(acc) == 0)"""
    def quant(n):
        s = np.asarray(n, np.float64) * 127 + 128
        bad = ~np.isfinite(s).all(-1)
        q = np.trunc(np.where(np.isfinite(s), s, 128.0))
        return (q - 128) / 127, bad
    p, bp = quant(pred)
    g, bg = quant(gt)
    g = g / np.sqrt((g ** 2).sum(-1, keepdims=True) + 1e-6)
    p = p / np.sqrt((p ** 2).sum(-1, keepdims=True) + 1e-6)
    err = np.arccos(np.clip((p * g).sum(-1), 1e-8, 1 - 1e-8)) * 180 / np.pi
    err[np.isnan(err) | bp | bg] = 0
    acc = np.asarray(acc, np.float64)
    err = err * acc
    with np.errstate(invalid="ignore", divide="ignore"):
        val = err.sum() / acc.sum()
    return (val, err) if return_map else val


# ---- SSIM ----------------------------------------------------------------------------------------------------------------
def test_ssim_restatement_matches_the_reference_golden():
    z = np.load(GOLDEN)
    names = list(z["names"])
    assert {"rand_11x11", "quant8", "identical", "constant", "gt_outside"} <= set(names)
    for name in names:
        a, b = z[f"{name}_a"], z[f"{name}_b"]
        assert a.dtype == np.float32 and a.shape == b.shape
        assert abs(ssim_np(a, b, 1) - float(z[f"{name}_ssim"])) <= 1e-12, name
    mk = [k for k in z.files if k.startswith("map_")][0]
    name = mk[4:]
    m = ssim_np(z[f"{name}_a"], z[f"{name}_b"], 1, return_map=True)
    assert m.shape == z[mk].shape and np.abs(m - z[mk]).max() <= 1e-12
    assert float(z["identical_ssim"]) == pytest.approx(1.0, abs=1e-12)
    assert (z["gt_outside_b"] > 1).any() and (z["gt_outside_b"] < 0).any()


def test_ssim_constant_images_closed_form():
    """variances are 0: only the luminance term (2 mu0 mu1 + c1) / (mu0^2 + mu1^2 + c1) remains"""
    a, b = np.full((13, 15, 3), 0.5, np.float32), np.full((13, 15, 3), 0.3, np.float32)
    c1, y = 1e-4, float(np.float32(0.3))
    assert ssim_np(a, b) == pytest.approx((2 * 0.5 * y + c1) / (0.25 + y * y + c1), abs=1e-12)


def test_gauss_taps_match_the_binding():
    from nmf_amd import hip
    np.testing.assert_array_equal(gauss_taps(), hip.ssim_taps())
    assert gauss_taps().sum() == pytest.approx(1.0, abs=1e-15)


# ---- normal error ----------------------------------------------------------------------------------------------------------
def test_normal_err_closed_forms():
    z = np.array([[0.0, 0.0, 1.0]])
    one = np.ones(1)
    # equal unit normals: only the 1e-6 of the renormalisation separates the dot from 1
    assert normal_err_np(z, z, one) == pytest.approx(np.degrees(np.arccos(1 / (1 + 1e-6))), abs=1e-9)
    assert normal_err_np(z, z, one) < 0.1
    # perpendicular: the dot is 0 -> clipped to 1e-8 -> 90 degrees
    assert normal_err_np(np.array([[1.0, 0, 0]]), z, one) == pytest.approx(90.0, abs=1e-5)
    # opposite: the dot -1 is clipped to 1e-8 as well, so the error is capped near 90 degrees
    assert normal_err_np(-z, z, one) == pytest.approx(90.0, abs=1e-5)
    # zero alpha everywhere: 0 / 0
    assert np.isnan(normal_err_np(z, z, np.zeros(1)))
    # a NaN pixel counts as 0 error but its alpha stays in the denominator
    pred = np.array([[1.0, 0, 0], [np.nan, 0, 0]])
    gt = np.array([[0, 0, 1.0], [0, 0, 1.0]])
    v, m = normal_err_np(pred, gt, np.ones(2), return_map=True)
    assert m[1] == 0 and v == pytest.approx(m[0] / 2, abs=1e-12)


def test_normal_err_weights_by_alpha():
    rng = np.random.default_rng(0)
    p, g = rng.standard_normal((50, 3)), rng.standard_normal((50, 3))
    acc = rng.uniform(0, 1, 50)
    v, m = normal_err_np(p, g, acc, return_map=True)
    assert v == pytest.approx(m.sum() / acc.sum(), abs=1e-12) and 0 < v < 180


# ---- host side of the C ABI ---------------------------------------------------------------------------------------------
def _lib():
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    lib.nmf_ssim_workspace_bytes.restype = C.c_int64
    lib.nmf_normal_err_workspace_bytes.restype = C.c_int64
    return lib


def test_metrics_workspace_sizes_are_host_arithmetic():
    """one fp64 partial per 16 x 32 output tile of a view (SSIM); two per 4096 pixels of a view (normal error)"""
    lib = _lib()
    ss = lambda n, H, W, Cn=3: int(lib.nmf_ssim_workspace_bytes(C.c_int64(n), C.c_int32(H), C.c_int32(W), C.c_int32(Cn)))  # noqa: E731
    assert ss(1, 11, 11) == 8
    assert ss(8, 800, 800) == 8 * (-(-790 // 16)) * (-(-790 // 32)) * 8
    assert ss(3, 27, 43) == 3 * 2 * 2 * 8
    assert ss(0, 800, 800) == ss(1, 10, 800) == ss(1, 800, 800, 4) == 0
    ne = lambda n, P: int(lib.nmf_normal_err_workspace_bytes(C.c_int64(n), C.c_int64(P)))  # noqa: E731
    assert ne(1, 1) == 16 and ne(2, 4096) == 32 and ne(2, 4097) == 64 and ne(5, 640000) == 5 * 157 * 16
    assert ne(0, 100) == ne(3, 0) == 0


def test_metrics_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib()
    one = C.c_void_p(16)                                 # (never dereferenced: every call fails on its arguments)
    taps = (C.c_double * 11)()

    def ssim(n, H, W, Cn, tp=C.addressof(taps), ptr=one, ws=1 << 20):
        return lib.nmf_ssim(ptr, ptr, C.c_int64(n), C.c_int32(H), C.c_int32(W), C.c_int32(Cn), C.c_void_p(tp), C.c_double(1e-4),
                            C.c_double(9e-4), ptr, None, ptr, C.c_int64(ws), None)

    assert ssim(1, 10, 20, 3) < 0 and b"nmf_ssim" in lib.nmf_last_error_string()
    assert ssim(1, 20, 10, 3) < 0
    assert ssim(1, 20, 20, 4) < 0 and b"C must be 3" in lib.nmf_last_error_string()
    assert ssim(1, 20, 20, 3, tp=None) < 0
    assert ssim(1, 20, 20, 3, ptr=None) < 0 and b"null" in lib.nmf_last_error_string()
    assert ssim(-1, 20, 20, 3) < 0
    assert ssim(2, 100, 100, 3, ws=8) < 0 and b"workspace too small" in lib.nmf_last_error_string()
    assert ssim(0, 20, 20, 3, ptr=None, ws=0) == 0                               # nothing to do

    def nerr(n, P, ptr=one, ws=1 << 20):
        return lib.nmf_normal_err(ptr, ptr, ptr, C.c_int64(n), C.c_int64(P), ptr, None, ptr, C.c_int64(ws), None)

    assert nerr(1, 100, ptr=None) < 0 and b"nmf_normal_err" in lib.nmf_last_error_string()
    assert nerr(1, 0) < 0 and nerr(-2, 10) < 0
    assert nerr(3, 10000, ws=16) < 0 and b"workspace too small" in lib.nmf_last_error_string()
    assert nerr(0, 100, ptr=None, ws=0) == 0


def test_metric_wrappers_refuse_cpu_tensors():
    from nmf_amd import hip
    a = torch.rand(16, 16, 3)
    with pytest.raises(hip.NmfHipError):
        hip.ssim(a, a)
    with pytest.raises(hip.NmfHipError):
        hip.normal_err(a.reshape(-1, 3), a.reshape(-1, 3), torch.ones(256))


def test_rgb_ssim_refuses_unsupported_filter_sizes():
    from nmf_amd.utils import rgb_ssim
    a = np.zeros((16, 16, 3), np.float32)
    with pytest.raises(NotImplementedError):
        rgb_ssim(a, a, 1.0, filter_size=7)
    with pytest.raises(AssertionError):
        rgb_ssim(a[..., :2], a[..., :2], 1.0)


# ---- BlenderDataset normal maps ------------------------------------------------------------------------------------------
def _scene(tmp_path, normal_ext=None):
    from PIL import Image
    os.makedirs(tmp_path / "test", exist_ok=True)
    frames = []
    for i in range(3):
        Image.fromarray(np.full((6, 5, 4), 200, np.uint8), "RGBA").save(tmp_path / "test" / f"r_{i}.png")
        frames.append({"file_path": f"./test/r_{i}", "transform_matrix": np.eye(4).tolist()})
    meta = {"camera_angle_x": 0.69, "w": 5, "h": 6, "frames": frames}
    if normal_ext:
        meta["normal_ext"] = normal_ext
    json.dump(meta, open(tmp_path / "transforms_test.json", "w"))


def test_blender_get_normal_decodes_8bit_and_unit_maps(tmp_path):
    from PIL import Image
    from nmf_amd.dataLoader import BlenderDataset
    _scene(tmp_path)
    rng = np.random.default_rng(3)
    n8 = rng.integers(0, 256, size=(6, 5, 4), dtype=np.uint8)
    n8[0, 0, :3] = 128                                                  # (0, 0, 0): the eps clip keeps it finite
    Image.fromarray(n8, "RGBA").save(tmp_path / "test" / "r_0_normal.png")
    n01 = rng.integers(0, 2, size=(6, 5, 3), dtype=np.uint8)            # a map already in [0, 1]
    Image.fromarray(n01, "RGB").save(tmp_path / "test" / "r_2_normal.png")
    ds = BlenderDataset(str(tmp_path), split="test", is_stack=True)
    assert ds.normal_paths[1] == os.path.join(str(tmp_path), "./test/r_1_normal.png")
    assert [ds.has_normal(i) for i in range(3)] == [True, False, True]
    g = ds.get_normal(0)
    ref = (n8[..., :3].astype(np.float32) - 128) / 127
    ref = ref / np.maximum(np.linalg.norm(ref, axis=-1, keepdims=True), np.finfo(np.float32).eps)
    assert g.shape == (6, 5, 3) and g.dtype == torch.float32
    np.testing.assert_allclose(g.numpy(), ref, rtol=0, atol=1e-6)
    assert (g[0, 0] == 0).all()
    np.testing.assert_array_equal(ds.get_normal(2).numpy(), (n01.astype(np.float32) - 0.5) * 2)


def test_blender_normal_ext_from_the_meta(tmp_path):
    from nmf_amd.dataLoader import BlenderDataset
    _scene(tmp_path, normal_ext=".jpg")
    ds = BlenderDataset(str(tmp_path), split="test", is_stack=True)
    assert all(p.endswith("_normal.jpg") for p in ds.normal_paths) and not ds.has_normal(0)
    with pytest.raises(NotImplementedError):
        BlenderDataset(str(tmp_path), split="test", stack_norms=True)
