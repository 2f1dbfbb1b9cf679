"""Camera paths without a GPU: the path builders of nmf_amd/camera_path.py (orthonormal frames, the orbit's geometry, interpolation
through its keys, the transforms-file round trip, a data set's render_path), the numpy fp32 restatements of the two kernels of
csrc/camera.hip that tests/test_hip_camera_path.py compares bit for bit (camera_rays_np against float64 and against the loader's
construction, frame_finish_np), the refusals of both entry points and the depth colour table."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from nmf_amd import camera_path as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the restatements the GPU tests use --------------------------------------------------------------------------------------------
def camera_rays_np(c2w, fx, fy, cx, cy, H, W, dtype=np.float32):
    """nmf_camera_rays in the kernel's order, one rounding per operation in `dtype`, from the fp32 values the call passes
    -> [H W, 6] (origin | direction)"""
    T = dtype
    m = np.asarray(c2w, dtype=np.float32).astype(T)
    fx, fy, cx, cy = (T(F(v)) for v in (fx, fy, cx, cy))
    col = np.broadcast_to(np.arange(W, dtype=T)[None, :], (H, W))
    row = np.broadcast_to(np.arange(H, dtype=T)[:, None], (H, W))
    x = ((col + T(0.5)) - cx) / fx
    y = ((row + T(0.5)) - cy) / fy
    n = np.sqrt((x * x + y * y) + T(1))
    dx, dy, dz = x / n, y / n, T(1) / n
    world = [(m[i, 0] * dx + m[i, 1] * dy) + m[i, 2] * dz for i in range(3)]
    origin = [np.full((H, W), m[i, 3], dtype=T) for i in range(3)]
    out = np.stack(origin + world, -1).reshape(H * W, 6)
    assert out.dtype == T
    return out


def quantise_np(kind, v, near=0.0, far=1.0, lut=None):
    """one panel of nmf_frame_finish in fp32: v [H, W, 3] (rgb, normal) or [H, W] (depth, acc) -> uint8 [H, W, 3]"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(v, dtype=F)
        v = np.where(np.isnan(v), F(0), v)
        if kind == "rgb":
            return (np.clip(v, F(0), F(1)) * F(255)).astype(np.uint8)
        if kind == "normal":
            return np.clip(v * F(127) + F(128), F(0), F(255)).astype(np.uint8)
        if kind == "acc":
            q = (F(255) * np.clip(v, F(0), F(1))).astype(np.uint8)
            return np.repeat(q[..., None], 3, -1)
        t = np.clip((v - F(near)) / ((F(far) - F(near)) + F(1e-8)), F(0), F(1))
        q = (F(255) * t).astype(np.uint8)
        return np.repeat(q[..., None], 3, -1) if lut is None else np.asarray(lut)[q]


def frame_finish_np(H, W, rgb=None, depth=None, normal=None, acc=None, near=0.0, far=1.0, lut=None):
    """nmf_frame_finish: the non-null panels side by side -> uint8 [H, n_panels W, 3]"""
    panels = []
    for kind, v, c in (("rgb", rgb, 3), ("depth", depth, 1), ("normal", normal, 3), ("acc", acc, 1)):
        if v is not None:
            panels.append(quantise_np(kind, np.asarray(v).reshape((H, W, 3) if c == 3 else (H, W)), near, far, lut))
    return np.concatenate(panels, 1)


def random_pose(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, rng.uniform(-5, 5, size=3)
    return m.astype(np.float32)


def random_cameras(n, seed):
    """(c2w, fx, fy, cx, cy, H, W): focal lengths 20..1200 (fx != fy), sizes 1..70, principal points off centre by up to 3 pixels"""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        H, W = int(rng.integers(1, 71)), int(rng.integers(1, 71))
        fx, fy = (float(F(v)) for v in rng.uniform(20, 1200, size=2))
        cx, cy = float(F(W / 2 + rng.uniform(-3, 3))), float(F(H / 2 + rng.uniform(-3, 3)))
        yield random_pose(rng), fx, fy, cx, cy, H, W


def test_ray_restatement_against_float64_and_the_loader():
    """Bounds (not fitted to the code): every component within 2^-20 of float64 and of the loader's route
    get_rays(normalised get_ray_directions, c2w); |d| within 2^-21 of 1.  The chain rounds ~12 times on values of size <= 1.75
    before the division by n, first-order worst case about 15 units of 2^-24 = 0.94 * 2^-20."""
    from nmf_amd.dataLoader.blender import get_ray_directions, get_rays
    worst = [0.0, 0.0, 0.0]
    for c2w, fx, fy, cx, cy, H, W in random_cameras(100, seed=3):
        got = camera_rays_np(c2w, fx, fy, cx, cy, H, W)
        ref = camera_rays_np(c2w, fx, fy, cx, cy, H, W, dtype=np.float64)
        assert np.array_equal(got[:, :3], np.broadcast_to(c2w[:3, 3], (H * W, 3)))
        d = get_ray_directions(H, W, [fx, fy], center=[cx, cy])
        d = d / torch.norm(d, dim=-1, keepdim=True)
        o_t, d_t = get_rays(d, torch.from_numpy(c2w))
        worst[0] = max(worst[0], np.abs(got[:, 3:].astype(np.float64) - ref[:, 3:]).max())
        worst[1] = max(worst[1], np.abs(got[:, 3:] - d_t.numpy()).max())
        worst[2] = max(worst[2], np.abs(np.linalg.norm(got[:, 3:].astype(np.float64), axis=-1) - 1).max())
        assert np.array_equal(o_t.numpy(), got[:, :3])
    print("units of 2^-24: float64", worst[0] * 2 ** 24, "loader", worst[1] * 2 ** 24, "unit length", worst[2] * 2 ** 24)
    assert worst[0] <= 2.0 ** -20 and worst[1] <= 2.0 ** -20 and worst[2] <= 2.0 ** -21


def test_frame_restatement_on_values_with_known_bytes():
    lut = np.arange(768, dtype=np.uint8).reshape(256, 3)
    v = np.array([[np.nan, -np.inf, -0.5, 0.0, 0.5, 1.0, 1.5, np.inf, 254 / 255, 1 / 255]], dtype=F)
    assert quantise_np("acc", v)[0, :, 0].tolist() == [0, 0, 0, 0, 127, 255, 255, 255, 254, 1]
    assert quantise_np("rgb", np.repeat(v[..., None], 3, -1))[0, :, 1].tolist() == [0, 0, 0, 0, 127, 255, 255, 255, 254, 1]
    assert quantise_np("normal", np.repeat(v[..., None], 3, -1))[0, :, 2].tolist() == [128, 0, 64, 128, 191, 255, 255, 255, 254, 128]
    d = np.array([[np.nan, 1.0, 2.0, 4.0, 6.0, 9.0, np.inf, -np.inf]], dtype=F)
    assert quantise_np("depth", d, 2.0, 6.0)[0, :, 0].tolist() == [0, 0, 0, 127, 255, 255, 255, 0]
    assert np.array_equal(quantise_np("depth", d, 2.0, 6.0, lut)[0, 3], lut[127])
    strip = frame_finish_np(1, 10, rgb=np.repeat(v[..., None], 3, -1), acc=v)
    assert strip.shape == (1, 20, 3) and strip[0, 14].tolist() == [127, 127, 127]


# ---- paths -------------------------------------------------------------------------------------------------------------------------
def _check_frames(c2ws):
    assert c2ws.dtype == np.float32 and c2ws.shape[1:] == (4, 4)
    R = c2ws[:, :3, :3].astype(np.float64)
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-6
    assert (np.linalg.det(R) > 0).all()
    assert np.array_equal(c2ws[:, 3], np.broadcast_to(np.array([0, 0, 0, 1], dtype=np.float32), (c2ws.shape[0], 4)))


def test_look_at_axes_and_refusal():
    m = cp.look_at((4.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    assert np.allclose(m[:3, 2], [-1, 0, 0]) and np.allclose(m[:3, 1], [0, 0, -1]) and np.allclose(m[:3, 0], [0, 1, 0])   # f, down, right
    assert np.allclose(m[:3, 3], [4, 0, 0]) and np.linalg.det(m[:3, :3]) == pytest.approx(1.0)
    with pytest.raises(ValueError):
        cp.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        cp.look_at((1.0, 2.0, 3.0), (1.0, 2.0, -1.0), up=(0, 0, 2.0))


def test_orbit_geometry():
    n, center, radius, elev = 24, np.array([0.3, -0.2, 0.1]), 4.0, 30.0
    c2ws = cp.orbit(n, center, radius, elev, start_deg=10.0)
    _check_frames(c2ws)
    assert c2ws.shape == (n, 4, 4)
    eye, fwd = c2ws[:, :3, 3].astype(np.float64), c2ws[:, :3, 2].astype(np.float64)
    rel = center - eye
    miss = np.linalg.norm(rel - (rel * fwd).sum(-1, keepdims=True) * fwd, axis=-1)          # the forward axis passes through center
    assert miss.max() <= 1e-5 * radius
    dist = np.linalg.norm(rel, axis=-1)
    assert np.abs(dist - radius).max() <= 1e-5 * radius
    assert np.abs(np.degrees(np.arcsin(-rel[:, 2] / dist)) - elev).max() <= 1e-4
    az = np.degrees(np.arctan2(-rel[:, 1], -rel[:, 0]))
    step = np.mod(np.diff(np.concatenate([az, az[:1]])), 360.0)
    assert np.abs(step - 360.0 / n).max() <= 1e-4 and abs(az[0] - 10.0) <= 1e-4


def test_spiral_is_closed_and_orthonormal():
    n = 40
    c2ws = cp.spiral(n, (0, 0, 0), 4.0, (10.0, 50.0), turns=2, radius_scale=(0.8, 1.2))
    _check_frames(c2ws)
    rel = c2ws[:, :3, 3].astype(np.float64)
    dist = np.linalg.norm(rel, axis=-1)
    elev = np.degrees(np.arcsin(rel[:, 2] / dist))
    assert dist.min() >= 3.2 - 1e-5 and dist.max() <= 4.8 + 1e-5 and elev.min() >= 10 - 1e-4 and elev.max() <= 50 + 1e-4
    assert dist[n // 4] == pytest.approx(4.8, abs=1e-5) and elev[3 * n // 4] == pytest.approx(10.0, abs=1e-4)
    assert dist[0] == pytest.approx(4.0, abs=1e-5) and elev[0] == pytest.approx(30.0, abs=1e-4)          # k = n would be k = 0 again
    az = np.degrees(np.arctan2(rel[:, 1], rel[:, 0]))
    assert np.mod(az[1] - az[0], 360.0) == pytest.approx(360.0 * 2 / n, abs=1e-4)


@pytest.mark.parametrize("closed", [True, False])
def test_interpolate_passes_through_its_keys(closed):
    rng = np.random.default_rng(7)
    K = 5
    keys = np.stack([random_pose(rng) for _ in range(K)])
    c2ws = cp.interpolate(keys, 4 * K if closed else 4 * (K - 1) + 1, closed=closed)
    _check_frames(c2ws)
    for i in range(K):
        assert np.abs(c2ws[4 * i, :3, 3] - keys[i, :3, 3]).max() <= 1e-6
        assert np.abs(c2ws[4 * i, :3, :3] - keys[i, :3, :3]).max() <= 1e-6
    # between two keys the rotation stays on the shorter arc: the angle to either key is below the angle between them
    ang = lambda A, B: np.degrees(np.arccos(np.clip((np.trace(A.T.astype(np.float64) @ B) - 1) / 2, -1, 1)))       # noqa: E731
    for i in range(K - 1):
        full = ang(keys[i, :3, :3], keys[i + 1, :3, :3])
        assert ang(keys[i, :3, :3], c2ws[4 * i + 2, :3, :3]) == pytest.approx(full / 2, abs=1e-3)


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def toy_scene(root, views=5, res=8, radius=4.0, elev_deg=25.0):
    """a test split in the format tools/make_blender_scene.py writes, with its cameras (look_at_blender) on the circle of one radius and
    elevation, and noise for frames: the poses are what is under test"""
    from PIL import Image
    look_at = _load_tool("make_blender_scene").look_at_blender
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "test"), exist_ok=True)
    frames = []
    for i in range(views):
        az, el = 2 * np.pi * (i + 0.3) / views, np.radians(elev_deg)
        eye = radius * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        Image.fromarray(rng.integers(0, 256, size=(res, res, 4), dtype=np.uint8), "RGBA").save(os.path.join(root, "test", f"r_{i}.png"))
        frames.append({"file_path": f"./test/r_{i}", "transform_matrix": look_at(eye).tolist()})
    with open(os.path.join(root, "transforms_test.json"), "w") as f:
        json.dump({"camera_angle_x": 0.6911112070083618, "w": res, "h": res, "frames": frames}, f)
    return root


def test_from_dataset_and_render_path(tmp_path):
    from nmf_amd.dataLoader import BlenderDataset
    scene = toy_scene(str(tmp_path / "toy"), views=5, radius=4.0, elev_deg=25.0)
    ds = BlenderDataset(scene, split="test", is_stack=True, N_vis=-1)
    center, radius, elev = cp.dataset_orbit(ds)
    assert np.abs(center).max() == 0 and radius == pytest.approx(4.0, abs=1e-5) and np.abs(elev - 25.0).max() <= 1e-4
    c2ws = cp.from_dataset(ds, "orbit", 12)
    _check_frames(c2ws)
    rel = c2ws[:, :3, 3].astype(np.float64)
    assert np.abs(np.linalg.norm(rel, axis=-1) - 4.0).max() <= 1e-5
    assert np.abs(np.degrees(np.arcsin(rel[:, 2] / 4.0)) - 25.0).max() <= 1e-3
    # a data set's own poses are OpenCV frames of look_at: the same axes as this module's
    assert np.abs(cp.look_at(ds.poses[0, :3, 3].numpy(), (0, 0, 0))[:3, :3] - ds.poses[0, :3, :3].numpy()).max() <= 1e-6
    _check_frames(cp.from_dataset(ds, "spiral", 9))
    interp = cp.from_dataset(ds, "interp", 20)                       # 5 poses: all of them are keys
    _check_frames(interp)
    assert np.abs(interp[4] - ds.poses[1].numpy()).max() <= 1e-6
    with pytest.raises(ValueError):
        cp.from_dataset(ds, "zigzag", 4)
    # load_path is the loader's arithmetic
    assert np.array_equal(cp.load_path(os.path.join(scene, "transforms_test.json")), ds.poses.numpy())
    assert ds.render_path.shape == (120, 4, 4) and ds.render_path is ds.render_path
    assert np.array_equal(ds.render_path, cp.from_dataset(ds, "orbit", 120))
    cam = cp.dataset_camera(ds)
    assert cam["w"] == cam["h"] == 8 and cam["fx"] == ds.fx and cam["cx"] == 4.0 and cam["near_far"] == [2.0, 6.0]


def test_path_file_round_trip(tmp_path):
    c2ws = cp.spiral(7, (0.1, 0.2, 0.3), 3.0, (5.0, 60.0))
    file = cp.save_path(str(tmp_path / "transforms_path.json"), c2ws, 0.69, 32, 24, (2.5, 7.0))
    assert np.array_equal(cp.load_path(file), c2ws)
    meta = json.load(open(file))
    assert set(meta) == {"camera_angle_x", "w", "h", "near_far", "frames"} and meta["frames"][3]["file_path"] == "./path/r_3"
    assert meta["near_far"] == [2.5, 7.0] and (meta["w"], meta["h"]) == (32, 24)
    # Blender convention: the camera looks down -z with +y up
    b = np.array(meta["frames"][0]["transform_matrix"])
    assert np.allclose(b[:3, 2], -c2ws[0, :3, 2]) and np.allclose(b[:3, 1], -c2ws[0, :3, 1]) and np.allclose(b[:3, 0], c2ws[0, :3, 0])
    poses, cam = cp.load_path(file, with_camera=True)
    assert cam["w"] == 32 and cam["h"] == 24 and cam["fx"] == cam["fy"] == pytest.approx(16 / np.tan(0.345)) and cam["cx"] == 16.0
    file = cp.save_path(str(tmp_path / "b.json"), c2ws, 0.69, 32, 24, (2.5, 7.0), intrinsics=(41.5, 40.25, 15.0, 13.5))
    poses, cam = cp.load_path(file, with_camera=True)
    assert np.array_equal(poses, c2ws) and (cam["fx"], cam["fy"], cam["cx"], cam["cy"]) == (41.5, 40.25, 15.0, 13.5)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
POSE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.5, 0.25, 2.0]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    f = C.c_float
    lib.nmf_camera_rays.argtypes = [f] * 16 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.nmf_frame_finish.argtypes = [C.c_void_p] * 4 + [f, f, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    return lib, hip


def test_symbols_are_declared_exported_and_bound():
    lib, hip = _lib()
    hdr = open(os.path.join(ROOT, "include", "nmf_hip.h")).read()
    for name in ("nmf_camera_rays", "nmf_frame_finish"):
        assert f"int {name}(" in hdr and hasattr(lib, name) and name in hip.EXPORTS
    assert hip.version() >= 124 and "#define NMF_ABI_VERSION %d" % hip.version() in hdr


def test_camera_rays_refusals_name_the_function():
    """every refusal with NULL device pointers: nothing can be launched, and the argument checks come before the pointer's"""
    lib, _ = _lib()
    inf, nan = float("inf"), float("nan")
    call = lambda pose=POSE, fx=100.0, fy=90.0, cx=3.0, cy=4.0, H=5, W=7: lib.nmf_camera_rays(*pose, fx, fy, cx, cy, H, W, None, None)  # noqa: E731
    cases = [(dict(), -1, b"null pointer"), (dict(H=0), -1, b"below 1"), (dict(W=-3), -1, b"below 1"),
             (dict(fx=0.0), -1, b"fx and fy"), (dict(fy=inf), -1, b"fx and fy"), (dict(fx=nan), -1, b"fx and fy"),
             (dict(cx=nan), -1, b"finite"), (dict(cy=-inf), -1, b"finite"),
             (dict(H=46341, W=46341), -2, b"2^31 - 1")]
    for k in range(12):
        cases.append((dict(pose=POSE[:k] + [nan if k % 2 else inf] + POSE[k + 1:]), -1, b"finite"))
    for kw, code, word in cases:
        assert call(**kw) == code, kw
        msg = lib.nmf_last_error_string()
        assert b"nmf_camera_rays" in msg and word in msg, (kw, msg)


def test_frame_finish_refusals_name_the_function():
    lib, _ = _lib()
    inf, nan = float("inf"), float("nan")
    call = lambda near=2.0, far=6.0, H=5, W=7: lib.nmf_frame_finish(None, None, None, None, near, far, None, H, W, None, None)  # noqa: E731
    for kw, word in [(dict(), b"all four"), (dict(H=0), b"below 1"), (dict(W=0), b"below 1"), (dict(near=nan), b"finite"),
                     (dict(far=inf), b"finite"), (dict(far=2.0), b"above near"), (dict(near=7.0), b"above near")]:
        assert call(**kw) == -1, kw
        msg = lib.nmf_last_error_string()
        assert b"nmf_frame_finish" in msg and word in msg, (kw, msg)


def test_wrappers_refuse_host_tensors():
    _, hip = _lib()
    with pytest.raises(hip.NmfHipError):
        hip.camera_rays(np.eye(4), 100.0, 100.0, 4.0, 4.0, 8, 8, out=torch.empty(64, 6))
    with pytest.raises(hip.NmfHipError):
        hip.camera_rays(np.eye(4), 100.0, 100.0, 4.0, 4.0, 8, 8, device="cpu")
    with pytest.raises(hip.NmfHipError):
        hip.frame_finish(8, 8, rgb=torch.zeros(64, 3))
    with pytest.raises(hip.NmfHipError):
        hip.frame_finish(8, 8)


def test_depth_colour_table():
    _, hip = _lib()
    t = hip.depth_colour_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    for q, row in ((0, (0, 0, 128)), (64, (0, 129, 255)), (128, (130, 255, 126)), (191, (255, 129, 0)), (255, (128, 0, 0))):
        assert tuple(int(v) for v in t[q]) == row, q
