"""Camera paths on the GPU: nmf_camera_rays and nmf_frame_finish bit for bit against the numpy fp32 restatements of
tests/test_camera_path_cpu.py, renderer.evaluation_path against the test's own sequence of calls (the evaluation render is
bit-deterministic, as tests/test_hip_relight_eval.py relies on), and the --path / --render-path command lines."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from nmf_amd import camera_path as cp
from nmf_amd import hip
from test_camera_path_cpu import camera_rays_np, frame_finish_np, quantise_np, random_pose
from test_hip_metrics import _s1_model, _tiny_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
# fewer pixels than a wave; a tail after whole groups of four; a row that crosses a 256-lane boundary; several workgroups and a count
# that is no multiple of any vector width
SIZES = [(1, 1), (5, 7), (3, 257), (64, 65)]


@pytest.mark.parametrize("H,W", SIZES)
def test_camera_rays_bit_identical_to_the_restatement(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    fx, fy, cx, cy = 111.25, 97.5, W / 2 + 1.75, H / 2 - 2.25
    for c2w in [np.eye(4, dtype=np.float32)] + [random_pose(rng) for _ in range(3)]:
        got = hip.camera_rays(c2w, fx, fy, cx, cy, H, W, device=DEV)
        assert got.shape == (H * W, 6) and got.dtype == torch.float32
        again = hip.camera_rays(torch.from_numpy(c2w), fx, fy, cx, cy, H, W, out=torch.full((H * W, 6), 7.0, device=DEV))
        assert torch.equal(got, again)                                             # two runs, the same bytes
        g = got.cpu().numpy()
        want = camera_rays_np(c2w, fx, fy, cx, cy, H, W)
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32))             # origins and directions, bit for bit
        ref = camera_rays_np(c2w, fx, fy, cx, cy, H, W, dtype=np.float64)
        assert np.abs(g[:, 3:].astype(np.float64) - ref[:, 3:]).max() <= 2.0 ** -20


def test_camera_rays_equal_the_loaders_rays_to_rounding():
    """the rays a data set builds on the host for its poses (get_rays of the normalised get_ray_directions): within 2^-20"""
    from nmf_amd.dataLoader.blender import get_ray_directions, get_rays
    H, W, fx = 40, 52, 61.0
    c2w = cp.orbit(5, (0, 0, 0), 4.0, 30.0)[3]
    d = get_ray_directions(H, W, [fx, fx])
    o_t, d_t = get_rays(d / torch.norm(d, dim=-1, keepdim=True), torch.from_numpy(c2w))
    got = hip.camera_rays(c2w, fx, fx, W / 2, H / 2, H, W, device=DEV).cpu()
    assert torch.equal(got[:, :3], o_t) and (got[:, 3:] - d_t).abs().max().item() <= 2.0 ** -20


def _maps(H, W, near, far, seed):
    """float maps with the values at which the conversions can go wrong: NaN, +-inf, negatives, values above 1, exact k / 255, depths
    below near and above far, normals of length 0 and 1"""
    rng = np.random.default_rng(seed)
    P = H * W
    special = np.array([np.nan, np.inf, -np.inf, -0.25, 0.0, 1.0, 1.5, 3e38, -3e38, 1e-9], dtype=np.float32)
    k255 = (rng.integers(0, 256, size=64) / 255.0).astype(np.float32)

    def sprinkle(a):
        flat = a.reshape(-1)
        pick = rng.random(flat.size) < 0.3
        flat[pick] = rng.choice(np.concatenate([special, k255]), size=int(pick.sum()))
        return a
    rgb = sprinkle(rng.uniform(-0.2, 1.2, size=(P, 3)).astype(np.float32))
    acc = sprinkle(rng.uniform(-0.2, 1.2, size=P).astype(np.float32))
    depth = rng.uniform(near - 1, far + 1, size=P).astype(np.float32)
    pick = rng.random(P) < 0.3
    depth[pick] = rng.choice(np.concatenate([special, np.float32(near) + k255 * np.float32(far - near), [near, far]]).astype(np.float32),
                             size=int(pick.sum()))
    normal = rng.normal(size=(P, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    normal[rng.random(P) < 0.2] = 0.0
    normal[rng.random(P) < 0.1] = [0.0, 0.0, 1.0]
    normal = sprinkle(normal)
    return dict(rgb=rgb, depth=depth, normal=normal, acc=acc)


@pytest.mark.parametrize("H,W", SIZES)
def test_frame_finish_equals_the_restatement_byte_for_byte(H, W):
    near, far = 2.5, 7.0
    host = _maps(H, W, near, far, seed=H * 100 + W)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
    jet = hip.depth_colour_table()
    other = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=(256, 3), dtype=np.uint8)).to(DEV)
    names = ("rgb", "depth", "normal", "acc")
    n_checked = 0
    for r in range(1, 5):
        for subset in itertools.combinations(names, r):
            for lut, lut_np in (("jet", jet), (None, None), (other, other.cpu().numpy())):
                if lut is other and (H, W) != (5, 7):
                    continue
                n = 3 * H * W * len(subset)
                for guard in (64, 61):                                   # a dword-aligned strip, and one that is not (byte stores)
                    buf = torch.full((guard + n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
                    out = hip.frame_finish(H, W, **{k: dev[k] for k in subset}, near_far=(near, far), lut=lut, out=buf[guard:guard + n])
                    assert out.shape == (H, len(subset) * W, 3)
                    b = buf.cpu().numpy()
                    assert (b[:guard] == 0xA5).all() and (b[guard + n:] == 0xA5).all(), (subset, guard)      # the guard band is untouched
                    want = frame_finish_np(H, W, **{k: host[k] for k in subset}, near=near, far=far, lut=lut_np)
                    assert np.array_equal(b[guard:guard + n].reshape(want.shape), want), (subset, lut is None, guard)
                    n_checked += 1
    assert n_checked == (15 * 2 + (15 if (H, W) == (5, 7) else 0)) * 2
    fresh = hip.frame_finish(H, W, rgb=dev["rgb"], acc=dev["acc"])
    assert fresh.dtype == torch.uint8 and np.array_equal(fresh.cpu().numpy(), frame_finish_np(H, W, rgb=host["rgb"], acc=host["acc"]))


def test_frame_finish_wrapper_checks_shapes():
    rgb = torch.zeros(35, 3, device=DEV)
    with pytest.raises(hip.NmfHipError):
        hip.frame_finish(5, 8, rgb=rgb)
    with pytest.raises(hip.NmfHipError):
        hip.frame_finish(5, 7, rgb=rgb, out=torch.empty(5, 7, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(hip.NmfHipError):
        hip.frame_finish(5, 7, rgb=rgb, near_far=(3.0, 3.0))
    with pytest.raises(hip.NmfHipError):
        hip.camera_rays(np.eye(4), 0.0, 10.0, 3.0, 3.0, 5, 7, device=DEV)
    with pytest.raises(hip.NmfHipError):
        hip.camera_rays(np.eye(4), 10.0, 10.0, 3.0, 3.0, 5, 7, out=torch.empty(35, 5, device=DEV))


# ---- renderer.evaluation_path ------------------------------------------------------------------------------------------------------
RES, FRAMES, SEED = 32, 3, 21
CAMERA = dict(w=RES, h=RES, fx=46.5, fy=46.5, cx=RES / 2, cy=RES / 2, near_far=[2.5, 7.0])
PANELS = ("rgb", "depth", "normal")


@pytest.fixture(scope="module")
def model():
    return _s1_model()


@pytest.fixture(scope="module")
def expected(model):
    """the frames of the path by the test's own calls on a fresh DeviceNoise of the seed: hip.camera_rays -> render_images ->
    the 8-bit conversions on the host (map_to_8bit; quantise_np for depth and normal)"""
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import map_to_8bit, render_images
    nerf, _ = model
    c2ws = cp.orbit(FRAMES, (0, 0, 0), 4.0, 30.0)
    noise = DeviceNoise(torch.device(DEV), seed=SEED)
    frames = []
    for k in range(FRAMES):
        rays = hip.camera_rays(c2ws[k], CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"], RES, RES, device=DEV)
        ims = render_images(nerf, rays, CAMERA["fx"], noise=noise, keys=("rgb_map", "depth", "world_normal"))
        frames.append(dict(rgb=map_to_8bit(ims["rgb_map"].reshape(RES, RES, 3).cpu().numpy()),
                           depth=quantise_np("depth", ims["depth"].reshape(RES, RES).cpu().numpy(), 2.5, 7.0, hip.depth_colour_table()),
                           normal=quantise_np("normal", ims["world_normal"].reshape(RES, RES, 3).cpu().numpy())))
    assert len({f["rgb"].tobytes() for f in frames}) == FRAMES and frames[0]["rgb"].std() > 5          # three different pictures
    return c2ws, frames


def _run(model, c2ws, out, **kw):
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import evaluation_path
    return evaluation_path(None, model[0], c2ws, None, str(out), noise=DeviceNoise(torch.device(DEV), seed=SEED), panels=PANELS,
                           camera=CAMERA, **kw)


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for nm in names:
            with open(os.path.join(d, nm), "rb") as f:
                out[os.path.relpath(os.path.join(d, nm), root)] = f.read()
    return out


def test_evaluation_path_writes_the_frames_of_its_own_sequence(model, expected, tmp_path):
    from PIL import Image
    c2ws, frames = expected
    res = _run(model, c2ws, tmp_path / "a", prtx="p_", writer_depth=2)
    assert res["frames"] == FRAMES and res["panels"] == list(PANELS) and res["rays_per_s"] > 0
    assert set(res["seconds"]) == {"rays", "render", "finish", "write_wait", "total", "animation"}
    assert all(v >= 0 for v in res["seconds"].values()) and res["seconds"]["render"] > res["seconds"]["rays"] > 0
    for k in range(FRAMES):
        for panel, sub in (("rgb", ""), ("depth", "depth"), ("normal", "world_normal")):
            png = np.asarray(Image.open(tmp_path / "a" / sub / f"p_{k:03d}.png"))
            assert png.shape == (RES, RES, 3) and np.array_equal(png, frames[k][panel]), (k, panel)
    assert not os.path.exists(tmp_path / "a" / "acc_map")
    for name, panel in (("p_video.png", "rgb"), ("p_depthvideo.png", "depth")):
        video = Image.open(tmp_path / "a" / name)
        assert video.n_frames == FRAMES and video.info.get("loop") == 0
        for k in range(FRAMES):
            video.seek(k)
            assert np.array_equal(np.asarray(video.convert("RGB")), frames[k][panel]), (name, k)
    assert np.array_equal(cp.load_path(tmp_path / "a" / "transforms_path.json"), c2ws)
    poses, cam = cp.load_path(tmp_path / "a" / "transforms_path.json", with_camera=True)
    assert cam == CAMERA
    # the synchronous writer writes the same files
    _run(model, c2ws, tmp_path / "b", prtx="p_", writer_depth=0)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert set(a) == set(b) and len(a) == 3 * FRAMES + 3 and all(a[k] == b[k] for k in a)
    # other containers
    _run(model, c2ws, tmp_path / "c", animation="none")
    assert sorted(os.listdir(tmp_path / "c")) == ["000.png", "001.png", "002.png", "depth", "transforms_path.json", "world_normal"]
    _run(model, c2ws, tmp_path / "d", animation="gif")
    assert Image.open(tmp_path / "d" / "video.gif").n_frames == FRAMES and os.path.exists(tmp_path / "d" / "depthvideo.gif")


@pytest.mark.parametrize("writer_depth", [0, 2])
def test_a_failing_writer_raises_in_the_caller(model, expected, tmp_path, monkeypatch, writer_depth):
    import threading
    from nmf_amd import renderer
    calls, orig = [], renderer._png

    def failing(path, arr):
        calls.append(path)
        if len(calls) == 2:
            raise OSError("disk full (made up by the test)")
        orig(path, arr)
    monkeypatch.setattr(renderer, "_png", failing)
    with pytest.raises(OSError, match="disk full"):
        _run(model, expected[0], tmp_path / "x", writer_depth=writer_depth)
    assert not [t for t in threading.enumerate() if t.name == "nmf-path-writer"]          # joined before the exception left
    assert len(calls) == 2 and not os.path.exists(tmp_path / "x" / "video.png")


def test_evaluation_path_takes_the_camera_of_a_data_set(model, tmp_path):
    from PIL import Image
    from nmf_amd.dataLoader import BlenderDataset
    scene = tmp_path / "tiny"
    _tiny_scene(scene)
    ds = BlenderDataset(str(scene), split="test", is_stack=True, N_vis=-1)
    from nmf_amd.renderer import evaluation_path
    res = evaluation_path(ds, model[0], ds.render_path[:2], None, str(tmp_path / "o"), panels=("rgb", "acc"), animation="none")
    assert res["frames"] == 2 and res["panels"] == ["rgb", "acc"]
    assert np.asarray(Image.open(tmp_path / "o" / "acc_map" / "001.png")).shape == (16, 16, 3)
    with pytest.raises(ValueError):
        evaluation_path(ds, model[0], ds.render_path[:1], None, str(tmp_path / "o"), panels=("depth",))


def test_from_dataset_returns_what_the_scene_tool_used(tmp_path):
    """a scene written by tools/make_blender_scene.py: its cameras sit at radius 4 with z / 4 drawn uniformly from (0.15, 0.9) by a
    seeded generator, the training views first -- the orbit of its test split has that radius and the mean of those elevations"""
    from nmf_amd.dataLoader import BlenderDataset
    from test_hip_metrics import _load_tool
    scene = tmp_path / "scene"
    _load_tool("make_blender_scene").main(["--out", str(scene), "--views", "1", "--test-views", "3", "--res", "32", "--grid", "32",
                                           "--bg", "32"])
    rng = np.random.default_rng(0)
    zs = []
    for _ in range(1 + 3):
        zs.append(rng.uniform(0.15, 0.9))
        rng.uniform(0, 2 * np.pi)
    want = np.degrees(np.arcsin(zs[1:]))
    ds = BlenderDataset(str(scene), split="test", is_stack=True, N_vis=-1)
    center, radius, elev = cp.dataset_orbit(ds)
    assert np.abs(center).max() == 0 and abs(radius - 4.0) <= 1e-5 and np.abs(elev - want).max() <= 1e-4
    eyes = cp.from_dataset(ds, "orbit", 8)[:, :3, 3].astype(np.float64)
    assert np.abs(np.linalg.norm(eyes, axis=-1) - 4.0).max() <= 1e-5
    assert np.abs(np.degrees(np.arcsin(eyes[:, 2] / 4.0)) - want.mean()).max() <= 1e-3
    assert np.array_equal(cp.load_path(scene / "transforms_test.json"), ds.poses.numpy())


# ---- the command lines -------------------------------------------------------------------------------------------------------------
PARENT_KEYS = {"frames", "width", "height", "chunk", "seconds", "rays_per_s", "relit"}


def test_render_path_command_line(model, tmp_path, capsys):
    from nmf_amd import render as R
    nerf, cfg = model
    ck = str(tmp_path / "m.th")
    nerf.save(ck, cfg["arch"])
    base = ["--ckpt", ck, "--views", "1", "--res", str(RES)]
    plain = R.main(base)
    assert set(plain) == PARENT_KEYS                                                    # without --path: the parent's line
    a = tmp_path / "a"
    rec = R.main(base + ["--path", "orbit", "--frames", "3", "--out", str(a), "--panels", "rgb,depth,normal"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and set(lines[0]) == PARENT_KEYS and set(lines[1]) == PARENT_KEYS | {"path"}
    assert lines[1] == json.loads(json.dumps(rec))
    p = rec["path"]
    assert p["frames"] == 3 and p["panels"] == ["rgb", "depth", "normal"] and p["width"] == p["height"] == RES and p["kind"] == "orbit"
    files = _files(a / "path")
    assert set(files) == ({f"{k:03d}.png" for k in range(3)} | {f"{d}/{k:03d}.png" for d in ("depth", "world_normal") for k in range(3)}
                          | {"video.png", "depthvideo.png", "transforms_path.json"})
    assert os.path.exists(a / "000.png")                                                # the view frames of --out, as before
    eyes = cp.load_path(a / "path" / "transforms_path.json")[:, :3, 3]
    assert np.abs(np.linalg.norm(eyes, axis=-1) - 4.0).max() <= 1e-5 and np.abs(eyes[:, 2] - 2.0).max() <= 1e-5      # radius 4, 30 degrees
    # the saved path renders the same frames again, byte for byte
    b = tmp_path / "b"
    R.main(base + ["--path", str(a / "path" / "transforms_path.json"), "--out", str(b), "--panels", "rgb,depth,normal"])
    again = _files(b / "path")
    assert set(again) == set(files) and all(again[k] == files[k] for k in files if k.endswith(".png"))
    assert np.array_equal(cp.load_path(b / "path" / "transforms_path.json"), cp.load_path(a / "path" / "transforms_path.json"))
    capsys.readouterr()
    with pytest.raises(SystemExit):
        R.main(base + ["--path", "orbit"])                                              # needs --out
    with pytest.raises(SystemExit):
        R.main(base + ["--path", "interp", "--out", str(b)])                            # needs a data set
    with pytest.raises(SystemExit):
        R.main(base + ["--path", "orbit", "--out", str(b), "--panels", "depth"])


def test_train_render_path(tmp_path, capsys, monkeypatch):
    from nmf_amd import train as T
    scene = tmp_path / "tiny"
    _tiny_scene(scene)
    monkeypatch.chdir(tmp_path)
    flags = ["--datadir", str(scene), "--near-far", "2.5", "7", "--iters", "3", "--grid", "16", "--bg", "16", "--eval-every", "3",
             "--test-views", "1"]
    T.main(flags + ["--render-path"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and lines[-1]["path"]["frames"] == 120 and lines[-1]["path"]["panels"] == ["rgb", "depth"]
    folder = tmp_path / "log" / "tiny_test" / "imgs_path_all"
    names = set(os.listdir(folder))
    assert {f"{k:03d}.png" for k in range(120)} <= names and {"video.png", "depthvideo.png", "transforms_path.json", "depth"} <= names
    assert len(os.listdir(folder / "depth")) == 120 and cp.load_path(folder / "transforms_path.json").shape == (120, 4, 4)
    with pytest.raises(SystemExit):
        T.main(["--iters", "1", "--render-path"])                                       # the synthetic orbit has no render_path
