"""Scene composition on the GPU (nmf_amd/compose.py, csrc/compose.hip): the merge and placement kernels against
their numpy restatements (tests/test_compose_cpu.py), a single-part scene against the part rendered alone (bitwise), the opacity law
of overlapping parts, parts beyond their trained range, bounce rays that travel in the world, the environment rule, the command line."""
import json
import os

import numpy as np
import pytest
import torch

from nmf_amd import hip, synthetic
from test_compose_cpu import merge_rank_np, merge_scatter_np, rays_place_margin, rays_place_np, rotate_rows_np

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = 32
SEED = 31


@pytest.fixture(scope="module")
def model():
    from nmf_amd.config import build_model
    nerf, cfg = build_model(grid=32, bg_resolution=32, device=DEV)
    nerf.load_state_dict(synthetic.state_dict_s1(grid=32, bg_resolution=32, seed=0), strict=False)
    nerf.sampler.update(nerf.rf, init=False)
    nerf.sampler.update(nerf.rf, init=True)
    nerf.eval()
    return nerf, cfg


@pytest.fixture(scope="module")
def camera():
    """all pixels of a 32 x 32 S1 camera: rays [1024, 6] on the device, focal"""
    rays, focal = synthetic.camera_rays(0, wh=RES, all_pixels=True)
    return rays.to(DEV).contiguous(), focal


def _noise():
    from nmf_amd.noise import DeviceNoise
    return DeviceNoise(torch.device(DEV, torch.cuda.current_device()), seed=SEED)


def _placement(spec):
    from nmf_amd.compose import Placement
    return Placement.from_spec(spec)


def _general_case():
    """the placement and rays of the placement test; its margin is the one the rotated normals are compared under too"""
    P = _placement("t=0.5,-0.25,0.125;r=33,12,-70;s=0.6")
    rays = synthetic.camera_rays(0, wh=RES, all_pixels=True)[0].numpy()
    return P, rays


@pytest.fixture(scope="module")
def margin():
    P, rays = _general_case()
    m = max(rays_place_margin(rays, P.R, P.t, P.s, inv) for inv in (0, 1))
    print(f"restatement margin of nmf_rays_place (4 x |fp32 restatement - float64|): {m:.3e}")
    assert 0 < m < 1e-5
    return m


# ---- 1. merge, exact -------------------------------------------------------------------------------------------------------------------
SIGNED_PERMUTATIONS = ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],
                       [[1, 0, 0], [0, 0, -1], [0, 1, 0]])


def _lists(K, B, rng):
    counts = rng.choice([0, 1, 2, 63, 64, 65, 300], size=(K, B))
    counts[:, 5] = 0                                        # a ray that is empty in every part
    counts[:, 11] = 300                                     # ... and one that is long in every part
    if K >= 2:
        counts[1] = 0                                       # a part without samples
    offsets, zs = [], []
    for k in range(K):
        offsets.append(np.concatenate([[0], np.cumsum(counts[k])]).astype(np.int64))
        # multiples of 1/8 below 16: ties inside a list and across lists are common
        zs.append(np.concatenate([np.sort(rng.integers(0, 128, size=c)) for c in counts[k]] + [[]]).astype(np.float32) / 8)
    scales = [float(2.0 ** e) for e in rng.integers(-2, 3, size=K)]
    return offsets, zs, scales


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_merge_is_the_stable_merge(K, margin):
    B = 37
    rng = np.random.default_rng(100 + K)
    offsets, zs, scales = _lists(K, B, rng)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dt)      # noqa: E731
    dst, off_m = hip.merge_rank([t(o) for o in offsets], [t(z) for z in zs], scales, B)
    want, want_off = merge_rank_np(offsets, zs, scales, B)
    assert off_m.dtype == torch.int64 and np.array_equal(off_m.cpu().numpy(), want_off)
    M = int(want_off[-1])
    for k in range(K):
        assert dst[k].dtype == torch.int64 and np.array_equal(dst[k].cpu().numpy(), want[k]), k
    assert sorted(np.concatenate([d.cpu().numpy() for d in dst]).tolist()) == list(range(M))           # a permutation
    again, _ = hip.merge_rank([t(o) for o in offsets], [t(z) for z in zs], scales, B)
    assert all(torch.equal(a, b) for a, b in zip(dst, again))

    # scatter: every merged array against the restatement, bit for bit
    f, i = np.float32, np.int32
    got = dict(sigma=torch.zeros(M, device=DEV), dist=torch.zeros(M, device=DEV), z=torch.zeros(M, device=DEV),
               normal=torch.zeros(M, 3, device=DEV), ray_id=torch.zeros(M, dtype=torch.int32, device=DEV),
               part=torch.zeros(M, dtype=torch.int32, device=DEV), src=torch.zeros(M, dtype=torch.int32, device=DEV),
               inv=torch.full((M,), -7, dtype=torch.int32, device=DEV))
    ref = {k: v.cpu().numpy().copy() for k, v in got.items()}
    row_base = 0
    for k in range(K):
        m = len(zs[k])
        sigma, dist = rng.random(m).astype(f) * 40, rng.random(m).astype(f) * 0.05
        n = rng.normal(size=(m, 3)).astype(f)
        ray_id = np.repeat(np.arange(B), np.diff(offsets[k])).astype(i)
        inv = np.where(rng.random(m) < 0.3, np.arange(m), -1).astype(i)
        R = np.array(SIGNED_PERMUTATIONS[k % 4], dtype=np.float64)
        ratio = [1.0, 0.5, 1.25, 3.0][k % 4]
        args = dict(part=k, sigma_ratio=ratio, scale=scales[k], R=R, row_base=row_base)
        hip.merge_scatter(dst[k], M, sigma=t(sigma), dist=t(dist), z=t(zs[k]), normal=t(n), ray_id=t(ray_id), inv=t(inv), out=got, **args)
        merge_scatter_np(ref, want[k], sigma=sigma, dist=dist, z=zs[k], normal=n, ray_id=ray_id, inv=inv, **args)
        row_base += m
    for name in got:
        assert got[name].cpu().numpy().tobytes() == ref[name].tobytes(), name
    # the merged list is depth-ordered inside every ray, and ties keep the part order
    z_m, part_m = ref["z"], ref["part"]
    for r in range(B):
        a, b = int(want_off[r]), int(want_off[r + 1])
        assert np.all(np.diff(z_m[a:b]) >= 0)
        tie = np.diff(z_m[a:b]) == 0
        assert np.all(np.diff(part_m[a:b])[tie] >= 0)

    # a general rotation of the normals: the restatement's bits, and float64 within the margin of the placement test
    P, _ = _general_case()
    k = K - 1 if len(zs[K - 1]) else 0
    n = rng.normal(size=(len(zs[k]), 3)).astype(f)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out = dict(normal=torch.zeros(M, 3, device=DEV))
    hip.merge_scatter(dst[k], M, part=k, normal=t(n), R=P.R, out=out)
    rot = out["normal"].cpu().numpy()[want[k]]
    assert rot.tobytes() == rotate_rows_np(n, P.R).tobytes()
    dev64 = float(np.abs(rot.astype(np.float64) - rotate_rows_np(n, P.R, np.float64)).max())
    print(f"K={K}: rotated normals, max |kernel - float64| = {dev64:.3e} (margin {margin:.3e})")
    assert dev64 <= margin


# ---- 2. placement ----------------------------------------------------------------------------------------------------------------------
def test_rays_place_matches_its_restatement(margin):
    P, rays = _general_case()
    dev = torch.from_numpy(rays).to(DEV)
    for inv in (0, 1):
        got = hip.rays_place(dev, P, inverse=inv).cpu().numpy()
        assert got.tobytes() == rays_place_np(rays, P.R, P.t, P.s, inv).tobytes(), inv
        d64 = float(np.abs(got.astype(np.float64) - rays_place_np(rays, P.R, P.t, P.s, inv, np.float64)).max())
        print(f"nmf_rays_place inverse={inv}: max |kernel - float64| = {d64:.3e} (margin {margin:.3e})")
        assert d64 <= margin
        assert hip.rays_place(dev, P.R, P.t, P.s, inverse=inv).cpu().numpy().tobytes() == got.tobytes()          # the matrix form
    # the identity returns the input's bits, signed zeros included
    odd = rays.copy()
    odd[0, :] = [-0.0, 0.0, 1.5, -0.0, -1.0, 0.0]
    for inv in (0, 1):
        assert hip.rays_place(torch.from_numpy(odd).to(DEV), _placement(""), inverse=inv).cpu().numpy().tobytes() == odd.tobytes()
    assert hip.rays_place(torch.zeros(0, 6, device=DEV), P).shape == (0, 6)
    with pytest.raises(hip.NmfHipError):
        hip.rays_place(dev, np.diag([1.0, 1.0, 1.1]), np.zeros(3), 1.0)
    with pytest.raises(hip.NmfHipError):
        hip.rays_place(dev, np.eye(3), np.zeros(3), 0.0)


# ---- 3. a single part is the part ----------------------------------------------------------------------------------------------------
def _same_weight_kernels(nerf, rays, focal):
    """are rf.query_weights and rf.query + Composite the same bits?  (both are vm_query_fwd followed by composite_fwd)"""
    from nmf_amd.functional import Composite
    with torch.no_grad():
        S = nerf.sampler.sample_compact(rays, focal, is_train=False, dynamic_batch_size=False, noise=_noise())
        off = S.offsets[: S.b + 1]
        w1 = nerf.rf.query_weights(S.xyzt, S.dist, off, S.b, want_app=False, want_normal=True)[0]
        w2 = Composite.apply(nerf.rf.query(S.xyzt, want_app=False, want_normal=True)[0], S.dist, off, S.b, float(nerf.rf.distance_scale))
    assert S.M > 1000
    return torch.equal(w1, w2)


ANCHORS = {"identity": "", "translated_half": "t=0.5,-0.25,0.125;s=0.5", "yaw": "r=37.3,0,0"}


@pytest.mark.parametrize("name", list(ANCHORS))
def test_single_part_scene_is_the_part_bitwise(name, model, camera, margin, monkeypatch):
    from nmf_amd.compose import ComposedScene
    nerf, _ = model
    L, focal = camera
    if not _same_weight_kernels(nerf, L, focal):            # the baseline then goes through query + Composite as the scene does
        owner = next(c for c in type(nerf.rf).__mro__ if "query_weights" in c.__dict__)
        monkeypatch.delattr(owner, "query_weights")
        print("rf.query_weights and rf.query + Composite differ: the baseline runs without query_weights")
    else:
        print("rf.query_weights and rf.query + Composite give the same bits")
    P = _placement(ANCHORS[name])
    n, f = nerf.sampler.near_far
    scene = ComposedScene([(nerf, P)], near_far=(n * P.s, f * P.s))
    W = hip.rays_place(L, P, inverse=False)                 # world rays that see the placed part as the camera sees the part
    local = hip.rays_place(W, P, inverse=True)
    kw = dict(is_train=False, bg_col=torch.ones(3, device=DEV))
    with torch.no_grad():
        base, bst = nerf(local, focal, draw_debug=False, noise=_noise(), **kw)
        got, gst = scene(W, focal, draw_debug=False, noise=_noise(), **kw)
        assert float(base["acc_map"].max()) > 0.9 and len(bst["n_samples"]) == 2           # the object is hit, bounce rays re-traced
        for key in ("rgb_map", "acc_map", "rgb_lin"):
            assert torch.equal(got[key], base[key]), (name, key)
        assert gst["n_samples"] == bst["n_samples"] and gst["rays_kept"] == W.shape[0] and bool(gst["whole_valid"].all())
        # depth and normals in the world frame
        based, _ = nerf(local, focal, draw_debug=True, noise=_noise(), **kw)
        gotd, _ = scene(W, focal, draw_debug=True, noise=_noise(), **kw)
        assert torch.equal(gotd["depth"], P.s * based["depth"]), name
        assert torch.equal(gotd["surf_width"], based["surf_width"])
        acc = based["acc_map"][:, None].double()
        R = torch.from_numpy(P.R).to(DEV)
        want_n = (based["world_normal"].double() - (1 - acc)) @ R.T + (1 - acc)
        dn = float((gotd["world_normal"].double() - want_n).abs().max())
        print(f"{name}: world_normal against the rotated local one, max deviation {dn:.3e} (margin {margin:.3e})")
        assert dn <= margin
        with pytest.raises(NotImplementedError):
            gotd["albedo"]
        with pytest.raises(NotImplementedError):
            "roughness" in gotd
    with pytest.raises(ValueError):
        scene(W, focal, is_train=True)


def test_single_part_scene_at_the_arguments_of_a_retrace(model, camera):
    """the identity scene called as a level-1 render: no background colour, no tonemap, a near override, mip values"""
    from nmf_amd.compose import ComposedScene
    nerf, _ = model
    L, focal = camera
    scene = ComposedScene([(nerf, _placement(""))], near_far=tuple(nerf.sampler.near_far))
    mip = torch.linspace(-6.0, -1.0, L.shape[0], device=DEV)
    kw = dict(recur=1, bg_col=None, tonemap=False, override_near=3.1, start_mipval=mip, is_train=False, draw_debug=False)
    with torch.no_grad():
        base, bst = nerf(L, focal, noise=_noise(), **kw)
        got, gst = scene(L, focal, noise=_noise(), **kw)
    assert float(base["acc_map"].max()) > 0.9 and float(base["acc_map"].min()) < 0.1
    for key in ("rgb_map", "acc_map"):
        assert torch.equal(got[key], base[key]), key
    assert gst["n_samples"] == bst["n_samples"] and "rgb_lin" not in got


# ---- 4. opacity law ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
def test_overlapping_parts_add_their_optical_depths(level, model, camera):
    from nmf_amd.compose import ComposedScene
    nerf, _ = model
    W, focal = camera
    P0, P1 = _placement(""), _placement("t=0.6,0.3,0;r=40,0,0;s=0.7")
    kw = dict(is_train=False, draw_debug=False)
    if level == 1:
        kw.update(recur=1, bg_col=None, tonemap=False, override_near=0.5, start_mipval=torch.full((W.shape[0],), -3.0, device=DEV))
    with torch.no_grad():
        a0 = ComposedScene([(nerf, P0)])(W, focal, noise=_noise(), **kw)[0]["acc_map"].double()
        a1 = ComposedScene([(nerf, P1)])(W, focal, noise=_noise(), **kw)[0]["acc_map"].double()
        pair = ComposedScene([(nerf, P0), (nerf, P1)])
        ims, st = pair(W, focal, noise=_noise(), **kw)
        if level == 0:
            width = ims["surf_width"]
        else:           # (a level-1 render has no debug images: the merged segment lengths from the level-0 call's kernels)
            S = [pair._sampler(k).sample_compact(hip.rays_place(W, P, inverse=True), focal, override_near=0.5 / P.s, is_train=False,
                                                 dynamic_batch_size=False) for k, P in enumerate((P0, P1))]
            width = sum(s.offsets[1: W.shape[0] + 1] - s.offsets[: W.shape[0]] for s in S)
    both = int(((a0 > 0.5) & (a1 > 0.5)).sum())
    assert both > 20 and int((a0 > 0.5).sum()) > both and int((a1 > 0.5).sum()) > both           # a partial overlap
    want = 1 - (1 - a0) * (1 - a1)
    err = (ims["acc_map"].double() - want).abs()
    bound = 4 * (width.double() + 2) * 2.0 ** -24
    print(f"level {level}: opacity law, max error {float(err.max()):.3e}, max error / bound {float((err / bound).max()):.3f}, "
          f"longest merged segment {int(width.max())}")
    assert bool((err <= bound).all())
    assert int(width.sum()) == st["n_samples"][0]


# ---- 5. a part renders at any distance ----------------------------------------------------------------------------------------------
def test_a_part_beyond_its_trained_far_plane(model):
    from nmf_amd.compose import ComposedScene
    nerf, _ = model
    d = np.array([0.36, -0.8, 0.48])
    u = np.cross(d, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(u, d)
    g = np.linspace(-1.3, 1.3, 24)
    o = -4.5 * d + (g[:, None, None] * u + g[None, :, None] * v).reshape(-1, 3)
    rays = torch.from_numpy(np.concatenate([o, np.broadcast_to(d, o.shape)], 1).astype(np.float32)).to(DEV)
    D = 8.0                                                  # 4.5 + 8 > the trained far plane at 7
    assert 4.5 + D - 1.5 * np.sqrt(3) > nerf.sampler.near_far[1]
    step = float(hip.host(nerf.sampler.stepsize))
    kw = dict(is_train=False, draw_debug=True)
    with torch.no_grad():
        near = ComposedScene([(nerf, _placement(""))])(rays, 500.0, noise=_noise(), **kw)[0]
        far = ComposedScene([(nerf, _placement("t=" + ",".join(repr(float(x)) for x in D * d)))])(rays, 500.0, noise=_noise(), **kw)[0]
    hit = near["acc_map"] > 0.5
    assert 50 < int(hit.sum()) < rays.shape[0] - 50
    assert torch.equal(far["acc_map"] > 0.5, hit)
    # (the depth image is sum_k w_k z_k, which a move by D raises by acc D: the expected depth sum_k w_k z_k / acc is what grows by D)
    grow = (far["depth"] / far["acc_map"] - near["depth"] / near["acc_map"])[hit]
    print(f"depth grows by {float(grow.min()):.4f} .. {float(grow.max()):.4f} for a move of {D} (step {step:.4f})")
    assert float((grow - D).abs().max()) <= 2 * step


# ---- 6. bounce rays travel in the world ---------------------------------------------------------------------------------------------
def test_bounce_rays_travel_in_the_world(model, camera):
    from nmf_amd.compose import ComposedScene, Placement
    nerf, _ = model
    L, focal = camera
    calls = []

    class Recording(ComposedScene):
        def _render(self, rays, focal, start_mipval, bg_col, recur, *a, **k):
            calls.append((recur, rays[:, :3].detach().clone()))
            return super()._render(rays, focal, start_mipval, bg_col, recur, *a, **k)

    P0 = _placement("t=3,0,0")
    W = hip.rays_place(L, P0, inverse=False)
    scene = Recording([(nerf, P0)])
    with torch.no_grad():
        ims, _ = scene(W, focal, is_train=False, noise=_noise())
    assert float(ims["acc_map"].max()) > 0.9
    deep = [o for r, o in calls if r == 1]
    assert deep and sum(o.shape[0] for o in deep) >= 500
    step = float(hip.host(nerf.sampler.stepsize))
    box = torch.from_numpy(scene.world_aabb()).to(DEV)
    pad = 5e-3 * P0.s + step
    own = nerf.rf.aabb.to(DEV).double()
    for o in deep:
        o = o.double()
        assert bool(((o >= box[0] - pad) & (o <= box[1] + pad)).all())
        assert not bool(((o >= own[0]) & (o <= own[1])).all(dim=1).any())          # none in part 0's LOCAL box: they are world points

    # a second, smaller part hovering above the first: it shows in the reflections (and shadows) of the first one's top face
    P1 = Placement(None, (3.0, 0.0, 1.7), 0.5)
    pair = ComposedScene([(nerf, P0), (nerf, P1)])
    with torch.no_grad():
        on, _ = pair(W, focal, is_train=False, noise=_noise())
        pair.cross_reflections = False
        off, _ = pair(W, focal, is_train=False, noise=_noise())
        a0 = ComposedScene([(nerf, P0)])(W, focal, is_train=False, noise=_noise())[0]["acc_map"]
        a1 = ComposedScene([(nerf, P1)])(W, focal, is_train=False, noise=_noise())[0]["acc_map"]
    assert torch.equal(on["acc_map"], off["acc_map"])
    of_part0 = (a0 > 0.9) & (a1 < 1e-3)
    assert int(of_part0.sum()) > 50
    differs = (on["rgb_lin"] != off["rgb_lin"]).any(dim=1)
    print(f"cross reflections change {int((differs & of_part0).sum())} of {int(of_part0.sum())} pixels of part 0")
    assert bool((differs & of_part0).any())


# ---- 7. one environment, in the world ------------------------------------------------------------------------------------------------
def test_environment_rule(model, camera):
    from nmf_amd import relight
    from nmf_amd.compose import ComposedScene
    nerf, _ = model
    W, focal = camera
    scene = ComposedScene([(nerf, _placement("")), (nerf, _placement("t=0.9,0.9,0;r=55,0,0;s=0.5")), (nerf, _placement("t=0,0,1.4;s=0.4"))])
    own = nerf.bg_module
    render = lambda: scene(W, focal, is_train=False, noise=_noise())[0]["rgb_map"]          # noqa: E731
    with torch.no_grad():
        assert scene.bg_module is own                       # part 0 is not rotated: its lighting is the world's
        assert scene.local_env(0) is own and scene.local_env(2) is own and scene.local_env(1) is not own
        first = render()
        turned = relight.rotate_env(own, relight.rotation(yaw=120.0, pitch=30.0))
        with relight.relit(scene, turned):
            assert scene.bg_module is turned
            assert scene.local_env(0) is turned and scene.local_env(2) is turned         # R = I: the module itself, not a copy
            assert scene.local_env(1) is not turned and scene.local_env(1) is not own
            second = render()
        assert scene.bg_module is own and scene.local_env(0) is own
        third = render()
    assert not torch.equal(first, second) and float((first - second).abs().max()) > 0.02
    assert torch.equal(first, third)
    # the rotated part's local map IS the world map seen from its frame: L_1(d) = L_w(R_1 d), up to the resampling
    R1 = torch.from_numpy(scene.parts[1][1].R).float().to(DEV)
    d = torch.nn.functional.normalize(torch.randn(512, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1)), dim=1)
    rough = torch.full((512,), -2.0, device=DEV)
    with torch.no_grad():
        a = scene.local_env(1)(d, rough).reshape(-1, 3)
        b = own((d @ R1.T).contiguous(), rough).reshape(-1, 3)
        c = own(d, rough).reshape(-1, 3)                     # (the unrotated lookup: what a wrong rotation would give)
    err, wrong = float((a - b).abs().mean()), float((a - c).abs().mean())
    print(f"local map of the rotated part against the world map along R d: mean |diff| {err:.4f}, along d {wrong:.4f}")
    assert err < 0.5 * wrong


# ---- 8. command line -----------------------------------------------------------------------------------------------------------------
PARENT_KEYS = {"frames", "width", "height", "chunk", "seconds", "rays_per_s", "relit"}


def test_render_command_line_composes(model, tmp_path, capsys):
    from nmf_amd import camera_path as cp
    from nmf_amd import render as R
    nerf, cfg = model
    a, b = str(tmp_path / "a.th"), str(tmp_path / "b.th")
    nerf.save(a, cfg["arch"])
    nerf.save(b, cfg["arch"])
    out = tmp_path / "d"
    base = ["--ckpt", a, "--views", "1", "--res", str(RES)]
    rec = R.main(base + ["--insert", b + "@t=1.2,0,0;r=40,0,0;s=0.7", "--out", str(out)])
    assert rec["parts"] == 2 and len(rec["placements"]) == 2 and rec["placements"][1]["scale"] == 0.7
    assert rec["placements"][0]["translation"] == [0.0, 0.0, 0.0] and set(rec) == PARENT_KEYS | {"parts", "placements"}
    assert os.path.getsize(out / "000.png") > 0
    plain = R.main(base)
    assert set(plain) == PARENT_KEYS                        # without --insert / --place: the parent's line
    rec2 = R.main(base + ["--insert", b + "@t=1.2,0,0;r=40,0,0;s=0.7", "--place", "r=10,0,0", "--out", str(out), "--path", "orbit",
                          "--frames", "2", "--panels", "rgb,depth", "--near-far", "0.5", "12"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 3 and lines[2] == json.loads(json.dumps(rec2)) and lines[0]["parts"] == 2
    p = rec2["path"]
    assert p["frames"] == 2 and p["panels"] == ["rgb", "depth"] and p["kind"] == "orbit"
    names = set(os.listdir(out / "path"))
    assert {"000.png", "001.png", "depth", "video.png", "depthvideo.png", "transforms_path.json"} <= names
    assert set(os.listdir(out / "path" / "depth")) == {"000.png", "001.png"}
    # the orbit circles the box around both objects, at 4 x the ratio of that box's diagonal to one object's
    eyes = cp.load_path(out / "path" / "transforms_path.json")[:, :3, 3].astype(np.float64)
    corners = np.array([[x, y, z] for x in (-1.5, 1.5) for y in (-1.5, 1.5) for z in (-1.5, 1.5)])
    pts = np.concatenate([_placement(sp).apply(corners) for sp in ("r=10,0,0", "t=1.2,0,0;r=40,0,0;s=0.7")])
    lo, hi = pts.min(0), pts.max(0)
    radius = 4.0 * max(np.linalg.norm(hi - lo) / np.linalg.norm([3.0, 3.0, 3.0]), 1.0)
    assert np.abs(np.linalg.norm(eyes - 0.5 * (lo + hi), axis=1) - radius).max() < 1e-4
    assert np.abs(eyes[:, 2] - (0.5 * (lo + hi)[2] + radius * 0.5)).max() < 1e-4                    # elevation 30 degrees
