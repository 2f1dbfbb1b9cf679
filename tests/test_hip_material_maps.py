"""Material maps of the fused evaluation pass (nmf_material_maps, StepCore.render(want_materials=True)): albedo, roughness, diffuse,
tint and spec per ray, as the reference's evaluation writes them (renderer.py:440-463), against its fixtures, a float64 restatement,
the operator-graph module path (draw_debug=True), and through renderer.render_images / evaluation / the render command line."""
import os

import numpy as np
import pytest
import torch

from conftest import Golden, assert_close
from test_hip_e2e import DEV, _fixture_rays, _full_size_model, _pin_reference_bookkeeping
from test_hip_metrics import _load_tool, _s1_model, _tiny_scene

pytestmark = pytest.mark.gpu

MAPS = ("albedo", "roughness", "diffuse", "tint", "spec")


def _fused(nerf):
    from nmf_amd.renderer import _eval_pass
    nerf.eval()
    fp = _eval_pass(nerf)
    assert fp is not None and fp.core() is not None, "the fused evaluation pass must be the one under test"
    return fp


def _restate(tr, core):
    """the table of the maps in float64 over the inputs the pass recorded (models/microfacet.py Shaded.debug, per ray)"""
    d = lambda k: tr[k].double()                                             # noqa: E731
    app, n, w, offsets, rays = d("mm_app0"), d("mm_normals0"), d("mm_w0"), tr["mm_offsets0"].long(), d("mm_rays0")
    inv, row_off, cnt = tr["mm_inv0"].long(), tr["mm_row_off0"].long(), tr["mm_cnt0"].long()
    inc, brdf, conv, acc = d("mm_incoming0"), d("mm_brdf0"), d("mm_conv0").reshape(9, 3), d("mm_acc0")
    W, b = core.head_W.double().reshape(11, 24), core.head_b.double().reshape(11)
    dm, db, tb, fb, rb = core.head_p
    a = app @ W.T + b
    albedo = torch.sigmoid(dm * a[:, 0:3] + db).clip(0, 1)
    f0 = torch.sigmoid(a[:, 6:9] + fb)
    r1 = (torch.sigmoid(a[:, 9:10] + rb) * 0.5).clip(1e-2, 1)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    Y = torch.stack([torch.full_like(x, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z,
                     0.4886025119029199 * x, 1.0925484305920792 * x * y, 1.0925484305920792 * y * z,
                     0.31539156525252005 * (3 * z * z - 1), 1.0925484305920792 * x * z, 0.5462742152960396 * (x * x - y * y)], 1)
    E = Y @ conv
    M, B, Mb = app.shape[0], offsets.shape[0] - 1, row_off.shape[0] - 1
    ray_id = torch.repeat_interleave(torch.arange(B, device=app.device), offsets[1:] - offsets[:-1])
    v = rays[ray_id, 3:6]
    cos_t = (-v * n).sum(-1, keepdim=True).abs()
    Fr = f0 + (1 - f0) * (1 - cos_t).clip(0, 1) ** 5
    row_of_ray = torch.repeat_interleave(torch.arange(Mb, device=app.device), row_off[1:] - row_off[:-1])
    ec = cnt.double().clip(min=1)[row_of_ray][:, None]
    spec_rows = torch.zeros(Mb, 3, dtype=torch.float64, device=app.device).index_add_(0, row_of_ray, inc / ec)
    brdf_rows = torch.zeros(Mb, 3, dtype=torch.float64, device=app.device).index_add_(0, row_of_ray, brdf / ec)
    has = inv >= 0
    spec = torch.zeros(M, 3, dtype=torch.float64, device=app.device)
    brgb = torch.zeros_like(spec)
    spec[has] = spec_rows[inv[has]]
    brgb[has] = brdf_rows[inv[has]]
    per = dict(albedo=albedo, roughness=r1.expand(-1, 3), diffuse=(1 - Fr) * albedo * E, tint=Fr * brgb, spec=spec)
    out = {}
    for k, X in per.items():
        s = torch.zeros(B, 3, dtype=torch.float64, device=app.device).index_add_(0, ray_id, w[:, None] * X)
        out[k] = s + (1 - acc)[:, None]                                        # white background
    return out


@pytest.mark.parametrize("name", ["e2e_full_eval", "e2e_g300_eval"])
def test_material_maps_vs_reference_eval_fixture(name):
    """albedo / roughness / diffuse against the reference's own evaluation forward (noise-independent maps), all five maps against a
    float64 restatement over the level-0 rows the pass recorded (spec and tint depend on the secondary rays' noise)"""
    from nmf_amd.noise import ReplayNoise
    g = Golden(name)
    nerf = _full_size_model(g)
    fp = _fused(nerf)
    pins = _pin_reference_bookkeeping(g)
    rays, focal = _fixture_rays(g)
    torch.manual_seed(g["noise_seed"])
    out = fp.render_chunk(rays.to(DEV), focal, ReplayNoise(DEV, None, pins=pins), want_maps=True, want_materials=True)
    assert len(out) == 7
    maps = out[-1]
    assert out[2] == g["n_rays"] and set(maps) == set(MAPS)
    for k in MAPS:
        assert maps[k].shape == (g["n_rays"], 3) and torch.isfinite(maps[k]).all(), k
    for k in ("albedo", "roughness"):
        assert_close(maps[k].cpu(), g["debug/" + k], rtol=1e-4, atol=1e-4, what=k)
    assert_close(maps["diffuse"].cpu(), g["debug/diffuse"], rtol=2e-3, atol=5e-4, what="diffuse")
    ref = _restate(pins.trace, fp.core())
    for k in MAPS:
        assert_close(maps[k].cpu(), ref[k].float().cpu(), rtol=1e-5, atol=2e-5, what=k + " (float64 restatement)")
    assert float(maps["spec"].std()) > 1e-3 and float((maps["tint"] - 1).abs().max()) > 1e-3      # not the background only


def test_material_maps_vs_module_path_and_invariance():
    """the fused maps against the operator graph's (render_images(draw_debug=True): the same field tables, heads and conv, another
    summation order), the other outputs bit-identical with the maps on or off, the maps bit-identical over two runs"""
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import render_images
    g = Golden("e2e_full_eval")
    nerf = _full_size_model(g)
    fp = _fused(nerf)
    rays, focal = _fixture_rays(g)
    rays = rays.to(DEV)
    run = lambda m: fp.render_chunk(rays, focal, DeviceNoise(torch.device(DEV), seed=5), want_maps=True, want_materials=m)  # noqa: E731
    off, on, again = run(False), run(True), run(True)
    assert len(off) == 6 and len(on) == 7
    for i in (0, 1, 4, 5):
        assert torch.equal(off[i], on[i]), i
    assert off[2] == on[2] and off[3] == on[3]
    for k in MAPS:
        assert torch.equal(on[-1][k], again[-1][k]), k
    mod = render_images(nerf, rays, focal, 4096, DeviceNoise(torch.device(DEV), seed=5), keys=MAPS, draw_debug=True)
    for k in ("albedo", "roughness", "diffuse"):
        assert_close(on[-1][k].cpu(), mod[k].cpu(), rtol=1e-5, atol=1e-5, what=k + " (module path)")


def test_render_images_routes_material_keys_to_the_fused_pass():
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import render_images
    g = Golden("e2e_g300_eval")
    nerf = _full_size_model(g)
    fp = _fused(nerf)
    rays, focal = _fixture_rays(g)
    calls = []
    orig = fp.render_chunk
    fp.render_chunk = lambda *a, **k: (calls.append(k.get("want_materials")), orig(*a, **k))[1]
    try:
        keys = ("rgb_map",) + MAPS
        ims = render_images(nerf, rays.to(DEV), focal, 1024, DeviceNoise(torch.device(DEV), seed=3), keys=keys)
    finally:
        fp.render_chunk = orig
    assert calls and all(calls)
    for k in keys:
        assert ims[k].shape == (g["n_rays"], 3), k
    assert_close(ims["albedo"].cpu(), g["debug/albedo"], rtol=1e-4, atol=1e-4, what="albedo (public route)")


def test_evaluation_writes_material_maps(tmp_path):
    from PIL import Image
    from nmf_amd import exr
    from nmf_amd.dataLoader import BlenderDataset
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import MATERIAL_KEYS, evaluation, map_to_8bit, render_images
    scene = tmp_path / "scene"
    _load_tool("make_blender_scene").main(["--out", str(scene), "--views", "1", "--test-views", "2", "--res", "64",
                                           "--grid", "32", "--bg", "32"])
    ds = BlenderDataset(str(scene), split="test", is_stack=True, N_vis=-1)
    nerf, _ = _s1_model()
    _fused(nerf)
    plain, out = tmp_path / "plain", tmp_path / "mm"
    evaluation(ds, nerf, None, None, str(plain), N_vis=-1, noise=DeviceNoise(torch.device(DEV), seed=21))
    evaluation(ds, nerf, None, None, str(out), N_vis=-1, noise=DeviceNoise(torch.device(DEV), seed=21), material_maps=True)
    listing = lambda p: sorted(os.path.relpath(os.path.join(r, f), p) for r, _, fs in os.walk(p) for f in fs)      # noqa: E731
    assert all(not os.path.exists(plain / d) for d in ("albedo", "roughness", "tint", "diffuse", "spec", "rgbd"))
    extra = set(listing(out)) - set(listing(plain))
    want = {f"{d}/{i:03d}.png" for d in ("albedo", "roughness", "tint", "diffuse") for i in range(2)}
    want |= {f"{d}/{i:03d}.exr" for d in ("spec", "rgbd") for i in range(2)}
    assert extra == want and set(listing(plain)) <= set(listing(out))
    noise = DeviceNoise(torch.device(DEV), seed=21)
    for i in range(2):
        ims = render_images(nerf, ds.all_rays[i].to(DEV), float(ds.fx), noise=noise,
                            keys=("rgb_map", "acc_map", "world_normal", "depth") + MATERIAL_KEYS)
        for k in ("albedo", "roughness", "tint", "diffuse"):
            png = np.asarray(Image.open(out / k / f"{i:03d}.png"))
            assert np.array_equal(png, map_to_8bit(ims[k].reshape(64, 64, 3).cpu().numpy())), (k, i)
        assert np.array_equal(exr.imread(str(out / "spec" / f"{i:03d}.exr")), ims["spec"].reshape(64, 64, 3).cpu().numpy())
        assert np.array_equal(exr.imread(str(out / "rgbd" / f"{i:03d}.exr"))[..., 0], ims["depth"].reshape(64, 64).cpu().numpy())
    assert float(ims["albedo"].std()) > 0


def test_render_eval_dir_material_maps_command_line(tmp_path, capsys, monkeypatch):
    from nmf_amd import render as R
    from nmf_amd import train as T
    scene = tmp_path / "tiny"
    _tiny_scene(scene)
    monkeypatch.chdir(tmp_path)
    ck = str(tmp_path / "out.th")
    T.main(["--datadir", str(scene), "--near-far", "2.5", "7", "--iters", "3", "--grid", "16", "--bg", "16", "--eval-every", "3",
            "--test-views", "1", "--save", ck])
    ev = tmp_path / "ev"
    rec = R.main(["--ckpt", ck, "--datadir", str(scene), "--eval-dir", str(ev), "--material-maps"])
    assert np.isfinite(rec["psnr"])
    for d, ext in (("albedo", "png"), ("roughness", "png"), ("tint", "png"), ("diffuse", "png"), ("spec", "exr"), ("rgbd", "exr")):
        for i in range(3):
            assert os.path.exists(ev / d / f"{i:03d}.{ext}"), (d, i)
    capsys.readouterr()
