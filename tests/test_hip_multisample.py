"""Multi-sample frames on the GPU (nmf_amd/multisample.py, csrc/accum.hip): nmf_camera_rays_at, nmf_accum_update,
nmf_accum_active and nmf_accum_resolve bit for bit against the numpy fp32 restatements of tests/test_multisample_cpu.py, one sample
through the accumulator against the pass's own rgb_map of nmf_ray_compose_fwd, and render_frame / evaluation_path / the command line
end to end on scene S1 (32 x 32 frames, the camera of tests/test_hip_camera_path.py)."""
import json
import os

import numpy as np
import pytest
import torch

from nmf_amd import camera_path as cp
from nmf_amd import hip
from test_camera_path_cpu import random_pose
from test_hip_metrics import _load_tool, _s1_model
from test_multisample_cpu import (PL_M2, PLANES, TILE, U, F, accum_active_np, accum_resolve_np, camera_rays_at_np, random_pass, run_passes,
                                  state_from_words, state_np, state_words)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAMES_HW = [(5, 7), (37, 53)]                    # 35 and 1961 pixels: neither a multiple of 64; the second spans eight workgroups


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


# ---- nmf_camera_rays_at ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FRAMES_HW)
def test_camera_rays_at_bit_identical_to_the_restatement(H, W):
    from nmf_amd.multisample import pass_offset
    rng = np.random.default_rng(H * 100 + W)
    P = H * W
    fx, fy, cx, cy = 111.25, 97.5, W / 2 + 1.75, H / 2 - 2.25
    c2w = random_pose(rng)
    lists = [None] + [np.sort(rng.choice(P, size=n, replace=False)).astype(np.int32) for n in sorted({min(n, P) for n in (0, 1, 63, 64, 65, 257)})]
    for k in range(4):                                                                   # passes 0 to 3, as render_frame calls them
        (jx, jy), seed = pass_offset(k), k
        for pix in lists:
            n = P if pix is None else len(pix)
            got = hip.camera_rays_at(c2w, fx, fy, cx, cy, H, W, jitter=(jx, jy), seed=seed, pix=None if pix is None else _dev(pix), device=DEV)
            assert got.shape == (n, 6) and got.dtype == torch.float32
            want = camera_rays_at_np(c2w, fx, fy, cx, cy, H, W, jx, jy, seed, pix)
            assert np.array_equal(_bits(got), want.view(np.uint32)), (k, n)
            again = hip.camera_rays_at(c2w, fx, fy, cx, cy, H, W, jitter=(jx, jy), seed=seed, pix=None if pix is None else _dev(pix),
                                       out=torch.full((n + 3, 6), 7.0, device=DEV))
            assert torch.equal(got, again)                                               # two runs, the same bytes
        if k == 0:                                                                       # the anchor: the bytes of nmf_camera_rays
            full = hip.camera_rays_at(c2w, fx, fy, cx, cy, H, W, device=DEV)
            assert torch.equal(full, hip.camera_rays(c2w, fx, fy, cx, cy, H, W, device=DEV))
        else:
            assert not torch.equal(hip.camera_rays_at(c2w, fx, fy, cx, cy, H, W, jitter=(jx, jy), seed=seed, device=DEV)[:, 3:],
                                   hip.camera_rays(c2w, fx, fy, cx, cy, H, W, device=DEV)[:, 3:])
    # ids outside the frame: those rows keep the sentinel, and so does everything past the list
    pix = np.array([-1, 0, P - 1, P, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    buf = torch.full((len(pix) + 64, 6), -77.0, device=DEV)
    hip.camera_rays_at(c2w, fx, fy, cx, cy, H, W, jitter=(0.25, 0.75), seed=5, pix=_dev(pix), out=buf)
    want = camera_rays_at_np(c2w, fx, fy, cx, cy, H, W, 0.25, 0.75, 5, pix, out=np.full((len(pix), 6), -77.0, dtype=F))
    assert np.array_equal(_bits(buf[:len(pix)]), want.view(np.uint32)) and (buf[len(pix):] == -77.0).all()
    assert (buf[[0, 3, 4, 5]] == -77.0).all() and (buf[[1, 2]] != -77.0).all()


# ---- nmf_accum_update ------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _guarded_state(P, words=None):
    """a zeroed (or given) state between two bands of GUARD sentinel floats -> (the whole buffer, the state's view)"""
    n = hip.accum_state_bytes(1, P) // 4
    buf = torch.full((n + 2 * GUARD,), -12345.0, device=DEV)
    st = buf[GUARD:GUARD + n]
    if words is None:
        st.zero_()
    else:
        st.copy_(_dev(np.asarray(words).view(F)))
    return buf, st


def _guards_intact(buf):
    return bool((buf[:GUARD] == -12345.0).all()) and bool((buf[-GUARD:] == -12345.0).all())


@pytest.mark.parametrize("with_maps", [True, False])
def test_accum_update_bit_identical_over_17_passes(with_maps):
    H, W = 37, 53
    P = H * W
    buf, st = _guarded_state(P)

    def on_pass(k, pix, inputs):
        lin, acc, mp, depth, nm = (_dev(a) for a in inputs)
        hip.accum_update(st, H, W, lin, acc, mp, depth if with_maps else None, nm if with_maps else None,
                         pix=None if k == 0 else _dev(pix))                                # (pass 0: the null list; pass 5: the full one as a list)
    want = run_passes(P, 17, seed=11, with_maps=with_maps, record=on_pass)
    got = state_from_words(st.cpu().numpy(), P)
    assert np.array_equal(got["count"], want["count"])                                   # as integers
    assert np.array_equal(got["planes"].view(np.uint32), want["planes"].view(np.uint32))
    assert _guards_intact(buf)
    if not with_maps:
        assert not got["planes"][4:8].any()                                              # depth and normal means were left alone
    # ids outside the frame are skipped (nothing moves), an empty list launches nothing
    before = buf.clone()
    bad = _dev(np.array([-1, P, P + 5, 2 ** 31 - 1], dtype=np.int32))
    lin, acc, mp, depth, nm = (_dev(a) for a in random_pass(np.random.default_rng(0), 4))
    hip.accum_update(st, H, W, lin, acc, mp, depth, nm, pix=bad)
    hip.accum_update(st, H, W, lin[:0], acc[:0], mp[:0], pix=bad[:0])
    assert torch.equal(buf, before)


def test_one_full_pass_leaves_the_inputs_bits():
    H, W = 37, 53
    P = H * W
    buf, st = _guarded_state(P)
    inputs = random_pass(np.random.default_rng(3), P)
    hip.accum_update(st, H, W, *(_dev(a) for a in inputs))
    got = state_from_words(st.cpu().numpy(), P)
    lin, acc, mp, depth, nm = inputs
    pl = got["planes"]
    assert (got["count"] == 1).all() and not pl[11:14].any() and _guards_intact(buf)
    for a, b in ((pl[0:3].T, lin), (pl[3], acc), (pl[4], depth), (pl[5:8].T, nm), (pl[8:11].T, mp)):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    out = hip.accum_resolve(st, H, W, tonemap=False, bg=(0.0, 0.0, 0.0))
    assert np.array_equal(_bits(out["acc"]), acc.view(np.uint32)) and np.array_equal(_bits(out["depth"]), depth.view(np.uint32))
    assert np.array_equal(_bits(out["normal"]), nm.view(np.uint32)) and (out["se"] == 0).all() and (out["count"] == 1).all()


# ---- nmf_accum_active ------------------------------------------------------------------------------------------------------------------
# The scan tile is NMF_ACCUM_TILE = 256 pixels (one workgroup) and the scan walks 256 tiles per round: 70001 pixels are 274 tiles,
# so the frame crosses a tile edge 273 times and the scan runs a second round with a carry.
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 4097, 70001])
def test_accum_active_equals_flatnonzero(P):
    assert TILE == 256 and (P != 70001 or (P // TILE >= 2 and -(-P // TILE) > 256))
    rng = np.random.default_rng(P)
    ids = np.arange(P)
    patterns = dict(all=np.ones(P, bool), none=np.zeros(P, bool), alternating=ids % 2 == 1, last=ids == P - 1, random=rng.random(P) < 0.1)
    for name, on in patterns.items():
        # written into the state directly: an active pixel is either short of min_spp or has four samples and M2 = 1 in one channel
        # (se = sqrt(1 / 12)); the others have four samples and M2 = 0, or are at max_spp with a large M2
        st = state_np(P)
        short = on & (rng.random(P) < 0.5)
        st["count"][:] = np.where(short, rng.integers(0, 4, size=P), 4)
        done = ~on & (rng.random(P) < 0.3)
        st["count"][done] = 16
        ch = rng.integers(0, 3, size=P)
        st["planes"][PL_M2 - 1 + ch, ids] = np.where((on & ~short) | done, 1.0, 0.0).astype(F)
        want = accum_active_np(st, 4, 16, 0.01)
        assert np.array_equal(want, np.flatnonzero(on)), name
        buf, dev_state = _guarded_state(P, state_words(st, P))
        lst, n = hip.accum_active(dev_state, 1, P, 4, 16, 0.01, out=torch.full((P,), -7, dtype=torch.int32, device=DEV))
        assert int(n.item()) == len(want), name                                          # the length
        assert np.array_equal(lst.cpu().numpy()[:len(want)], want), name                 # as integers
        assert (lst[len(want):] == -7).all(), name                                       # nothing past the list
        lst2, n2 = hip.accum_active(dev_state, 1, P, 4, 16, 0.01, out=torch.full((P,), -7, dtype=torch.int32, device=DEV))
        assert torch.equal(lst, lst2) and torch.equal(n, n2), name                       # two runs, the same bytes
        assert _guards_intact(buf)
        assert np.array_equal(dev_state.cpu().numpy().view(np.uint32)[:PLANES * P], state_words(st, P)[:PLANES * P])     # the planes are only read
    # the tolerance's ends on the last pattern's state: 0 keeps every pixel with M2 > 0 below max_spp, +inf none of them
    for tol in (0.0, float("inf")):
        lst, n = hip.accum_active(dev_state, 1, P, 4, 16, tol)
        assert np.array_equal(lst.cpu().numpy()[:int(n.item())], accum_active_np(st, 4, 16, tol))


# ---- nmf_accum_resolve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tonemap", [True, False])
@pytest.mark.parametrize("noclip", [True, False])
def test_accum_resolve_bit_identical_to_the_restatement(tonemap, noclip):
    H, W = 37, 53
    P = H * W
    st = run_passes(P, 17, seed=13)
    st["planes"][0, :6] = [0.0, 0.0031308, np.nextafter(F(0.0031308), F(1)), 1.0, 1.5, -0.25]      # the knee, the clip, a negative radiance
    buf, dev_state = _guarded_state(P, state_words(st, P))
    bg = (1.0, 0.5, 0.25)
    got = hip.accum_resolve(dev_state, H, W, bg=bg, tonemap=tonemap, noclip=noclip)
    want = accum_resolve_np(st, bg, tonemap, noclip)
    for k in ("rgb_map", "acc", "depth", "normal", "se", "count"):
        assert np.array_equal(_bits(got[k]), np.ascontiguousarray(want[k]).view(np.uint32)), k
    assert _guards_intact(buf) and (got["se"] > 0).all()
    only = hip.accum_resolve(dev_state, H, W, want=("se",))
    assert set(only) == {"se"} and torch.equal(only["se"], got["se"])
    with pytest.raises(hip.NmfHipError):
        hip.accum_resolve(dev_state, H, W, want=("albedo",))


@pytest.mark.parametrize("tonemap", [True, False])
@pytest.mark.parametrize("noclip", [True, False])
def test_one_sample_against_the_pass_own_rgb_map(tonemap, noclip):
    """One pass of nmf_ray_compose_fwd folded in and resolved: rgb_lin and acc come back as the pass's bits, so rgb_map differs from the
    pass's own only by the roundings the two kernels take differently (u = 2^-24, one rounding's relative error).  shade.hip is built
    with contraction on and uses powf; accum.hip takes no fma and the correctly rounded power.  With x = rgb_lin, p = x^(1/2.4),
    o = 1.055 p - 0.055, t = 1 - acc (one subtraction in both: the same bits), r = o + t bg:
      the power     powf is within 1 ulp = 2 u p (HIP's documented bound), the rounded double power within u p: 3 u p apart, times 1.055
      o             accum rounds the product and the difference (u 1.055 p + u |o|); compose does the same or, fused, rounds once
                    (u |o|): at most 2 (u 1.055 p + u |o|) apart
      the clip      monotone, moves nothing apart
      r             accum rounds t bg and the sum (u |t bg| + u |r|), compose the same or one fma (u |r|): 2 (u |t bg| + u |r|) apart
    Below the knee and without the tonemap o is one product or x itself in both: only the last line applies."""
    rng = np.random.default_rng(17)
    B = 1500
    counts = rng.integers(0, 40, size=B)
    counts[:10] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    M = int(offsets[-1])
    w = (rng.random(M) / np.repeat(np.maximum(counts, 1), counts) * rng.uniform(0.2, 1.0, size=B).repeat(counts)).astype(F)
    refl = rng.uniform(0, 1.6, size=(M, 3)).astype(F)
    refl *= np.where(rng.random(B) < 0.2, F(0.001), F(1)).astype(F).repeat(counts)[:, None]      # rays whose sums lie under the knee
    rays = rng.normal(size=(B, 6)).astype(F)
    bg = np.array([[1.0, 0.5, 0.25]], dtype=F)
    rgb_map, acc, lin, _ = hip.ray_compose_fwd(_dev(w), _dev(refl), _dev(np.arange(M, dtype=np.int32)), None, _dev(rays), _dev(offsets), B,
                                               _dev(bg), False, tonemap, noclip, False)
    buf, st = _guarded_state(B)
    hip.accum_update(st, 1, B, lin, acc, rgb_map)
    got = hip.accum_resolve(st, 1, B, bg=tuple(float(v) for v in bg[0]), tonemap=tonemap, noclip=noclip)
    state = state_from_words(st.cpu().numpy(), B)
    assert np.array_equal(state["planes"][0:3].T.copy().view(np.uint32), _bits(lin)) and np.array_equal(_bits(got["acc"]), _bits(acc))
    assert np.array_equal(state["planes"][8:11].T.copy().view(np.uint32), _bits(rgb_map)) and _guards_intact(buf)
    x = lin.cpu().numpy().astype(np.float64)
    t_bg = np.abs((1.0 - acc.cpu().numpy().astype(np.float64))[:, None] * bg.astype(np.float64))
    r = np.abs(rgb_map.cpu().numpy().astype(np.float64))
    bound = 2 * U * (t_bg + r)
    if tonemap:
        p = np.power(np.maximum(x, 0.0031308), 1.0 / 2.4)
        o = np.abs(1.055 * p - 0.055)
        bound = bound + np.where(x > float(F(0.0031308)), U * (3 * 1.055 * p + 2 * (1.055 * p + o)), 0.0)
    diff = np.abs(got["rgb_map"].cpu().numpy().astype(np.float64) - rgb_map.cpu().numpy().astype(np.float64))
    print(f"tonemap {tonemap} noclip {noclip}: largest |resolve - compose| = {diff.max() / U:.2f} u, largest share of its bound "
          f"{(diff / bound).max():.3f}; {int((diff == 0).sum())} of {diff.size} equal")
    assert (x > 0.0031308).any() and (x <= 0.0031308).any() and (diff <= bound).all()


# ---- end to end on S1 ------------------------------------------------------------------------------------------------------------------
RES, SEED = 32, 21
CAMERA = dict(w=RES, h=RES, fx=46.5, fy=46.5, cx=RES / 2, cy=RES / 2, near_far=[2.5, 7.0])
KEYS = ("rgb_map", "acc_map", "depth", "world_normal")


@pytest.fixture(scope="module")
def model():
    return _s1_model()


def _noise():
    from nmf_amd.noise import DeviceNoise
    return DeviceNoise(torch.device(DEV), seed=SEED)


def _pose():
    return cp.orbit(3, (0, 0, 0), 4.0, 30.0)[0]


@pytest.fixture(scope="module")
def frames(model):
    """the S1 view of the first orbit pose at 32 x 32 under every sampling rule the tests look at, each from a fresh DeviceNoise of the
    seed: name -> (ims, stats) with the maps as numpy arrays"""
    from nmf_amd.multisample import render_frame
    nerf, _ = model
    rules = dict(fixed8=dict(spp=8, tol=None), fixed16=dict(spp=16, tol=None), fixed4=dict(spp=4, tol=None),
                 adaptive=dict(spp=16, min_spp=4, tol=1 / 255), tol0=dict(spp=16, min_spp=4, tol=0.0),
                 tolinf=dict(spp=16, min_spp=4, tol=float("inf")))
    out = {}
    for name, kw in rules.items():
        ims, stats = render_frame(nerf, _pose(), CAMERA, noise=_noise(), keys=KEYS, **kw)
        out[name] = ({k: v.cpu().numpy() for k, v in ims.items()}, stats)
    return out


def _run_path(model, out, **kw):
    from nmf_amd.renderer import evaluation_path
    return evaluation_path(None, model[0], cp.orbit(2, (0, 0, 0), 4.0, 30.0), None, str(out), noise=_noise(), panels=("rgb", "depth"),
                           camera=CAMERA, **kw)


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for nm in names:
            with open(os.path.join(d, nm), "rb") as f:
                out[os.path.relpath(os.path.join(d, nm), root)] = f.read()
    return out


def test_spp_1_is_todays_path(model, tmp_path):
    res_a = _run_path(model, tmp_path / "a")
    res_b = _run_path(model, tmp_path / "b", spp=1)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert set(a) == set(b) == {"000.png", "001.png", "depth/000.png", "depth/001.png", "video.png", "depthvideo.png", "transforms_path.json"}
    assert all(a[k] == b[k] for k in a)
    assert set(res_a) == set(res_b) and "rays_rendered" not in res_b


def test_fixed_count(frames):
    ims, stats = frames["fixed8"]
    assert (ims["count"] == 8).all() and stats == dict(passes=8, rays_rendered=8 * RES * RES)
    assert set(ims) == set(KEYS) | {"se", "count"}
    assert ims["rgb_map"].shape == (RES * RES, 3) and ims["world_normal"].shape == (RES * RES, 3) and ims["depth"].shape == (RES * RES,)
    assert all(np.isfinite(v).all() for v in ims.values()) and ims["rgb_map"].std() > 0.02


def test_background_pixels_stop_at_min_spp(frames):
    for name in ("fixed8", "fixed16", "adaptive"):
        ims, _ = frames[name]
        empty = ims["acc_map"] == 0                                                      # acc >= 0: a zero mean is zero in every pass
        assert empty.sum() >= 16 and (ims["se"][empty] == 0).all(), name
        assert (ims["rgb_map"][empty] == 1).all(), name                                  # the white background, exactly
    ims, _ = frames["adaptive"]
    assert (ims["count"][ims["acc_map"] == 0] == 4).all()
    assert set(np.unique(ims["count"])) <= set(range(4, 17))


def test_tolerance_ends(frames):
    ims, stats = frames["tol0"]
    assert (ims["count"][ims["se"] > 0] == 16).all() and (ims["count"][ims["se"] == 0] == 4).all() and (ims["se"] > 0).sum() > RES * RES // 2
    assert stats["passes"] == 16 and stats["rays_rendered"] == int(ims["count"].sum())
    ims, stats = frames["tolinf"]
    assert (ims["count"] == 4).all() and stats == dict(passes=4, rays_rendered=4 * RES * RES)


def test_adaptive_work_is_below_the_fixed_count(frames):
    ims, stats = frames["adaptive"]
    assert stats["rays_rendered"] == int(ims["count"].sum()) < 16 * RES * RES
    assert 4 <= stats["passes"] <= 16
    done = ims["count"] < 16
    assert (ims["se"][done] <= F(1 / 255)).all()                                         # a pixel that stopped early met the tolerance
    print("adaptive:", stats, "mean count", float(ims["count"].mean()), "mean se x 255", float(ims["se"].mean() * 255))


def test_standard_error_falls_as_one_over_sqrt_n(frames):
    """se at 16 fixed samples over se at 4: sqrt(4 / 16) = 0.5 expected.  A 4-sample se scatters by about 41 % per pixel; the median
    over 200 or more pixels tightens that to a few percent, so [0.35, 0.7] is more than five of those wide."""
    (a, _), (b, _) = frames["fixed16"], frames["fixed4"]
    sel = (a["acc_map"] > 0.5) & (b["se"] > 0)
    assert sel.sum() >= 200, int(sel.sum())
    ratio = float(np.median(a["se"][sel] / b["se"][sel]))
    print(f"{int(sel.sum())} pixels, median se_16 / se_4 = {ratio:.4f}; mean se_4 x 255 = {float(b['se'][sel].mean() * 255):.3f}, "
          f"mean se_16 x 255 = {float(a['se'][sel].mean() * 255):.3f}")
    assert 0.35 <= ratio <= 0.7


def test_composed_and_relit_models_render(model):
    from nmf_amd import relight
    from nmf_amd.compose import ComposedScene, Placement
    from nmf_amd.multisample import render_frame
    nerf, _ = model
    scene = ComposedScene([(nerf, Placement.identity())], near_far=tuple(nerf.sampler.near_far))
    shapes = dict(rgb_map=(RES * RES, 3), acc_map=(RES * RES,), depth=(RES * RES,), world_normal=(RES * RES, 3), se=(RES * RES,),
                  count=(RES * RES,))
    ims, stats = render_frame(scene, _pose(), CAMERA, spp=2, noise=_noise(), keys=KEYS)
    assert {k: tuple(v.shape) for k, v in ims.items()} == shapes and all(bool(torch.isfinite(v).all()) for v in ims.values())
    assert stats == dict(passes=2, rays_rendered=2 * RES * RES) and float(ims["acc_map"].max()) > 0.5
    with relight.relit(nerf, relight.rotate_env(nerf.bg_module, relight.rotation(90.0))) as n:
        lit, stats = render_frame(n, _pose(), CAMERA, spp=2, noise=_noise(), keys=KEYS)
    assert {k: tuple(v.shape) for k, v in lit.items()} == shapes and all(bool(torch.isfinite(v).all()) for v in lit.values())
    assert stats["passes"] == 2 and (lit["count"] == 2).all()
    # a data set's rays: the same pixels without jitter, through rays[pix]
    rays = hip.camera_rays(_pose(), CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"], RES, RES, device=DEV)
    own, stats = render_frame(nerf, rays, CAMERA["fx"], spp=6, min_spp=2, tol=1 / 255, jitter=False, noise=_noise(), keys=("rgb_map", "rgb_lin"))
    assert set(own) == {"rgb_map", "rgb_lin", "se", "count"} and stats["rays_rendered"] == int(own["count"].sum()) < 6 * RES * RES
    with pytest.raises(ValueError):
        render_frame(nerf, rays, CAMERA["fx"], spp=2)                                    # jitter needs a pose


def test_evaluation_with_spp_writes_the_sample_maps(model, tmp_path):
    from PIL import Image
    from nmf_amd.dataLoader import BlenderDataset
    from nmf_amd.renderer import evaluation
    scene = tmp_path / "scene"
    _load_tool("make_blender_scene").main(["--out", str(scene), "--views", "1", "--test-views", "1", "--res", "32", "--grid", "32", "--bg", "32"])
    ds = BlenderDataset(str(scene), split="test", is_stack=True, N_vis=-1)
    out = tmp_path / "imgs"
    res = evaluation(ds, model[0], None, None, str(out), N_vis=-1, noise=_noise(), spp=4, min_spp=2, tol=1 / 255)
    assert len(res["psnrs"]) == 1 and np.isfinite(res["psnrs"][0])
    for sub in ("", "spp", "noise", "world_normal", "acc_map"):
        assert np.asarray(Image.open(out / sub / "000.png")).shape[:2] == (32, 32), sub
    assert np.asarray(Image.open(out / "spp" / "000.png")).max() == 255
    with pytest.raises(ValueError):
        evaluation(ds, model[0], None, None, str(out), N_vis=-1, spp=2, material_maps=True)


def test_command_line_with_spp(model, tmp_path, capsys):
    from PIL import Image
    from nmf_amd import render as R
    nerf, cfg = model
    ck = str(tmp_path / "m.th")
    nerf.save(ck, cfg["arch"])
    a = tmp_path / "a"
    rec = R.main(["--ckpt", ck, "--views", "1", "--res", str(RES), "--path", "orbit", "--frames", "2", "--spp", "4", "--adaptive", "1",
                  "--out", str(a)])
    line = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    assert line == json.loads(json.dumps(rec)) and rec["sampling"] == dict(spp=4, min_spp=4, adaptive=1.0)
    p = rec["path"]
    assert p["frames"] == 2 and p["passes"] == [4, 4] and p["rays_rendered"] == [4 * RES * RES] * 2
    files = _files(a / "path")
    assert set(files) == ({f"{d}{k:03d}.png" for d in ("", "depth/", "spp/", "noise/") for k in range(2)}
                          | {"video.png", "depthvideo.png", "transforms_path.json"})
    assert Image.open(a / "path" / "video.png").n_frames == 2 and os.path.exists(a / "000.png")
    assert np.asarray(Image.open(a / "path" / "spp" / "000.png")).shape == (RES, RES, 3)
    rec = R.main(["--ckpt", ck, "--views", "1", "--res", str(RES), "--path", "orbit", "--frames", "2", "--spp", "6", "--adaptive", "1",
                  "--min-spp", "2", "--out", str(tmp_path / "b")])
    capsys.readouterr()
    assert all(2 * RES * RES < n < 6 * RES * RES for n in rec["path"]["rays_rendered"]) and rec["sampling"]["min_spp"] == 2
    # the views and the light turntable take the same sampling through their own rays (no jitter)
    c = tmp_path / "c"
    rec = R.main(["--ckpt", ck, "--views", "2", "--res", str(RES), "--spp", "3", "--light-turntable", "2", "--out", str(c)])
    capsys.readouterr()
    assert rec["sampling"] == dict(spp=3, min_spp=3, adaptive=None) and rec["frames"] == 2 and rec["light_frames"] == 2
    assert sorted(os.listdir(c)) == ["000.png", "001.png", "light_000.png", "light_001.png"]
    assert np.asarray(Image.open(c / "000.png")).std() > 5
