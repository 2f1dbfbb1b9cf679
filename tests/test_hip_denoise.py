"""Denoised frames on the GPU (nmf_amd/multisample.py, csrc/denoise.hip): nmf_denoise and its three stages bit for
bit against denoise_np of tests/test_denoise_cpu.py, and render_frame / evaluation_path / evaluation / the command line with denoise
end to end on scene S1 (32 x 32 frames, the camera and fixtures of tests/test_hip_multisample.py's kind)."""
import json
import os

import numpy as np
import pytest
import torch

from nmf_amd import camera_path as cp
from nmf_amd import hip
from test_denoise_cpu import DEFAULTS, WIDE, WS_PLANES, denoise_finish_np, denoise_level_np, denoise_np, denoise_prepare_np, mixed_state
from test_hip_metrics import _load_tool, _s1_model
from test_multisample_cpu import PL_M2, F, accum_resolve_np, state_words

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = -12345.0
FRAMES_HW = [(1, 1), (5, 7), (37, 53)]            # 1, 35 and 1961 pixels: the last two no multiple of 64, the last eight workgroups
BG = (1.0, 0.5, 0.25)
OUTPUTS = ("rgb_map", "rgb_lin", "acc", "se")


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def _guarded(n, fill=None):
    """n floats between two bands of GUARD sentinels -> (the whole buffer, the view)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(DEV))
    return buf, view


def _intact(*bufs):
    return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()) for b in bufs)


def _states(H, W):
    """the mixed state of the CPU tests (counts 0 to 3, NaNs were planted in one pass); for one pixel also a state that is not fixed"""
    out = [mixed_state(H, W, seed=10 * H + W)]
    if H * W == 1:
        st = mixed_state(5, 7, seed=1)
        one = dict(count=np.array([3], dtype=np.int32), planes=st["planes"][:, 5:6].copy())
        one["planes"][PL_M2 - 1:PL_M2 + 2, 0] = [0.3, 0.1, 0.2]
        out.append(one)
    return out


@pytest.mark.parametrize("levels", [0, 1, 3, 5])                                          # steps up to 16: beyond the two small frames
@pytest.mark.parametrize("H,W", FRAMES_HW)
def test_denoise_bit_identical_to_the_restatement(H, W, levels):
    P = H * W
    for st in _states(H, W):
        sbuf, state = _guarded(hip.accum_state_bytes(H, W) // 4, state_words(st, P).view(F))
        before = sbuf.clone()
        for widths in ({}, WIDE):
            prm = dict(DEFAULTS, **widths, levels=levels)
            wbuf, ws = _guarded(hip.denoise_workspace_bytes(H, W) // 4)
            obufs, out = {}, {}
            for k in OUTPUTS:
                obufs[k], out[k] = _guarded(3 * P if k in ("rgb_map", "rgb_lin") else P)
            got = hip.denoise(state, H, W, bg=BG, tonemap=True, noclip=False, want=OUTPUTS, workspace=ws, out=out, **prm)
            want = denoise_np(st, H, W, bg=BG, tonemap=True, noclip=False, **prm)
            for k in OUTPUTS:
                assert got[k].data_ptr() == out[k].data_ptr()
                assert np.array_equal(_bits(got[k]).reshape(-1), _bits(want[k]).reshape(-1)), (k, widths, levels)
            assert _intact(sbuf, wbuf, *obufs.values()) and torch.equal(sbuf, before)      # the state is only read
            # the other flags of the displayed colour, from the workspace as it stands
            for tonemap, noclip in ((True, True), (False, False), (False, True)):
                fin = hip.denoise_finish(ws, H, W, levels & 1, bg=BG, tonemap=tonemap, noclip=noclip)
                ref = denoise_np(st, H, W, bg=BG, tonemap=tonemap, noclip=noclip, **prm)
                assert set(fin) == {"rgb_map"} and np.array_equal(_bits(fin["rgb_map"]), _bits(ref["rgb_map"])), (tonemap, noclip)
            # two runs, the same bytes (new outputs, the same workspace)
            again = hip.denoise(state, H, W, bg=BG, want=OUTPUTS, workspace=ws, **prm)
            assert all(torch.equal(again[k].reshape(-1), got[k].reshape(-1)) for k in OUTPUTS) and _intact(wbuf)
            if levels == 0:                                                              # the resolved frame's bytes
                raw = hip.accum_resolve(state, H, W, bg=BG, want=("rgb_map", "acc"))
                assert torch.equal(raw["rgb_map"].reshape(-1), got["rgb_map"].reshape(-1)) and torch.equal(raw["acc"], got["acc"].reshape(-1))
                assert np.array_equal(_bits(raw["rgb_map"]), _bits(accum_resolve_np(st, BG)["rgb_map"]))


@pytest.mark.parametrize("H,W", FRAMES_HW[1:])
def test_the_stages_one_by_one(H, W):
    """prepare's planes, every level's set (steps 1, 2, 16: the last with every tap off the 5 x 7 frame) and finish, each against
    its own restatement, with the guards of the workspace checked after every launch"""
    P = H * W
    st = mixed_state(H, W, seed=H)
    prm = {k: v for k, v in dict(DEFAULTS, **WIDE).items() if k != "levels"}
    sbuf, state = _guarded(hip.accum_state_bytes(H, W) // 4, state_words(st, P).view(F))
    wbuf, ws = _guarded(hip.denoise_workspace_bytes(H, W) // 4)
    hip.denoise_prepare(state, ws, H, W)
    ref = denoise_prepare_np(st, H, W)
    planes = ws.cpu().numpy().reshape(WS_PLANES, P)
    assert np.array_equal(planes[0].view(np.int32), ref["fixed"].astype(np.int32)) and 0 < ref["fixed"].sum() < P
    assert np.array_equal(_bits(planes[1]), _bits(ref["gx"])) and np.array_equal(_bits(planes[2]), _bits(ref["gy"]))
    assert np.array_equal(_bits(planes[3:11]), _bits(ref["set"])) and _intact(wbuf, sbuf)
    s, src = ref["set"], 0
    for step in (1, 2, 16):
        hip.denoise_level(state, ws, H, W, step, src, **prm)
        nxt = denoise_level_np(st, ref, H, W, step, src=s, **prm)
        planes = ws.cpu().numpy().reshape(WS_PLANES, P)
        lo = 3 + 8 * (1 - src)
        assert np.array_equal(_bits(planes[lo:lo + 8]), _bits(nxt)), step
        assert np.array_equal(_bits(planes[3 + 8 * src:11 + 8 * src]), _bits(s)) and _intact(wbuf, sbuf)      # the source set is only read
        if (H, W) == (5, 7) and step == 16:
            assert np.array_equal(_bits(nxt), _bits(s))
        else:
            assert not np.array_equal(_bits(nxt), _bits(s))
        s, src = nxt, 1 - src
    fin = hip.denoise_finish(ws, H, W, src, bg=BG, tonemap=True, noclip=True, want=("rgb_lin", "se"))
    want = denoise_finish_np(s, BG, True, True)
    assert set(fin) == {"rgb_lin", "se"} and all(np.array_equal(_bits(fin[k]), _bits(want[k])) for k in fin) and _intact(wbuf)
    with pytest.raises(hip.NmfHipError):
        hip.denoise_finish(ws, H, W, src, want=("albedo",))
    with pytest.raises(hip.NmfHipError):
        hip.denoise_level(state, ws, H, W, 0, 0, **prm)
    with pytest.raises(hip.NmfHipError):
        hip.denoise_prepare(state, ws[:-1], H, W)


# ---- end to end on S1 ------------------------------------------------------------------------------------------------------------------
RES, SEED = 32, 21
CAMERA = dict(w=RES, h=RES, fx=46.5, fy=46.5, cx=RES / 2, cy=RES / 2, near_far=[2.5, 7.0])


@pytest.fixture(scope="module")
def model():
    return _s1_model()


def _noise():
    from nmf_amd.noise import DeviceNoise
    return DeviceNoise(torch.device(DEV), seed=SEED)


def _pose():
    return cp.orbit(3, (0, 0, 0), 4.0, 30.0)[0]


def _params(**kw):
    from nmf_amd.multisample import DenoiseParams
    return DenoiseParams(**kw)


def _run_path(model, out, **kw):
    from nmf_amd.renderer import evaluation_path
    return evaluation_path(None, model[0], cp.orbit(2, (0, 0, 0), 4.0, 30.0), None, str(out), noise=_noise(), panels=("rgb", "depth", "normal"),
                           camera=CAMERA, **kw)


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for nm in names:
            with open(os.path.join(d, nm), "rb") as f:
                out[os.path.relpath(os.path.join(d, nm), root)] = f.read()
    return out


def test_a_path_without_denoise_and_with_zero_levels_writes_the_same_files(model, tmp_path):
    """denoise=None is the frame as it was (nothing new runs); zero levels run prepare and finish and give the resolved frame's bytes,
    so every file of the path is the same; five levels change the frames and leave depth/, world_normal/, spp/ and noise/ alone"""
    res_a = _run_path(model, tmp_path / "a", spp=4)
    res_b = _run_path(model, tmp_path / "b", spp=4, denoise=_params(levels=0))
    res_c = _run_path(model, tmp_path / "c", spp=4, denoise=_params(levels=5))
    a, b, c = _files(tmp_path / "a"), _files(tmp_path / "b"), _files(tmp_path / "c")
    assert set(a) == set(b) == set(c) and len(a) == 2 * 5 + 3
    assert all(a[k] == b[k] for k in a)
    same = [k for k in a if a[k] == c[k]]
    assert {k for k in a if k.split("/")[0] in ("spp", "noise", "depth", "world_normal")} | {"transforms_path.json", "depthvideo.png"} == set(same)
    assert res_a["rays_rendered"] == res_b["rays_rendered"] == res_c["rays_rendered"] == [4 * RES * RES] * 2
    with pytest.raises(ValueError):
        _run_path(model, tmp_path / "d", spp=1, denoise=_params())


def test_render_frame_with_denoise(model):
    from nmf_amd.multisample import render_frame
    nerf, _ = model
    keys = ("rgb_map", "rgb_raw", "rgb_lin", "acc_map", "depth", "world_normal")
    plain, _ = render_frame(nerf, _pose(), CAMERA, spp=4, noise=_noise(), keys=tuple(k for k in keys if k != "rgb_raw"))
    ims, stats = render_frame(nerf, _pose(), CAMERA, spp=4, noise=_noise(), keys=keys, denoise=_params())
    assert stats == dict(passes=4, rays_rendered=4 * RES * RES) and set(ims) == set(keys) | {"se", "count"}
    assert all(bool(torch.isfinite(v).all()) for v in ims.values())
    assert torch.equal(ims["rgb_raw"], plain["rgb_map"])
    for k in ("se", "count", "acc_map", "depth", "world_normal"):                        # the measured maps stay the measured ones
        assert torch.equal(ims[k], plain[k]), k
    still = ims["se"] == 0
    assert int(still.sum()) >= 16 and torch.equal(ims["rgb_map"][still], plain["rgb_map"][still])
    assert torch.equal(ims["rgb_lin"][still], plain["rgb_lin"][still])
    moved = (ims["rgb_map"] != plain["rgb_map"]).any(-1)
    assert int(moved.sum()) > 0 and not bool((moved & still).any())
    print(f"{int(moved.sum())} of {int((~still).sum())} pixels with se > 0 moved; mean |denoised - raw| x 255 = "
          f"{float((ims['rgb_map'] - plain['rgb_map']).abs().mean() * 255):.3f}")
    # a data set's rays need the frame's shape
    rays = hip.camera_rays(_pose(), CAMERA["fx"], CAMERA["fy"], CAMERA["cx"], CAMERA["cy"], RES, RES, device=DEV)
    own, _ = render_frame(nerf, rays, CAMERA["fx"], spp=2, jitter=False, noise=_noise(), denoise=_params(levels=2), frame_hw=(RES, RES))
    assert set(own) == {"rgb_map", "se", "count"} and bool(torch.isfinite(own["rgb_map"]).all())
    with pytest.raises(ValueError):
        render_frame(nerf, rays, CAMERA["fx"], spp=2, jitter=False, noise=_noise(), denoise=_params())
    with pytest.raises(ValueError):
        render_frame(nerf, _pose(), CAMERA, spp=1, noise=_noise(), denoise=_params())


def test_composed_and_relit_models_render_denoised(model):
    from nmf_amd import relight
    from nmf_amd.compose import ComposedScene, Placement
    from nmf_amd.multisample import render_frame
    nerf, _ = model
    scene = ComposedScene([(nerf, Placement.identity())], near_far=tuple(nerf.sampler.near_far))
    ims, stats = render_frame(scene, _pose(), CAMERA, spp=2, noise=_noise(), keys=("rgb_map", "rgb_raw"), denoise=_params())
    assert ims["rgb_map"].shape == (RES * RES, 3) and bool(torch.isfinite(ims["rgb_map"]).all()) and stats["passes"] == 2
    assert not torch.equal(ims["rgb_map"], ims["rgb_raw"])
    with relight.relit(nerf, relight.rotate_env(nerf.bg_module, relight.rotation(90.0))) as n:
        lit, stats = render_frame(n, _pose(), CAMERA, spp=2, noise=_noise(), keys=("rgb_map", "rgb_lin"), denoise=_params())
    assert bool(torch.isfinite(lit["rgb_map"]).all()) and bool(torch.isfinite(lit["rgb_lin"]).all()) and (lit["count"] == 2).all()


def test_evaluation_takes_the_frame_from_the_data_set(model, tmp_path):
    from PIL import Image
    from nmf_amd.dataLoader import BlenderDataset
    from nmf_amd.renderer import evaluation
    scene = tmp_path / "scene"
    _load_tool("make_blender_scene").main(["--out", str(scene), "--views", "1", "--test-views", "1", "--res", "32", "--grid", "32", "--bg", "32"])
    ds = BlenderDataset(str(scene), split="test", is_stack=True, N_vis=-1)
    res = {}
    for name, kw in (("raw", {}), ("den", dict(denoise=_params()))):
        res[name] = evaluation(ds, model[0], None, None, str(tmp_path / name), N_vis=-1, noise=_noise(), spp=4, **kw)
        assert len(res[name]["psnrs"]) == 1 and np.isfinite(res[name]["psnrs"][0])
    raw, den = _files(tmp_path / "raw"), _files(tmp_path / "den")
    assert set(raw) == set(den)
    for sub in ("spp", "noise", "world_normal", "acc_map"):
        assert raw[f"{sub}/000.png"] == den[f"{sub}/000.png"], sub
    assert raw["000.png"] != den["000.png"] and np.asarray(Image.open(tmp_path / "den" / "000.png")).shape[:2] == (32, 32)
    with pytest.raises(ValueError):
        evaluation(ds, model[0], None, None, str(tmp_path / "x"), N_vis=-1, spp=1, denoise=_params())


def test_command_line_with_denoise(model, tmp_path, capsys):
    from nmf_amd import render as R
    nerf, cfg = model
    ck = str(tmp_path / "m.th")
    nerf.save(ck, cfg["arch"])
    rec = R.main(["--ckpt", ck, "--views", "1", "--res", str(RES), "--path", "orbit", "--frames", "2", "--spp", "4", "--adaptive", "1",
                  "--denoise", "--denoise-strength", "2", "--light-turntable", "1", "--out", str(tmp_path / "a")])
    line = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    assert line == json.loads(json.dumps(rec))
    assert rec["sampling"] == dict(spp=4, min_spp=4, adaptive=1.0, denoise=dict(DEFAULTS, k_c=2.0))
    files = _files(tmp_path / "a")
    assert {"000.png", "light_000.png", "path/000.png", "path/001.png", "path/noise/000.png", "path/spp/001.png"} <= set(files)
    rec = R.main(["--ckpt", ck, "--views", "1", "--res", str(RES), "--spp", "2", "--denoise", "3", "--out", str(tmp_path / "b")])
    capsys.readouterr()
    assert rec["sampling"]["denoise"] == dict(DEFAULTS, levels=3) and os.path.exists(tmp_path / "b" / "000.png")
