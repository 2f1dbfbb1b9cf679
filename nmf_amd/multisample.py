"""Multi-sample frames: several evaluation passes of one view accumulated per pixel on the device, with an
adaptive sample count.  A frame of render_images is ONE stochastic sample per pixel even with is_train=False (DeviceNoise rotates the
Sobol points of the secondary rays, the bounce selection and the re-trace top-k draw fresh uniforms); render_frame averages passes in
LINEAR radiance, tonemaps the mean, jitters the sub-pixel position when the rays come from a pose, and renders later passes only for
the pixels whose standard error in display units is still above `tol`.  The reference renders one sample per pixel.

The kernels are csrc/accum.hip (include/nmf_hip.h, "Multi-sample frames"): nmf_camera_rays_at, nmf_accum_update, nmf_accum_active,
nmf_accum_resolve.  With spp = 1 nothing here runs: renderer.evaluation_path / evaluate keep their single-pass code.

Denoised frames (csrc/denoise.hip, include/nmf_hip.h "Denoised frames"): render_frame(denoise=DenoiseParams()) runs a
variance-guided, edge-stopping a-trous filter over the finished state -- the grain sits in the specular term, and a pixel whose samples
all agreed (se = 0: the background, unscattered pixels) leaves with its bits.  Off by default: without `denoise` nothing new runs."""
import dataclasses
import math

import numpy as np
import torch

# the additive recurrence of the plastic number: the sub-pixel offsets of the passes (R2 sequence, low discrepancy for every prefix)
PLASTIC = (0.7548776662, 0.5698402910)
FRAME_KEYS = ("rgb_map", "acc_map", "depth", "world_normal", "rgb_lin")
# `--adaptive` without a value, in 8-bit levels (tol = ADAPTIVE_DEFAULT / 255): chosen from the table of DESIGN.md 10.11
ADAPTIVE_DEFAULT = 1.0


@dataclasses.dataclass(frozen=True)
class DenoiseParams:
    """The six numbers of the filter (include/nmf_hip.h, "Denoised frames"): levels of steps 1, 2, 4, ... (0 to 8; 0 is the undenoised
    frame), and the widths of the four edge tests -- k_c in standard errors of the displayed colour (the strength), k_n on the
    difference of the mean normals, k_z in depth gradients per pixel with eps_z the slack of a flat surface, k_a on the coverage.
    The defaults are the setting of DESIGN.md 10.12's table with the lowest error at 4 spp."""
    levels: int = 3
    k_c: float = 4.0
    k_n: float = 0.5
    k_z: float = 2.0
    eps_z: float = 0.02
    k_a: float = 0.25

    def __post_init__(self):
        if isinstance(self.levels, bool) or int(self.levels) != self.levels or not 0 <= self.levels <= 8:
            raise ValueError(f"DenoiseParams: levels is an integer in [0, 8], got {self.levels}")
        for name in ("k_c", "k_n", "k_z", "eps_z", "k_a"):
            v = float(getattr(self, name))
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"DenoiseParams: {name} is finite and positive, got {v}")

    def record(self):
        """the parameters as a JSON-able dict (the `sampling` record of nmf_amd.render)"""
        return {k: (int(v) if k == "levels" else float(v)) for k, v in dataclasses.asdict(self).items()}


DENOISE_KEYS = ("rgb_map", "rgb_lin", "acc_map", "se")


def pass_offset(k):
    """the sub-pixel point of pass k in [0, 1)^2 as two fp32 values: the pixel centre for pass 0, frac(0.5 + k PLASTIC) in float64
    rounded to fp32 afterwards (a value that rounds up to 1 wraps to 0)"""
    if k < 0:
        raise ValueError("pass_offset: k is at least 0")
    out = []
    for a in PLASTIC:
        v = np.float32(np.mod(0.5 + np.float64(k) * np.float64(a), 1.0))
        out.append(float(v) if v < 1.0 else 0.0)
    return tuple(out)


class FrameAccumulator:
    """The per-pixel state of one H x W frame on `device` (hip.accum_state_bytes, zeroed): sample count, running means of rgb_lin,
    acc, depth, normal and the displayed rgb_map, and rgb_map's sum of squared deviations per channel.
      update(ims, pix=None)        folds one pass (render_images' dict with rgb_lin, acc_map, rgb_map and optionally depth,
                                   world_normal, rows indexed by the entries of pix; None: all pixels)
      active(min_spp, max_spp, tol) -> (pix int32 [n] ascending, n): the pixels that still need samples; ONE read-back of n
      resolve(...)                 -> dict(rgb_map, acc_map, depth, world_normal, se, count) of the keys asked for
      denoise(params, ...)         -> dict(rgb_map, rgb_lin, acc_map, se) of the keys asked for: the filtered frame (DenoiseParams)
      reset()                      zeroes the state for the next frame"""

    def __init__(self, H, W, device="cuda"):
        from . import hip
        self.H, self.W = int(H), int(W)
        device = torch.device(device)
        if device.type != "cuda":
            raise hip.NmfHipError("FrameAccumulator: nmf_amd operators need device tensors (no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.state = torch.zeros(hip.accum_state_bytes(self.H, self.W) // 4, dtype=torch.int32, device=device)
        self._list = torch.empty(self.H * self.W, dtype=torch.int32, device=device)
        self._n = torch.zeros(1, dtype=torch.int32, device=device)

    def reset(self):
        self.state.zero_()

    def update(self, ims, pix=None):
        from . import hip
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()      # noqa: E731
        hip.accum_update(self.state, self.H, self.W, f(ims["rgb_lin"]), f(ims["acc_map"]), f(ims["rgb_map"]), depth=f(ims.get("depth")),
                         normal=f(ims.get("world_normal")), pix=pix)

    def active(self, min_spp, max_spp, tol):
        from . import hip
        hip.accum_active(self.state, self.H, self.W, min_spp, max_spp, tol, out=self._list, n_out=self._n)
        n = int(hip.Readback.of(self.device).start(self._n).get()[0])
        return self._list[:n], n

    def resolve(self, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False, keys=FRAME_KEYS):
        from . import hip
        names = dict(rgb_map="rgb_map", acc_map="acc", depth="depth", world_normal="normal", se="se", count="count")
        want = [k for k in names if k in keys or k in ("se", "count")]
        out = hip.accum_resolve(self.state, self.H, self.W, bg=bg, tonemap=tonemap, noclip=noclip, want=tuple(names[k] for k in want))
        res = {k: out[names[k]] for k in want}
        if "rgb_lin" in keys:      # the mean radiance itself: the same kernel without tonemap over a black background (v + t 0 = v)
            res["rgb_lin"] = hip.accum_resolve(self.state, self.H, self.W, bg=(0.0, 0.0, 0.0), tonemap=False, want=("rgb_map",))["rgb_map"]
        return res

    def denoise(self, params, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False, keys=("rgb_map",), frame_hw=None):
        """The a-trous filter over the state as it stands (the state is only read; the workspace is kept for the next frame) ->
        dict of the `keys` among rgb_map [P, 3], rgb_lin [P, 3], acc_map [P] (filtered) and se [P] = sqrt of the propagated variance
        guide (not an error estimate).  frame_hw: the (H, W) the P pixels form when the accumulator was made for a ray array (1 x P)."""
        from . import hip
        if not isinstance(params, DenoiseParams):
            raise TypeError("FrameAccumulator.denoise: params is a DenoiseParams")
        H, W = (self.H, self.W) if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1]))
        if H < 1 or W < 1 or H * W != self.H * self.W:
            raise ValueError(f"FrameAccumulator.denoise: frame_hw = {frame_hw} does not hold the accumulator's {self.H * self.W} pixels")
        names = dict(rgb_map="rgb_map", rgb_lin="rgb_lin", acc_map="acc", se="se")
        want = [k for k in DENOISE_KEYS if k in keys]
        if not want or set(keys) - set(DENOISE_KEYS):
            raise ValueError(f"FrameAccumulator.denoise: keys are a non-empty choice of {DENOISE_KEYS}")
        ws = getattr(self, "_denoise_ws", None)
        if ws is None:
            ws = self._denoise_ws = torch.empty(hip.denoise_workspace_bytes(H, W) // 4, dtype=torch.float32, device=self.device)
        out = hip.denoise(self.state, H, W, params.levels, params.k_c, params.k_n, params.k_z, params.eps_z, params.k_a, bg=bg,
                          tonemap=tonemap, noclip=noclip, want=tuple(names[k] for k in want), workspace=ws)
        return {k: out[names[k]] for k in want}


def _is_pose(x):
    return tuple(getattr(x, "shape", ())) in ((3, 4), (4, 4))


@torch.no_grad()
def render_frame(nerf, rays_or_pose, focal_or_camera, *, spp, min_spp=4, tol=None, jitter=True, noise=None, keys=("rgb_map",),
                 chunk=None, accumulator=None, render=None, denoise=None, frame_hw=None):
    """One view of `nerf` (a TensorNeRF, also inside relight.relit, or a ComposedScene: what render_images takes) from up to `spp`
    passes per pixel.

    rays_or_pose / focal_or_camera: a camera-to-world matrix ([3, 4] or [4, 4], host values) with camera = dict(w, h, fx, fy, cx, cy)
    -- the rays of every pass are made on the device (hip.camera_rays_at): pass 0 through the pixel centres (the bits of
    hip.camera_rays), pass k >= 1 through pass_offset(k) rotated per pixel by the hash of (pixel, k) when jitter is on -- or a ray
    array [P, 6] (a data set's view) with its focal length, which needs jitter=False: every pass renders rays[pix].

    The first min(min_spp, spp) passes render all pixels.  tol=None: so does every pass (fixed-count sampling).  Otherwise pass k
    renders the pixels whose standard error of the displayed colour, max_c sqrt(M2_c / (n (n - 1))), is above tol (display units:
    1 / 255 is one 8-bit level), and the loop ends when none is left or after spp passes.  Stopping on the running variance biases
    the mean slightly towards samples that happened to agree; that is accepted.

    -> (ims, stats): ims = the finished maps of `keys` (rgb_map [P, 3] = srgb(mean rgb_lin) + (1 - mean acc) white, acc_map [P],
    depth [P], world_normal [P, 3], rgb_lin [P, 3]: plain means) plus se [P] and count [P] (float); stats = dict(passes, rays_rendered).
    chunk: render_images' rays per chunk (default: the model's eval_batch_size).  accumulator / render: the FrameAccumulator to use
    (reset first; default: a new one) and the pass renderer (default: renderer.render_images) -- the seam the CPU tests drive the
    loop through.

    denoise: a DenoiseParams -- the finished state goes through FrameAccumulator.denoise, and rgb_map (and rgb_lin, when asked for)
    are the filtered ones; every other map, se and count among them, stays the measured one, and "rgb_raw" in keys adds the
    undenoised rgb_map.  It needs spp >= 2 (one sample has no variance).  The filter needs the frame's shape: a pose brings it, a ray
    array needs frame_hw = (H, W) with H W = P (its accumulator stays 1 x P for the passes).  None (the default): nothing new runs."""
    spp, min_spp = int(spp), int(min_spp)
    if spp < 1 or min_spp < 1:
        raise ValueError(f"render_frame: spp and min_spp are at least 1, got {spp} and {min_spp}")
    if tol is not None and not float(tol) >= 0.0:
        raise ValueError(f"render_frame: tol is None (fixed count) or at least 0, got {tol}")
    if set(keys) - set(FRAME_KEYS) - ({"rgb_raw"} if denoise is not None else set()):
        raise ValueError(f"render_frame: keys are a choice of {FRAME_KEYS}; the material maps are not accumulated")
    if denoise is not None:
        if not isinstance(denoise, DenoiseParams):
            raise TypeError("render_frame: denoise is a DenoiseParams or None")
        if spp < 2:
            raise ValueError(f"render_frame: denoise needs spp >= 2 (the variance of one sample is unknown), got spp = {spp}")
    min_spp = min(min_spp, spp)
    if render is None:
        from .renderer import render_images as render
    pose = _is_pose(rays_or_pose)
    if pose:
        cam = focal_or_camera
        H, W, focal = int(cam["h"]), int(cam["w"]), float(cam["fx"])
        c2w = np.asarray(rays_or_pose.cpu() if isinstance(rays_or_pose, torch.Tensor) else rays_or_pose, dtype=np.float32)
        device = accumulator.device if accumulator is not None else torch.device("cuda", torch.cuda.current_device())
    else:
        if jitter:
            raise ValueError("render_frame: sub-pixel jitter needs a pose (rays are made per pass); pass jitter=False with a ray array")
        rays_all = rays_or_pose
        H, W, focal = 1, int(rays_all.shape[0]), float(focal_or_camera)
        device = rays_all.device
    if denoise is not None:
        if pose:
            if frame_hw is not None and (int(frame_hw[0]), int(frame_hw[1])) != (H, W):
                raise ValueError(f"render_frame: frame_hw = {tuple(frame_hw)} is not the camera's {H} x {W}")
            frame_hw = (H, W)
        elif frame_hw is None or len(frame_hw) != 2 or min(int(v) for v in frame_hw) < 1 or int(frame_hw[0]) * int(frame_hw[1]) != H * W:
            raise ValueError(f"render_frame: denoise with a ray array needs frame_hw = (H, W) with H W = {H * W} rays, got {frame_hw}")
    acc = accumulator if accumulator is not None else FrameAccumulator(H, W, device)
    if accumulator is not None:
        if acc.H * acc.W != H * W:
            raise ValueError(f"render_frame: the accumulator holds {acc.H} x {acc.W} pixels, the frame has {H * W}")
        acc.reset()
    # (the filter's edge guides are the depth and normal means: a denoised frame accumulates both whatever the caller asked for)
    need = ("rgb_map", "acc_map", "rgb_lin") + tuple(k for k in ("depth", "world_normal") if k in keys or denoise is not None)
    P = H * W
    passes = rays_rendered = 0
    for k in range(spp):
        pix, n = None, P
        if tol is not None and k >= min_spp:
            pix, n = acc.active(min_spp, spp, float(tol))
            if n == 0:
                break
        if pose:
            from . import hip
            off, seed = (pass_offset(k), k) if jitter else ((0.5, 0.5), 0)
            rays = hip.camera_rays_at(c2w, cam["fx"], cam["fy"], cam["cx"], cam["cy"], acc.H, acc.W, jitter=off, seed=seed, pix=pix,
                                      device=device)
        else:
            rays = rays_all if pix is None else rays_all[pix.long()]
        acc.update(render(nerf, rays, focal, chunk=chunk, noise=noise, keys=need), pix)
        passes += 1
        rays_rendered += n
    noclip = bool(getattr(nerf, "hdr", False))
    if denoise is None:
        ims = acc.resolve(bg=(1.0, 1.0, 1.0), tonemap=True, noclip=noclip, keys=tuple(keys))
        return ims, dict(passes=passes, rays_rendered=rays_rendered)
    # the measured maps first (rgb_lin comes from the filter; the undenoised rgb_map only where rgb_raw asks for it), then the filter
    ims = acc.resolve(bg=(1.0, 1.0, 1.0), tonemap=True, noclip=noclip,
                      keys=tuple(k for k in keys if k not in ("rgb_raw", "rgb_lin")) + (("rgb_map",) if "rgb_raw" in keys else ()))
    if "rgb_raw" in keys:
        ims["rgb_raw"] = ims["rgb_map"]
    if "rgb_map" not in keys:
        ims.pop("rgb_map", None)
    den = acc.denoise(denoise, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=noclip, keys=("rgb_map", "rgb_lin"), frame_hw=frame_hw)
    ims.update({k: den[k] for k in ("rgb_map", "rgb_lin") if k in keys})
    return ims, dict(passes=passes, rays_rendered=rays_rendered)
