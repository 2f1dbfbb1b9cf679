"""Relighting: the environment map of a trained scene rotated, or replaced by a panorama imported without an optimisation run.

The reference shows its relighting off by rotating the lights in notebooks (scripts/car_rotating_lights.ipynb, rotating_ball.ipynb,
relighting_calc.ipynb) and imports a panorama by fitting a map to it (scripts/pano2cube.py; nmf_amd/pano2env.fit).  Both are one
operation here: a spherical radiance function resampled into the texel grid of an IntegralEquirect under a rotation
(csrc/envmap_resample.hip); the summed-area table, the prefiltered lookup, the SH irradiance and the fused eval pass
behind it are the ones every map goes through.

    R = rotation(yaw=30)                                  # +z up, degrees
    with relit(nerf, rotate_env(nerf.bg_module, R)):      # the scene's own lighting turned by 30 degrees about the vertical
        rgb = render_images(nerf, rays, focal)
    bg = import_panorama(exr.imread("studio.exr")[..., :3], res=512)

"Lighting rotated by R" means L'(d) = L(R^T d): light that came from v now comes from R v.
"""
import contextlib
import math

import numpy as np
import torch

from . import hip
from .modules.integral_equirect import IntegralEquirect


def _rot(axis, t):
    c, s = math.cos(t), math.sin(t)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def rotation(yaw=0.0, pitch=0.0, roll=0.0, degrees=True):
    """3x3 rotation, +z up: roll about +x, then pitch about +y, then yaw about +z (R = Rz(yaw) Ry(pitch) Rx(roll))"""
    k = math.pi / 180.0 if degrees else 1.0
    return _rot(2, yaw * k) @ _rot(1, pitch * k) @ _rot(0, roll * k)


def axis_angle(axis, angle):
    """3x3 rotation by `angle` radians about `axis` (Rodrigues; the axis need not be normalised)"""
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    n = float(np.linalg.norm(a))
    if not n > 0:
        raise ValueError("axis_angle: the axis has no direction")
    x, y, z = a / n
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def lookup_bias(H, W):
    """what a sharpest lookup at a texel centre returns of the texel's value: (W-1)(H-1)/(WH).  The SAT's W-1 columns and H-1 rows
    cover the sphere while the lookup normalises its box by W x H texels (the reference's (sw/2 W)(sh/2 H)); a panorama has bias 1."""
    return (W - 1) * (H - 1) / float(W * H)


def _matrix(R):
    if R is None:
        return np.eye(3)
    if isinstance(R, torch.Tensor):
        R = R.detach().cpu().numpy()
    R = np.asarray(R, dtype=np.float64)
    if R.shape != (3, 3):
        raise ValueError(f"a rotation is a 3x3 matrix, got {R.shape}")
    return R


def _fixed_module(res, mipbias, device):
    """an IntegralEquirect as render.load_fixed_bg builds it (learning rates 0), brightness 0 and mul 1"""
    bg = IntegralEquirect(bg_resolution=res, mipbias=mipbias, activation="exp", lr=0.0, init_val=-1.897, mul_lr=0.0,
                          brightness_lr=0, betas=[0.0, 0.0], mul_betas=[0.9, 0.9], mipbias_lr=0.0, mipnoise=0.0)
    return bg.to(device)


def _destination(out, res, device, mipbias):
    if out is None:
        return _fixed_module(int(res), mipbias, device)
    H, W = out.hw()
    if res is not None and (H, W) != (int(res), 2 * int(res)):
        raise ValueError(f"out is a {H}x{W} map, res asks for {int(res)}x{2 * int(res)}")
    if out.bg_mat.device != torch.device(device) or out.bg_mat.dtype != torch.float32 or not out.bg_mat.is_contiguous():
        raise hip.NmfHipError("out must hold a contiguous float32 bg_mat on the source's device")
    return out


def _written(out):
    # the kernel wrote bg_mat behind autograd's back: bump its version (as optim.py does after its kernel), so that the module's
    # tables, the SH projection and the fused pass rebuild IN PLACE on their next use
    torch.autograd.graph.increment_version(out.bg_mat)
    return out


@torch.no_grad()
def rotate_env(bg, R, res=None, supersample=4, out=None):
    """-> an IntegralEquirect that holds bg's lighting rotated by R, at resolution `res` (default: bg's, or out's).  The source is
    bg's ACTIVATED map (brightness, mul and the clip(max=20) are baked in), so the result has brightness 0 and mul 1; mipbias is
    copied.  out: a module of an earlier call, rewritten in place (a light turntable allocates nothing per frame)."""
    if out is bg:
        raise ValueError("rotate_env: out must not be the source module")
    src = bg._tables_checked()[0]
    Hs, Ws = src.shape[-2:]
    if out is None:
        out = _destination(None, res if res is not None else Hs, src.device, float(bg.mipbias.detach()))
    else:
        out = _destination(out, res, src.device, None)      # (a module made by rotate_env / import_panorama: brightness 0, mul 1)
        out.mipbias.copy_(bg.mipbias.detach())
    H, W = out.hw()
    hip.env_resample(src, hip.ENV_SRC_MODULE, _matrix(R), lookup_bias(Hs, Ws) / lookup_bias(H, W), supersample, out.bg_mat.detach())
    return _written(out)


def default_supersample(pano_width, res):
    return int(min(max(math.ceil(pano_width / (2.0 * res)), 1), 8))


@torch.no_grad()
def import_panorama(pano, res, R=None, supersample=None, out=None, device="cuda"):
    """pano: float [Hp,Wp,3] numpy array or tensor in pano2env.pixel_directions' parameterisation -> an IntegralEquirect at
    res x 2 res whose sharpest lookups return the panorama's radiance, area-averaged per texel (gain 1 / lookup_bias(res, 2 res);
    mipbias 0 as pano2env.fit and render.load_fixed_bg have it).  No optimisation run."""
    if out is not None:
        device = out.bg_mat.device
    if isinstance(pano, torch.Tensor):
        p = pano.detach()
    else:
        p = torch.as_tensor(np.ascontiguousarray(np.asarray(pano)[..., :3], dtype=np.float32))
    if p.dim() != 3 or p.shape[-1] < 3:
        raise ValueError(f"a panorama is [H,W,3], got {tuple(p.shape)}")
    p = p[..., :3].to(device=device, dtype=torch.float32).contiguous()
    out = _destination(out, res, p.device, 0)
    H, W = out.hw()
    if supersample is None:
        supersample = default_supersample(p.shape[1], H)
    hip.env_resample(p, hip.ENV_SRC_PANORAMA, _matrix(R), 1.0 / lookup_bias(H, W), supersample, out.bg_mat.detach())
    return _written(out)


@contextlib.contextmanager
def relit(nerf, bg):
    """installs `bg` as nerf.bg_module and restores the original on exit.  The fused pass caches which parameters it compares versions
    of (TrainPass._param_token) and refreshes that list only when the FIELD's parameter list changes, so a module swapped in after
    a render would be rendered from the replaced module's tables: both swaps tell the pass."""
    def swap(m):
        nerf.bg_module = m
        fp = getattr(nerf, "_fused_pass", None)
        if fp is not None:
            fp.invalidate_tables()

    old = nerf.bg_module
    swap(bg)
    try:
        yield nerf
    finally:
        swap(old)
