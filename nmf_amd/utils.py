"""Evaluation metrics and regularisers of the reference's utils.py.  `rgb_ssim` (:90-136) keeps its signature and return value; the
computation is the HIP kernel nmf_ssim (nmf_amd/csrc/metrics.hip) on the current device, whatever device the images are on.
`TVLoss` (:139-151) keeps its call signature; device tensors go through nmf_tv_fwd_bwd (nmf_amd/csrc/tv.hip)."""
import numpy as np
import torch

from . import hip


def _device_image(x):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """utils.py:90-136: SSIM of two [H, W, 3] images (numpy arrays or tensors, CPU or device) -> a Python float, or with
    return_map the [H-10, W-10, 3] map as a numpy array.  The images are taken as fp32; moments and the per-pixel formula
    are fp64 (the reference's float64 scipy convolutions)."""
    assert len(img0.shape) == 3
    assert img0.shape[-1] == 3
    assert img0.shape == img1.shape
    if filter_size != 11:
        raise NotImplementedError(f"rgb_ssim: filter_size {filter_size} (only 11 is compiled into nmf_ssim)")
    a = _device_image(img0)
    b = _device_image(img1).to(a.device)
    out = hip.ssim(a, b, max_val=max_val, k1=k1, k2=k2, return_map=return_map, filter_sigma=filter_sigma)
    if return_map:
        return out[1][0].cpu().numpy()
    return float(out[0].item())


def tv_reference(x):
    """utils.py:143-151 as written: the total variation of a [B,C,H,W] tensor (a last dimension of 1: a line)"""
    if x.shape[-1] == 1:
        h_tv = x[:, :, 1:, :] - x[:, :, :-1, :]
        return h_tv.abs().mean()
    h_tv = x[:, :, 1:, :-1] - x[:, :, :-1, :-1]
    w_tv = x[:, :, :-1, 1:] - x[:, :, :-1, :-1]
    return (w_tv ** 2 + h_tv ** 2 + 1e-5).sqrt().mean()


class TVLoss(torch.nn.Module):
    """utils.py:139-151.  A float32 device tensor [1,C,H,W] is ONE kernel launch per direction (functional.TVWeighted); a CPU tensor
    evaluates the reference's torch expression.  Any other device tensor is refused: there is no eager device path."""

    def forward(self, x):
        if not x.is_cuda:
            return tv_reference(x)
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[0] != 1:
            raise NotImplementedError(f"TVLoss on the device takes a float32 [1,C,H,W] tensor, not {x.dtype} {tuple(x.shape)}")
        from .functional import TVWeighted
        return TVWeighted.apply((hip.tv_kind(x),), (1.0,), x)

    def _tensor_size(self, t):
        return t[0].numel()
