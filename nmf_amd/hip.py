"""Binding of libnmf_hip.so (include/nmf_hip.h).  This is the ONLY way the host-side operator
classes reach the GPU kernels; there is no CPU or PyTorch fallback: if a library is missing the
import of any product operator raises.

torch is used for what it is here for: device memory (tensors), the current HIP stream and
torch.distributed.  Every wrapper takes torch tensors and has ONE implementation.  The rule: a wrapper
uses ctypes only if csrc/host_ext.cpp has no function for that entry point.  Where it has one, the wrapper
is one call into lib/_nmf_host.so for every argument form (output allocation, dtype / contiguity / device
checks and the C-ABI call in C++, ~3 us per call instead of 10-25 us of Python, and the code the fused
step runs); an allocating form at most allocates its outputs and calls the `*_into` function.  The ctypes
wrappers (off the per-step path) check the tensors and pass raw pointers + sizes + the current stream.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NMF_HIP_LIB") or os.path.join(_HERE, "lib", "libnmf_hip.so")      # (NMF_HIP_LIB: kernel experiments, tools/)
HOST_EXT_PATH = os.path.join(_HERE, "lib", "_nmf_host.so")
_BUILD_HINT = "build it with `python -c 'import __graft_entry__ as g; g.build()'` (or nmf_amd/csrc/build.sh)"


class NmfHipError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise NmfHipError(f"{LIB_PATH} not found: {_BUILD_HINT}.  nmf_amd has no CPU fallback.")
    return C.CDLL(LIB_PATH)


def _load_host():
    """lib/_nmf_host.so: the C++ wrappers and the fused training / evaluation pass (StepCore).  Required: a missing, broken or
    stale build raises like a missing libnmf_hip.so does"""
    if not os.path.exists(HOST_EXT_PATH):
        raise NmfHipError(f"{HOST_EXT_PATH} not found: {_BUILD_HINT}.  nmf_amd has no CPU fallback.")
    spec = importlib.util.spec_from_file_location("_nmf_host", HOST_EXT_PATH)
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    except ImportError as e:
        raise NmfHipError(f"{HOST_EXT_PATH} does not load ({e}): {_BUILD_HINT}") from e
    if mod.abi_version() != _lib.nmf_version():
        raise NmfHipError(f"{HOST_EXT_PATH} was built against ABI version {mod.abi_version()}, {LIB_PATH} is version "
                          f"{_lib.nmf_version()}: {_BUILD_HINT}")
    mod.set_error_class(NmfHipError)
    return mod


_lib = _load()
HOST_EXT = _load_host()


class MarchParams(C.Structure):
    _fields_ = [("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("alpha_inv", C.c_float * 3),
                ("stepsize", C.c_float), ("half_step", C.c_float), ("near_t", C.c_float), ("far_t", C.c_float),
                ("focal", C.c_float), ("n_steps", C.c_int32), ("grid", C.c_int32 * 3), ("is_train", C.c_int32),
                ("seed", C.c_uint64), ("offset", C.c_uint64), ("occ_min", C.c_float * 3), ("occ_max", C.c_float * 3)]


class VmParams(C.Structure):
    _fields_ = [("aabb_min", C.c_float * 3), ("inv_size", C.c_float * 3), ("density_shift", C.c_float),
                ("grid", C.c_int32), ("stencil", C.c_float * 5), ("stencil_off", C.c_float * 5)]


class AdamSlot(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_int64), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("step_size", C.c_double), ("bc2_sqrt", C.c_double),
                ("is_f64", C.c_int32), ("reserved", C.c_int32)]


class CopySlot(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("numel", C.c_int64), ("src_is_f64", C.c_int32),
                ("dst_is_f64", C.c_int32)]


EXPORTS = [
    "nmf_version", "nmf_last_error_string", "nmf_event_create", "nmf_event_create_timed", "nmf_event_elapsed_ms", "nmf_event_destroy", "nmf_event_record", "nmf_event_synchronize",
    "nmf_stream_wait_event", "nmf_host_alloc_mapped", "nmf_host_free_mapped", "nmf_publish_i64x2", "nmf_wait_seq", "nmf_set_launch_probe", "nmf_alpha_pack", "nmf_march_count", "nmf_march_scan", "nmf_march_scan_workspace_bytes",
    "nmf_march_fill", "nmf_march_dense", "nmf_vm_pack_density", "nmf_vm_query_fwd", "nmf_vm_query_rows", "nmf_vm_query_sigma", "nmf_sat_lookup_bwd_dirs",
    "nmf_vm_unpack_density_grad", "nmf_vm_bwd_workspace_bytes", "nmf_composite_fwd", "nmf_composite_bwd", "nmf_segment_sum",
    "nmf_sat_build", "nmf_sat_build_bwd", "nmf_sat_lookup_fwd", "nmf_sat_lookup_bwd", "nmf_sat_lookup_bwd_binned",
    "nmf_sat_lookup_bwd_workspace_bytes",
    "nmf_select_bounces", "nmf_select_total", "nmf_view_adjoint_to_rays", "nmf_expand_segments", "nmf_segment_sum_wide",
    "nmf_brdf_mlp_fwd", "nmf_brdf_mlp_image_bytes", "nmf_brdf_mlp_pack",
    "nmf_brdf_mlp_bwd_segments", "nmf_brdf_mlp_bwd_segments_workspace_bytes", "nmf_heads_fwd", "nmf_heads_bwd", "nmf_ggx_rays_fwd", "nmf_ggx_rays_bwd", "nmf_ggx_rays_bwd_view", "nmf_ggx_prob", "nmf_shade_mix_fwd", "nmf_shade_mix_bwd", "nmf_shade_mix_bwd_view",
    "nmf_adam_step", "nmf_bounce_index", "nmf_bounce_index_workspace_bytes", "nmf_bounce_prep_fwd", "nmf_bounce_prep_bwd",
    "nmf_ray_compose_fwd", "nmf_ray_compose_bwd", "nmf_l1_mean_fwd", "nmf_l1_mean_bwd", "nmf_sqerr_fwd", "nmf_sqerr_bwd",
    "nmf_loss_mix_fwd", "nmf_loss_mix_bwd", "nmf_loss_head", "nmf_loss_head_workspace_bytes", "nmf_bg_adjoint", "nmf_vm_query_bwd_segments", "nmf_vm_bwd_clean_bytes", "nmf_sh_project",
    "nmf_retrace_scores", "nmf_argsort_f32", "nmf_argsort_workspace_bytes", "nmf_topk_select", "nmf_topk_select_workspace_bytes", "nmf_alpha_coarse", "nmf_alpha_coarse_words", "nmf_bounce_index_select", "nmf_bounce_prep_fwd_heads", "nmf_bounce_prep_heads_bwd", "nmf_multi_copy",
    "nmf_ssim", "nmf_ssim_workspace_bytes", "nmf_normal_err", "nmf_normal_err_workspace_bytes",
    "nmf_material_maps", "nmf_material_maps_edit", "nmf_heads_edit",
    "nmf_mc_count", "nmf_mc_emit", "nmf_mc_workspace_bytes", "nmf_mc_case_triangles",
    "nmf_tv_fwd_bwd", "nmf_tv_workspace_bytes",
    "nmf_env_resample",
    "nmf_relight_frame", "nmf_relight_ratio", "nmf_relight_ratio_workspace_bytes", "nmf_relight_adjust",
    "nmf_relight_adjust_workspace_bytes",
    "nmf_camera_rays", "nmf_frame_finish",
    "nmf_atlas_texels", "nmf_atlas_store",
    "nmf_rays_place", "nmf_merge_rank", "nmf_merge_scatter",
    "nmf_accum_state_bytes", "nmf_camera_rays_at", "nmf_accum_update", "nmf_accum_active", "nmf_accum_resolve",
    "nmf_denoise_workspace_bytes", "nmf_denoise_prepare", "nmf_denoise_level", "nmf_denoise_finish", "nmf_denoise",
]
for _n in EXPORTS:
    if not hasattr(_lib, _n):
        raise NmfHipError(f"libnmf_hip.so does not export {_n}")


def _declare_from_header():
    """argtypes / restype of every entry point, derived from include/nmf_hip.h (pointers and arrays -> void*, so wrappers
    pass Tensor.data_ptr() integers straight through; scalars are converted by ctypes)."""
    import re
    hdr = os.path.join(os.path.dirname(_HERE), "include", "nmf_hip.h")
    if not os.path.exists(hdr):
        # without prototypes ctypes would pass Tensor.data_ptr() integers as 32-bit C ints (truncated device pointers)
        raise NmfHipError(f"{hdr} is missing: the C-ABI prototypes of libnmf_hip.so are read from it (keep include/ next "
                          "to the nmf_amd package)")
    text = re.sub(r"/\*.*?\*/", " ", open(hdr).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    scal = {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "float": C.c_float, "double": C.c_double}
    for ret, name, args in re.findall(r"\b(int64_t|int|const char\s*\*)\s+(nmf_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        fn = getattr(_lib, name, None)
        if fn is None:
            continue
        fn.restype = C.c_int64 if ret == "int64_t" else (C.c_char_p if "char" in ret else C.c_int)
        types = []
        args = re.sub(r"\(\s*\*\s*(\w+)\s*\)\s*\([^)]*\)", r"*\1", args)      # a function-pointer parameter is a pointer
        for a in [x.strip() for x in args.split(",")]:
            if a in ("void", ""):
                continue
            if "*" in a or "[" in a:
                types.append(C.c_void_p)
            else:
                tok = [t for t in a.replace("const", " ").split() if t in scal]
                if not tok:
                    raise NmfHipError(f"cannot derive the ctypes type of '{a}' in {name}")
                types.append(scal[tok[0]])
        fn.argtypes = types


_declare_from_header()


def version():
    return _lib.nmf_version()


def _check(code, what):
    if code != 0:
        raise NmfHipError(f"{what} failed: {_lib.nmf_last_error_string().decode()} [{code}]")


def _stream():
    # raw handle of torch's current stream on the current device (what torch.cuda.current_stream().cuda_stream
    # returns, without building the Stream object: this runs ~100 times per training step)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _p(t, dtype=None):
    """device pointer (integer) of a contiguous tensor; None -> NULL"""
    if t is None:
        return None
    if dtype is not None and t.dtype != dtype:
        raise NmfHipError(f"expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise NmfHipError("nmf_amd operators need device tensors (no CPU path)")
    if not t.is_contiguous():
        raise NmfHipError("tensor must be contiguous")
    return t.data_ptr() or None


def channels_last_ptr_ok(t):
    """True if a [1,C,H,W] tensor is stored [H][W][C] densely (what the kernels index)."""
    _, Cn, H, W = t.shape
    return t.stride(1) == 1 and t.stride(3) == Cn and t.stride(2) == W * Cn


_host_mirror = {}


def host(t):
    """numpy copy of a small tensor, cached per (storage, version): geometry constants (aabb, grid size, step size)
    live in module buffers on the device; reading them back costs a stream sync each, so it is done once per value."""
    if not isinstance(t, torch.Tensor):
        return np.asarray(t)
    if not t.is_cuda:
        return t.detach().numpy()
    key = (t.data_ptr(), t._version, tuple(t.shape), t.dtype)
    v = _host_mirror.get(id(t))
    if v is None or v[0] != key:
        if len(_host_mirror) > 256:
            _host_mirror.clear()
        v = (key, t.detach().cpu().numpy(), t)          # keeps t alive so id(t) stays unique
        _host_mirror[id(t)] = v
    return v[1]


class Readback:
    """A few int64 sizes from the device to the host, split into start() and get() so that work queued in between runs
    while the numbers travel.  Pinned staging buffers from a small ring per device (at most two are ever in flight)."""
    _ring = {}

    def __init__(self):
        self.pin = torch.empty(4, dtype=torch.int64).pin_memory()
        self.ev = torch.cuda.Event()
        self.n = 0

    @classmethod
    def of(cls, dev):
        r = cls._ring.setdefault(str(dev), [[cls() for _ in range(4)], 0])
        r[1] = (r[1] + 1) & 3
        return r[0][r[1]]

    def start(self, t):
        self.n = t.numel()
        self.pin[: self.n].copy_(t, non_blocking=True)
        self.ev.record()
        return self

    def get(self):
        self.ev.synchronize()
        return self.pin[: self.n].tolist()


# ---- sampler ----------------------------------------------------------------------------------
def march_params(aabb, alpha_inv, stepsize, near, far, focal, n_steps, grid, is_train, seed=0, offset=0, occ_box=None):
    """occ_box: optional ((x0,y0,z0), (x1,y1,z1)) world box outside of which the alpha mask cannot keep a step"""
    p = MarchParams()
    if occ_box is not None:
        p.occ_min[:] = [float(v) for v in occ_box[0]]
        p.occ_max[:] = [float(v) for v in occ_box[1]]
    else:
        p.occ_min[:] = [1.0, 1.0, 1.0]
        p.occ_max[:] = [-1.0, -1.0, -1.0]
    a = host(aabb).astype(np.float32)
    p.aabb_min[:] = a[0].tolist()
    p.aabb_max[:] = a[1].tolist()
    p.alpha_inv[:] = np.asarray(alpha_inv, dtype=np.float32).tolist() if alpha_inv is not None else [0, 0, 0]
    st = np.float32(stepsize)
    p.stepsize = float(st)
    p.half_step = float(np.float32(st / np.float32(2)))
    p.near_t = float(np.float32(near))
    p.far_t = float(np.float32(far))
    p.focal = float(np.float32(focal))
    p.n_steps = int(n_steps)
    p.grid[:] = [int(g) for g in grid] if grid is not None else [0, 0, 0]
    p.is_train = 1 if is_train else 0
    p.seed = int(seed)
    p.offset = int(offset)
    return p


def alpha_pack(volume):
    n = volume.numel()
    bits = torch.zeros((n + 31) // 32, dtype=torch.int32, device=volume.device)
    _check(_lib.nmf_alpha_pack(_p(volume.contiguous(), torch.float32), C.c_int64(n), _p(bits), _stream()), "nmf_alpha_pack")
    return bits


def alpha_coarse(bits, grid):
    """coarse occupancy mask (one bit per 8^3 voxels) for nmf_march_count; grid = (gx, gy, gz) of the alpha volume"""
    g = (C.c_int32 * 3)(*[int(v) for v in grid])
    words = _lib.nmf_alpha_coarse_words(g)
    coarse = torch.zeros(max(words, 1), dtype=torch.int32, device=bits.device)
    _check(_lib.nmf_alpha_coarse(_p(bits, torch.int32), g, _p(coarse), _stream()), "nmf_alpha_coarse")
    return coarse


def march_count(p, rays, jitter, alpha_bits, alpha_coarse=None):
    """-> (valid [B, ceil(n_steps / 64)] int64 bit words, counts [B] int32)"""
    return HOST_EXT.march_count(C.addressof(p), rays, jitter, alpha_bits, alpha_coarse, _stream())


def march_scan(counts, max_samples):
    """-> (offsets [B+1] int64, whole_valid [B] uint8, totals [2] int64 = (samples, rays) kept under max_samples)"""
    return HOST_EXT.march_scan(counts, int(max_samples), _stream())


def march_fill(p, rays, b, M, jitter, valid, offsets, want_z=True):
    """-> (xyzt [M,4], ray_id [M] int32, step_id [M] int32, z [M] or None, dist [M])"""
    return HOST_EXT.march_fill(C.addressof(p), rays, b, M, jitter, valid, offsets, want_z, _stream())


def march_dense(p, rays, b, jitter, valid):
    ray_valid = torch.empty((b, p.n_steps), dtype=torch.uint8, device=rays.device)
    z_vals = torch.empty((b, p.n_steps), dtype=torch.float32, device=rays.device)
    _check(_lib.nmf_march_dense(C.byref(p), _p(rays, torch.float32), C.c_int64(b), _p(jitter), _p(valid),
                                _p(ray_valid), _p(z_vals), _stream()), "nmf_march_dense")
    return ray_valid.bool(), z_vals


# ---- VM field ----------------------------------------------------------------------------------
def derivative_stencil_rows():
    """Rows of the 5x5 x-derivative stencil of GridSampler2D.backward (smoothing=1): a normalised 3x3
    Gaussian (std 1) correlated with [-0.5, 0, 0.5]; computed in fp32 exactly like the reference does
    (modules/grid_sample_Cinf.py:16-29,49-63,218-233): kx[i][j] = 0.5*(S[i-1][j-2] - S[i-1][j])."""
    n = np.arange(3, dtype=np.float32) - np.float32(1.0)
    g1 = np.exp(-(n ** 2) / np.float32(2.0)).astype(np.float32)
    S = np.outer(g1, g1).astype(np.float32)
    S = (S / S.sum(dtype=np.float32)).astype(np.float32)
    rows = []
    for i in (1, 2):          # S row 0 (== row 2) and S row 1
        r = S[i - 1]
        rows.append([-0.5 * r[0], -0.5 * r[1], 0.0, 0.5 * r[1], 0.5 * r[2]])
    return np.asarray(rows[1], np.float32), np.asarray(rows[0], np.float32)   # centre row, off-centre rows


def vm_params(aabb, inv_size, density_shift, grid):
    p = VmParams()
    p.aabb_min[:] = host(aabb).astype(np.float32)[0].tolist()
    p.inv_size[:] = host(inv_size).astype(np.float32).tolist()
    p.density_shift = float(density_shift)
    p.grid = int(grid)
    c, o = derivative_stencil_rows()
    p.stencil[:] = c.tolist()
    p.stencil_off[:] = o.tolist()
    return p


def vm_pack_density(p, planes, lines, out=None):
    """planes[i]: [G,G,16] channel-last storage, lines[i]: [G,16].  out = (dpk, dlk) of an earlier call re-packs in place."""
    if out is None:
        G, dev = p.grid, planes[0].device
        out = ([torch.empty((G, G, 48), dtype=torch.float32, device=dev) for _ in range(3)],
               [torch.empty((G, 32), dtype=torch.float32, device=dev) for _ in range(3)])
    HOST_EXT.vm_pack_density_into(C.addressof(p), list(planes), list(lines), list(out[0]), list(out[1]), _stream())
    return out


def vm_query_fwd(p, xyzt, dpk, dlk, app_planes, app_lines, basis, want_density=True, want_normal=True,
                 want_app=True, want_coef=False):
    """-> (sigma_feat [M], sigma [M], grad [M,3], normal [M,3], app [M,24], coef [M,72]); None for what is not asked for.  The tables
    are fp32 or bfloat16 (the dtype of the first table the query needs decides)"""
    return HOST_EXT.vm_query_fwd(C.addressof(p), xyzt, dpk, dlk, app_planes, app_lines, basis, want_density, want_normal,
                                 want_app, want_coef, _stream())


def vm_query_rows(p, xyzt, dpk, dlk):
    """value + gradient + normal of a few rows (16 lanes per row): -> (sigma_feat [M], grad [M,3], normal [M,3])"""
    return HOST_EXT.vm_query_rows(C.addressof(p), xyzt, list(dpk), list(dlk), _stream())


def vm_query_sigma(p, xyzt, planes, lines):
    """density value of all samples from the density factors themselves (planes [G,G,16], lines [G,16], fp32 or bfloat16):
    -> (sigma_feat [M], sigma [M]), the bits of vm_query_fwd"""
    return HOST_EXT.vm_query_sigma(C.addressof(p), xyzt, list(planes), list(lines), _stream())


def to_bf16_tables(srcs, dsts=None):
    """fp32 tables -> bfloat16 copies in ONE launch (nmf_multi_copy, round to nearest even); dsts = the list of an earlier
    call refreshes the copies in place."""
    if dsts is None:
        dsts = [torch.empty(t.shape, dtype=torch.bfloat16, device=t.device) for t in srcs]
    n = len(srcs)
    slots = (CopySlot * n)()
    for i, (a, b) in enumerate(zip(srcs, dsts)):
        if a.dtype != torch.float32 or b.dtype != torch.bfloat16 or a.numel() != b.numel():
            raise NmfHipError("to_bf16_tables: fp32 sources and bf16 destinations of equal size")
        _p(a), _p(b)                                  # device / contiguity checks
        slots[i] = CopySlot(a.data_ptr(), b.data_ptr(), a.numel(), 0, 2)
    multi_copy(slots, n)
    return dsts


VM_MAX_SEGMENTS = 4


def vm_bwd_clean_scratch(p, device):
    """the zeroed scratch a caller keeps between walks (vm_query_bwd_segments(..., clean=...)): counters that every walk hands back zero"""
    return torch.zeros(int(_lib.nmf_vm_bwd_clean_bytes(C.c_int32(p.grid))), dtype=torch.uint8, device=device)


def vm_query_bwd_segments(p, segs, dpk, dlk, app_planes, app_lines, basis, g_dpk, g_dlk, g_app_planes, g_app_lines,
                          g_basis=None, clean=None):
    """One backward walk over several sample sets (no concatenation).  segs: list of tuples
    (xyzt, sigma_feat, grad, d_sigma, d_sigma_feat, d_normal, d_app) -- the argument order of vm_query_bwd.
    clean: vm_bwd_clean_scratch (no memset launches)."""
    return HOST_EXT.vm_query_bwd_segments(C.addressof(p), list(segs), dpk, dlk, app_planes, app_lines, basis, g_dpk, g_dlk,
                                          g_app_planes, g_app_lines, g_basis, clean, _stream())


def vm_query_bwd(p, xyzt, dpk, dlk, app_planes, app_lines, basis, sigma_feat, grad, d_sigma, d_sigma_feat,
                 d_normal, d_app, g_dpk, g_dlk, g_app_planes, g_app_lines, g_basis=None):
    """the walk over ONE sample set: vm_query_bwd_segments with a single segment"""
    return vm_query_bwd_segments(p, [(xyzt, sigma_feat, grad, d_sigma, d_sigma_feat, d_normal, d_app)], dpk, dlk, app_planes,
                                 app_lines, basis, g_dpk, g_dlk, g_app_planes, g_app_lines, g_basis)


def vm_unpack_density_grad(p, g_dpk, g_dlk, out=None, l1=None):
    """out = (gp, gl) of an earlier call: the same tensors are overwritten (a training pass keeps its gradient tensors).
    l1 = (the six density parameters [planes + lines] in the gradients' storage order, 0-d device scale): the gradient of
    scale * sum_i mean |x_i| is added in the same launch (same bits as l1_mean_bwd(..., out=gp + gl) behind the unpack)"""
    return HOST_EXT.vm_unpack_density_grad(C.addressof(p), g_dpk, g_dlk, out, l1, _stream())


# ---- compositing --------------------------------------------------------------------------------
def composite_fwd(sigma, dist, offsets, b, distance_scale):
    """-> (weight [M], acc [b]); M == 0: nothing is launched, acc is zero"""
    return HOST_EXT.composite_fwd(sigma, dist, offsets, b, distance_scale, _stream())


def composite_bwd(sigma, dist, weight, offsets, b, distance_scale, d_weight):
    """-> d_sigma [M]"""
    return HOST_EXT.composite_bwd(sigma, dist, weight, offsets, b, distance_scale, d_weight, _stream())


def segment_sum(vals, scale, offsets, n_seg, lanes=1):
    """lanes=1: index-order sums (bit-reproducible); lanes=8: eight lanes per segment (tree sum)"""
    return HOST_EXT.segment_sum(vals, scale, offsets, n_seg, lanes, _stream())


# ---- environment map ---------------------------------------------------------------------------
def sat_build(bg_mat, brightness=0.0, mul=1.0, sc=None, out=None, pole=False, interleaved=False):
    """bg_mat [1,3,H,W] or [3,H,W] -> (activated, sat) [3,H,W] (+ pole-row means [2,3] with pole=True, + the channel-
    interleaved copy of sat [H,W,4] with interleaved=True: what the lookups read fastest).  sc: optional device float32 [3] =
    (mipbias, brightness, mul) read by the kernels instead of the by-value scalars (no host read-back of the parameters).
    out = the tuple of an earlier call (same flags) rebuilds the tables in place."""
    bg = bg_mat.reshape(3, bg_mat.shape[-2], bg_mat.shape[-1]).contiguous()
    if out is None:
        H, W = bg.shape[-2:]
        out = ((torch.empty_like(bg), torch.empty_like(bg))
               + ((torch.empty((2, 3), dtype=torch.float32, device=bg.device),) if pole else ())
               + ((torch.zeros((H, W, 4), dtype=torch.float32, device=bg.device),) if interleaved else ()))     # channel 3 is never written
    HOST_EXT.sat_build_into(bg, float(brightness), float(mul), sc, out[0], out[1], out[2] if pole else None,
                            out[-1] if interleaved else None, _stream())
    return (out[0], out[1]) + ((out[2],) if pole else ()) + ((out[-1],) if interleaved else ())


def _sat_layout(sat):
    """-> (H, W, layout) of a summed-area table: planar [3,H,W] (0) or channel-interleaved [H,W,4] (1)"""
    if sat.dim() == 3 and sat.shape[-1] == 4 and sat.shape[0] != 3:
        return sat.shape[0], sat.shape[1], 1
    return sat.shape[-2], sat.shape[-1], 0


def sh_project(vals, wq, sh_A, out=None):
    """-> (coeffs [K,3], conv [K,3]); wq [n,K] contiguous, sh_A [>=K]"""
    if out is None:
        K = wq.shape[1]
        out = (torch.empty((K, 3), dtype=torch.float32, device=vals.device),
               torch.empty((K, 3), dtype=torch.float32, device=vals.device))
    HOST_EXT.sh_project_into(vals, wq, sh_A, out[0], out[1], _stream())
    return out


def sat_build_bwd(d_sat, bg_mat, act, d_pole, brightness=0.0, mul=1.0, sc=None, out=None):
    """-> d_bg [3,H,W] (out: written in place)"""
    bg = bg_mat.reshape(3, bg_mat.shape[-2], bg_mat.shape[-1]).contiguous()
    if out is None:
        out = torch.empty_like(bg)
    HOST_EXT.sat_build_bwd_into(d_sat, bg, act, d_pole, float(brightness), float(mul), sc, out, _stream())
    return out


def sat_lookup_fwd(sat, dirs, sa, mipbias, pole_rows, sc=None):
    """dirs: [R,3] directions, or [R,6] ray rows (origin | direction) looked up along their columns 3..5; sat: the planar
    table [3,H,W] or sat_build's interleaved copy [H,W,4] (same results)"""
    return HOST_EXT.sat_lookup_fwd(sat, dirs, sa, mipbias, pole_rows, sc, _stream())


# lookups per call from which the table adjoint is binned (three more launches than the direct scatter; measured with
# tools/env_bwd_bench.py: 47 k lookups 53-73 us against 51 direct, 247 k lookups 138 against 176; in the training step the call
# sits on a side stream and the step time is the same either way, tools/ab_inprocess.py hip:ENV_BINNED_MIN_LOOKUPS).
# (a module constant: tests and tools/env_bwd_bench.py set it to compare the two forms)
# (from 30 k lookups: alone the two forms take the same time at 47 k -- 51 / 52 us -- but in the backward of a training step the leaf
# level's adjoint runs next to the binned adjoint of the level above, the value walk and the MLP backward, and the direct form's
# float atomics queue behind theirs at the memory side: 1.375 -> 1.361 ms per step)
ENV_BINNED_MIN_LOOKUPS = 30000


def sat_lookup_bwd(sat, dirs, sa, mipbias, d_out, d_sat, d_pole, d_mip=None, want_dirs=True, sc=None):
    """d_sat [H,W,4] / d_pole [2,3] / d_mip [1] are ACCUMULATED into (any may be None except d_pole).  Returns d_dirs shaped like
    dirs (None without want_dirs)."""
    return HOST_EXT.sat_lookup_bwd(sat, dirs, sa, mipbias, d_out, d_sat, d_pole, d_mip, want_dirs, sc,
                                   int(ENV_BINNED_MIN_LOOKUPS), _stream())


ENV_SRC_MODULE, ENV_SRC_PANORAMA = 0, 1


def env_resample(src, kind, R, gain, supersample, out):
    """Resample a spherical radiance function into a bg_mat under the rotation R (nmf_env_resample; nmf_amd/relight.py).
    src: float32 LINEAR radiance, [3,Hs,Ws] planar (kind ENV_SRC_MODULE: the activated table of a module) or [Hp,Wp,3] interleaved
    (kind ENV_SRC_PANORAMA); R: 3x3 rotation (host numbers); out: float32 [3,H,W] or [1,3,H,W], written in place with
    log(max(gain * mean, 1e-8)).  Returns out."""
    for name, t in (("src", src), ("out", out)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise NmfHipError(f"env_resample: {name} must be a device tensor (no CPU path)")
        if t.dtype != torch.float32:
            raise NmfHipError(f"env_resample: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise NmfHipError(f"env_resample: {name} must be contiguous")
    if src.device != out.device:
        raise NmfHipError("env_resample: src and out are on different devices")
    if kind == ENV_SRC_MODULE:
        if src.dim() != 3 or src.shape[0] != 3:
            raise NmfHipError(f"env_resample: a module source is [3,Hs,Ws], got {tuple(src.shape)}")
        Hs, Ws = src.shape[1], src.shape[2]
    elif kind == ENV_SRC_PANORAMA:
        if src.dim() != 3 or src.shape[2] != 3:
            raise NmfHipError(f"env_resample: a panorama source is [Hp,Wp,3], got {tuple(src.shape)}")
        Hs, Ws = src.shape[0], src.shape[1]
    else:
        raise NmfHipError(f"env_resample: unknown source kind {kind}")
    if out.dim() not in (3, 4) or out.shape[-3] != 3 or out.numel() != 3 * out.shape[-2] * out.shape[-1]:
        raise NmfHipError(f"env_resample: out is [3,H,W] or [1,3,H,W], got {tuple(out.shape)}")
    if src.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
        raise NmfHipError("env_resample: src and out share their storage")
    r = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(-1)]
    if len(r) != 9:
        raise NmfHipError("env_resample: R must be 3x3")
    _check(_lib.nmf_env_resample(_p(src), int(kind), Hs, Ws, *r, float(gain), int(supersample), _p(out), out.shape[-2], out.shape[-1],
                                 _stream()), "nmf_env_resample")
    return out


# ---- shading helpers -------------------------------------------------------------------------------
def select_bounces(weights, u, mode, mul, add=0.0, sum_w=1.0):
    """sum_w: python float, or a 0-d fp32 DEVICE tensor (read by the kernel: no host sync)."""
    dev_sum = sum_w if isinstance(sum_w, torch.Tensor) else None
    return HOST_EXT.select_bounces(weights, u, mode, mul, add, 1.0 if dev_sum is not None else sum_w, dev_sum, _stream())


_select_ws = {}


def select_total_workspace(dev, stream=None):
    """the partial-sum / ticket workspace of nmf_select_total: one per (device, stream) -- launches on different streams (the
    chunk contexts of an optimizer step, nmf_amd/fast_step.py) must not share it"""
    key = (dev, (stream if stream is not None else torch.cuda.current_stream(dev)).cuda_stream)
    ws = _select_ws.get(key)
    if ws is None:
        ws = _select_ws[key] = torch.zeros(258, dtype=torch.float64, device=dev)       # zeroed once; the kernel resets it
    return ws


def select_total(weights, u, extra):
    """-> 0-d fp32 device tensor clip(float(sum(w) + 1e-3 * (sum(u) + extra)), 1e-3) (one launch, float64 sums)"""
    return HOST_EXT.select_total(weights, u, float(extra), select_total_workspace(weights.device), _stream())


def view_adjoint_to_rays(ray_id, bidx, dv_a, dv_b, d_rays):
    """d_rays [B,6] (columns 3..5) -= per-row view adjoints dv_a [Mb,>=3] (+ dv_b), rows may be column slices"""
    return HOST_EXT.view_adjoint_to_rays(ray_id, bidx, dv_a, dv_b, d_rays, _stream())


def expand_segments(offsets, n_seg, total):
    """-> (seg [total] int32 = the segment of each element, loc [total] int32 = its index inside the segment)"""
    return HOST_EXT.expand_segments(offsets, n_seg, total, _stream())


def segment_sum_wide(vals, D, offsets, n_seg):
    """-> [n_seg, D]: per-segment sums of the first D columns of vals"""
    return HOST_EXT.segment_sum_wide(vals, D, offsets, n_seg, _stream())


def brdf_mlp_pack(weights, into=None):
    """The six weight tensors as the packed image the fused MLP kernels copy into LDS (nmf_brdf_mlp_pack): built once per weight
    update, passed as `image=` to brdf_mlp_fwd / brdf_mlp_bwd.  into: a uint8 device tensor of nmf_brdf_mlp_image_bytes() to reuse."""
    return HOST_EXT.brdf_mlp_pack(list(weights), into, _stream())


def brdf_mlp_fwd(weights, half_vec, diff_vec, feat_src, rough_src, src_idx, out_bias, max_workgroups=0, with_mask=False, image=None):
    """weights = (W0 [64,66], b0, W2 [64,64], b2, W4 [4,64], b4); max_workgroups: see brdf_mlp_bwd.  with_mask: also return
    the ReLU masks [R, 4] (int32 storage) that brdf_mlp_bwd takes together with the output.  image: brdf_mlp_pack(weights) --
    the same bits, a shorter launch (`weights` is then not read)."""
    r = HOST_EXT.brdf_mlp_fwd(list(weights or ()), half_vec, diff_vec, feat_src, rough_src, src_idx, out_bias, bool(with_mask),
                              int(max_workgroups), _stream(), image)
    return r if with_mask else r[0]


def brdf_mlp_bwd(weights, half_vec, diff_vec, feat_src, rough_src, src_idx, fwd_out, act_mask, d_out, grads, max_workgroups=0,
                 image=None):
    """fwd_out, act_mask: what brdf_mlp_fwd(..., with_mask=True) returned for the same inputs.  grads: six fp32 tensors
    shaped like `weights`, ACCUMULATED into (caller zeroes them once per pass).  max_workgroups > 0 caps the persistent
    workgroups (a launch that shares the chip with kernels of another stream).  -> d_feat [rows of feat_src, 24]: the adjoint of
    feat_src, summed over the rays that gathered each row (src_idx must be non-decreasing)."""
    return HOST_EXT.brdf_mlp_bwd(list(weights or ()), half_vec, diff_vec, feat_src, rough_src, src_idx, fwd_out, act_mask, d_out,
                                 list(grads), int(max_workgroups), _stream(), image)


def brdf_mlp_bwd_segments(weights, sets, grads, max_workgroups=0, image=None):
    """brdf_mlp_bwd over one or two ray sets in ONE launch (the evaluations of a level and of the level below share the weights).
    sets: tuples (half_vec, diff_vec, feat_src, rough_src, src_idx, fwd_out, act_mask, d_out) -> list of d_feat, one per set."""
    return HOST_EXT.brdf_mlp_bwd_sets(list(weights or ()), list(sets), list(grads), int(max_workgroups), _stream(), image)


def heads_fwd(feat, W, b, hp):
    """hp = (diffuse_mul, diffuse_bias, tint_bias, f0_bias, rough_bias)"""
    return HOST_EXT.heads_fwd(feat, W, b, list(hp), _stream())


def heads_bwd(feat, W, b, hp, d_out, gW, gb, add_into=None):
    """gW [11,24] / gb [11] are ACCUMULATED into.  add_into: another adjoint of the same rows (dense fp32 [M,24]); the result is
    added to it in place and it is returned (one launch less than `add_into += heads_bwd(...)`, the same bits)."""
    return HOST_EXT.heads_bwd(feat, W, b, list(hp), d_out, gW, gb, add_into, _stream())


def ggx_rays_fwd(V, N, r, x, off, cnt, sobol, row_of_ray, j_of_ray):
    """-> (L [R,3], half [R,3], diff [R,3], lpdf [R], mip [R], rays [R,6])"""
    return HOST_EXT.ggx_rays_fwd(V, N, r, x, off, cnt, sobol, row_of_ray, j_of_ray, _stream())


def ggx_prob(dir_in, dir_out, half, rough):
    R = dir_in.shape[0]
    out = torch.empty((R,), dtype=torch.float32, device=dir_in.device)
    _check(_lib.nmf_ggx_prob(_p(dir_in, torch.float32), _p(dir_out, torch.float32), _p(half, torch.float32),
                             _p(rough, torch.float32), C.c_int64(R), _p(out), _stream()), "nmf_ggx_prob")
    return out


def ggx_rays_bwd(V, N, r, off, sobol, row_of_ray, j_of_ray, dL, d_rays=None):
    """-> d_nr [R,4] = per-ray adjoints of (normal | roughness)"""
    return HOST_EXT.ggx_rays_bwd(V, N, r, off, sobol, row_of_ray, j_of_ray, dL, d_rays, _stream())


def ggx_rays_bwd_view(V, N, r, off, sobol, row_of_ray, j_of_ray, dL, d_rays=None):
    """-> d_nrv [R,7] = per-ray adjoints of (normal | roughness | view direction)"""
    return HOST_EXT.ggx_rays_bwd_view(V, N, r, off, sobol, row_of_ray, j_of_ray, dL, d_rays, _stream())


def shade_mix_bwd_view(V, f0, diff, cnt, row_of_ray, L, inc, brdf, d_rows):
    """shade_mix_bwd plus dV [R,3]"""
    return HOST_EXT.shade_mix_bwd_view(V, f0, diff, cnt, row_of_ray, L, inc, brdf, d_rows, _stream())


def shade_mix_fwd(V, f0, diff, cnt, row_of_ray, L, inc, brdf):
    """-> contrib [R,3]"""
    return HOST_EXT.shade_mix_fwd(V, f0, diff, cnt, row_of_ray, L, inc, brdf, _stream())


def shade_mix_bwd(V, f0, diff, cnt, row_of_ray, L, inc, brdf, d_rows):
    """-> (d_inc [R,3], d_brdf [R,3], dL [R,3], d_fd [R,6])"""
    return HOST_EXT.shade_mix_bwd(V, f0, diff, cnt, row_of_ray, L, inc, brdf, d_rows, _stream())


# ---- optimizer ----------------------------------------------------------------------------------
def adam_step(slots, n, guard=None):
    """slots: (AdamSlot * k) host array, the first n entries are applied in one launch (nmf_adam_step); guard: optional 0-d fp32
    device tensor, a non-finite value turns the launch into a no-op"""
    return HOST_EXT.adam_step(C.addressof(slots), int(n), guard, _stream())


# ---- shading glue --------------------------------------------------------------------------------
def bounce_index(counts, xyzt=None):
    """counts [M] int32 -> (bidx [M] int32, row_off [M+1] int64, cnt_rows [M] int32, inv [M] int32,
    totals [2] int64 = (R, Mb)); the caller slices bidx[:Mb] / row_off[:Mb+1] / cnt_rows[:Mb] once it has read totals.
    With xyzt [M,4]: a sixth output xyzt_rows [M,4] whose first Mb rows are xyzt[bidx]."""
    return HOST_EXT.bounce_index(counts, xyzt, _stream())


def bounce_prep_fwd_heads(bidx, normals, app, head_W, head_b, hp, xyzt, ray_id, rays, conv, feat_noise, anoise, min_rough, row_inputs=1):
    """heads_fwd(app, head_W, head_b, hp) + bounce_prep_fwd(..., heads, ...) in one launch -> (heads, V, N, r1, f0, diffuse, feat, xyz)"""
    return HOST_EXT.bounce_prep_fwd_heads(bidx, normals, app, head_W, head_b, list(hp), xyzt, ray_id, rays, conv, feat_noise, anoise,
                                          min_rough, int(row_inputs), _stream())


def bounce_index_select(weights, u, mode, mul, add=0.0, sum_w=1.0, xyzt=None):
    """select_bounces(weights, u, mode, mul, add, sum_w) + bounce_index(counts, xyzt) without materialising the counts: the count of a
    sample is evaluated inside the two launches of the index (nmf_bounce_index_select).  sum_w: float or 0-d device tensor."""
    dev_sum = sum_w if isinstance(sum_w, torch.Tensor) else None
    return HOST_EXT.bounce_index_select(weights, u, mode, mul, add, 1.0 if dev_sum is not None else sum_w, dev_sum, xyzt, _stream())


def bounce_prep_fwd(bidx, normals, app, heads, xyzt, ray_id, rays, conv, feat_noise, anoise, min_rough, row_inputs=False):
    """-> (V [Mb,3], N [Mb,3], r1 [Mb], f0 [Mb,3], diffuse [Mb,3], feat [Mb,24], xyz [Mb,3])"""
    return HOST_EXT.bounce_prep_fwd(bidx, normals, app, heads, xyzt, ray_id, rays, conv, feat_noise, anoise, min_rough,
                                    int(row_inputs), _stream())


def bounce_prep_bwd(inv, normals, heads, ray_id, rays, conv, min_rough, detach_n, dN, dr1, df0, ddiff, dfeat,
                    bidx=None, row_inputs=False):
    """row_inputs: heads is [Mb,11] and d_heads / d_app come back per bounce row ([Mb,11], [Mb,24]); row_inputs == 2: normals
    [Mb,3] and d_normals [Mb,3] are per bounce row too (inv may be None, M is taken from ray_id)"""
    return HOST_EXT.bounce_prep_bwd(inv, normals, heads, ray_id, rays, conv, float(min_rough), bool(detach_n), dN, dr1, df0, ddiff,
                                    dfeat, bidx, int(row_inputs), _stream())


def ray_compose_fwd(weight, refl_rows, inv, normals, rays, offsets, B, bg, bg_per_ray, tonemap, noclip, want_ori):
    """-> (rgb_map [B,3], acc [B], rgb_lin [B,3], ori [B] or None)"""
    return HOST_EXT.ray_compose_fwd(weight, refl_rows, inv, normals, rays, offsets, B, bg, bool(bg_per_ray), bool(tonemap),
                                    bool(noclip), bool(want_ori), _stream())


def ray_compose_bwd(weight, refl_rows, inv, normals, rays, ray_id, bg, bg_per_ray, tonemap, noclip, rgb_lin, d_rgb_map,
                    d_acc, d_ori, want_d_normals):
    """-> (d_weight [M], d_refl shaped like refl_rows or None, d_normals [M,3] or None)"""
    return HOST_EXT.ray_compose_bwd(weight, refl_rows, inv, normals, rays, ray_id, bg, bool(bg_per_ray), bool(tonemap),
                                    bool(noclip), rgb_lin, d_rgb_map, d_acc, d_ori, bool(want_d_normals), _stream())


# ---- loss terms ------------------------------------------------------------------------------------
def _dense_f32(t):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise NmfHipError("expected a float32 device tensor")
    if not (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)):
        raise NmfHipError("tensor storage must be dense")
    return t.data_ptr()


def l1_mean_fwd(tensors):
    n = len(tensors)
    out = torch.zeros((), dtype=torch.float32, device=tensors[0].device)
    ptrs = (C.c_void_p * n)(*[_dense_f32(t) for t in tensors])
    numel = (C.c_int64 * n)(*[t.numel() for t in tensors])
    _check(_lib.nmf_l1_mean_fwd(ptrs, numel, C.c_int32(n), _p(out), _stream()), "nmf_l1_mean_fwd")
    return out


def l1_mean_bwd(tensors, d_out, out=None):
    """-> gradients in the tensors' own memory order; out = existing gradient tensors of the same storage order to ADD into"""
    if out is None:
        grads = [torch.empty_like(t, memory_format=torch.preserve_format) for t in tensors]
        HOST_EXT.l1_mean_bwd_into(list(tensors), d_out, grads, False, _stream())
        return grads
    HOST_EXT.l1_mean_bwd_into(list(tensors), d_out, list(out), True, _stream())
    return out


def loss_mix_fwd(tensors, weights, scale):
    """scale * sum_i w_i * sum(x_i) -> 0-d tensor (one launch)"""
    n = len(tensors)
    out = torch.zeros((), dtype=torch.float32, device=tensors[0].device)
    ptrs = (C.c_void_p * n)(*[_dense_f32(t) for t in tensors])
    numel = (C.c_int64 * n)(*[t.numel() for t in tensors])
    w = (C.c_float * n)(*[float(v) for v in weights])
    _check(_lib.nmf_loss_mix_fwd(ptrs, numel, w, C.c_int32(n), C.c_float(scale), _p(out), _stream()), "nmf_loss_mix_fwd")
    return out


def loss_mix_bwd(shapes, weights, scale, d_out):
    """constant gradients d_out * scale * w_i shaped like the inputs (one launch)"""
    return HOST_EXT.loss_mix_bwd([list(s_) for s_ in shapes], [float(v) for v in weights], float(scale), d_out, _stream())


_loss_ws = {}


def loss_head_workspace(device, n_rays):
    """zeroed workspace of nmf_loss_head, one per (device, current stream), grown on demand (its ticket counter is zero between
    launches)"""
    key = (device, _stream())
    need = int(_lib.nmf_loss_head_workspace_bytes(C.c_int64(n_rays)))
    ws = _loss_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _loss_ws[key] = torch.zeros(max(2 * need, 4096), dtype=torch.uint8, device=device)
    return ws


def loss_head(pred, gt, d_out, scale, w_pred, w_a, w_b):
    """sqerr_fwd + loss_mix_bwd + sqerr_bwd of one chunk in one launch -> (loss 0-d, d_pred [B,3], g_a [B], g_b [B]):
    loss = sum (clip(pred) - clip(gt))^2 (summed in a fixed order, written: no zero fill), d_pred = 2 (pred - clip(gt)) *
    (d_out scale w_pred) inside [0,1], g_a / g_b filled with d_out scale w_a / w_b."""
    return HOST_EXT.loss_head(pred, gt, d_out, scale, w_pred, w_a, w_b, loss_head_workspace(pred.device, pred.shape[0]), _stream())


def bg_adjoint(acc, d_rgb):
    """(1 - acc)[:, None] * d_rgb in one launch (the background adjoint nmf_ray_compose_bwd leaves to the caller)"""
    return HOST_EXT.bg_adjoint(acc, d_rgb, _stream())


def sqerr_fwd(pred, gt):
    """-> 0-d sum (clip(pred, 0, 1) - clip(gt, 0, 1))^2 (the photometric term)"""
    return HOST_EXT.sqerr_fwd(pred, gt, _stream())


def sqerr_bwd(pred, gt, d_out):
    """-> d_pred = 2 (pred - clip(gt)) d_out inside [0, 1], 0 outside (d_out: 0-d device tensor)"""
    return HOST_EXT.sqerr_bwd(pred, gt, d_out, _stream())


# ---- total-variation regularisers --------------------------------------------------------------------
TV_KINDS = {"plane": 0, "line": 1, "env": 2}
_tv_ws = {}
_tv_scale = {}


def tv_kind(t):
    """the kind utils.TVLoss applies to a [1,C,H,W] tensor (utils.py:143: a last dimension of 1 is a line)"""
    return "line" if t.shape[-1] == 1 else "plane"


def _tv_launch(tensors, kinds, weights, scale, grads, want_value):
    """ONE nmf_tv_fwd_bwd launch over all tensors ([1,C,H,W] or [C,H,W] fp32 device tensors in any dense storage order)"""
    n = len(tensors)
    if not (n == len(kinds) == len(weights)) or (grads is not None and len(grads) != n):
        raise NmfHipError("tv: tensors / kinds / weights / grads differ in length")
    dev = tensors[0].device
    shape, xs, gs = (C.c_int32 * (3 * n))(), (C.c_int64 * (3 * n))(), (C.c_int64 * (3 * n))()
    for i, t in enumerate(tensors):
        g = grads[i] if grads is not None else None
        for u in (t, g):
            if u is None:
                continue
            if u.dtype != torch.float32 or not u.is_cuda or u.device != dev:
                raise NmfHipError("tv: expected float32 tensors on one device")
            if u.dim() not in (3, 4) or (u.dim() == 4 and u.shape[0] != 1) or (u is g and u.shape[-3:] != t.shape[-3:]):
                raise NmfHipError("tv: tensors are [1,C,H,W] (or [C,H,W]) and a gradient has its tensor's shape")
        shape[3 * i:3 * i + 3] = list(t.shape[-3:])
        xs[3 * i:3 * i + 3] = list(t.stride()[-3:])
        if g is not None:
            gs[3 * i:3 * i + 3] = list(g.stride()[-3:])
    kind = (C.c_int32 * n)(*[TV_KINDS[k] if isinstance(k, str) else int(k) for k in kinds])
    w = (C.c_float * n)(*[float(v) for v in weights])
    if not isinstance(scale, torch.Tensor):
        key = (dev, float(scale))
        if key not in _tv_scale:
            if len(_tv_scale) > 64:
                _tv_scale.clear()
            _tv_scale[key] = torch.full((), float(scale), dtype=torch.float32, device=dev)
        scale = _tv_scale[key]
    if scale.numel() != 1:
        raise NmfHipError("tv: the scale is a single device value")
    value, ws, ws_bytes = None, None, 0
    if want_value:
        need = int(_lib.nmf_tv_workspace_bytes(shape, kind, C.c_int32(n)))
        _check(min(need, 0), "nmf_tv_workspace_bytes")
        wkey = (dev, _stream())
        ws = _tv_ws.get(wkey)
        if ws is None or ws.numel() < need:                     # zeroed: the ticket is zero between launches
            ws = _tv_ws[wkey] = torch.zeros(max(2 * need, 4096), dtype=torch.uint8, device=dev)
        ws_bytes = ws.numel()
        value = torch.empty((), dtype=torch.float32, device=dev)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    gptrs = (C.c_void_p * n)(*[g.data_ptr() for g in grads]) if grads is not None else None
    _check(_lib.nmf_tv_fwd_bwd(ptrs, gptrs, shape, xs, gs if grads is not None else None, kind, w, C.c_int32(n),
                               _p(scale.reshape(()), torch.float32), _p(value), None if ws is None else C.c_void_p(ws.data_ptr()),
                               C.c_int64(ws_bytes), _stream()), "nmf_tv_fwd_bwd")
    return value


def tv_value_grad(tensors, kinds, weights, scale, grads=None, value=True):
    """-> (scale * sum_i w_i TV_i(x_i) as a 0-d tensor, grads): value and gradient in ONE launch.  kinds: 'plane' / 'line' / 'env'
    per tensor; scale: python float or 0-d device tensor.  grads: tensors to ADD scale * w_i * dTV_i/dx_i into (any dense storage
    order of the tensor's shape); None: new zero tensors in the tensors' own memory order.  value=False: the gradient only (-> None, grads)."""
    tensors = [t.detach() for t in tensors]
    if grads is None:
        grads = [torch.zeros_like(t, memory_format=torch.preserve_format) for t in tensors]
    return _tv_launch(tensors, kinds, weights, scale, list(grads), bool(value)), grads


def tv_value(tensors, kinds, weights, scale):
    """-> scale * sum_i w_i TV_i(x_i) (0-d tensor): the value mode of the same launch, nothing else is written"""
    return _tv_launch([t.detach() for t in tensors], kinds, weights, scale, None, True)


# ---- retrace selection ------------------------------------------------------------------------------
def retrace_scores(brdf, V_rows, N_rows, lpdf, w_rows, cnt_rows, row_of_ray):
    R = row_of_ray.shape[0]
    score = torch.empty(R, dtype=torch.float32, device=brdf.device)
    if R:
        _check(_lib.nmf_retrace_scores(_p(brdf, torch.float32), _p(V_rows, torch.float32), _p(N_rows, torch.float32),
                                       _p(lpdf, torch.float32), _p(w_rows, torch.float32), _p(cnt_rows, torch.int32),
                                       _p(row_of_ray, torch.int32), C.c_int64(R), _p(score), _stream()),
               "nmf_retrace_scores")
    return score


def argsort_f32(keys):
    """ascending argsort of a 1-D fp32 device tensor -> int32 indices"""
    n = keys.shape[0]
    order = torch.empty(n, dtype=torch.int32, device=keys.device)
    if n:
        nbytes = _lib.nmf_argsort_workspace_bytes(C.c_int64(n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
        _check(_lib.nmf_argsort_f32(_p(keys, torch.float32), C.c_int64(n), _p(order), _p(ws), C.c_int64(nbytes),
                                    _stream()), "nmf_argsort_f32")
    return order


def topk_select(keys, k):
    """The partition models/microfacet.py:506-537 takes from `color_contribution.argsort()`, by radix select (no full sort):
    -> (idx_top [k] int32 = argsort(keys)[n-k:] in that order, idx_rest [n-k] int32 = the other indices in index order)"""
    n = keys.shape[0]
    k = int(k)
    top = torch.empty(k, dtype=torch.int32, device=keys.device)
    rest = torch.empty(n - k, dtype=torch.int32, device=keys.device)
    if n:
        nbytes = _lib.nmf_topk_select_workspace_bytes(C.c_int64(n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=keys.device)
        _check(_lib.nmf_topk_select(_p(keys, torch.float32), C.c_int64(n), C.c_int64(k), _p(top) if k else None,
                                    _p(rest) if n - k else None, _p(ws), C.c_int64(nbytes), _stream()), "nmf_topk_select")
    return top, rest


def multi_copy(slots, n):
    """slots: (CopySlot * k) host array; copies the first n (src -> dst, with fp32 <-> fp64 conversion) in one launch"""
    return HOST_EXT.multi_copy(C.addressof(slots), int(n), _stream())


# ---- evaluation metrics (renderer.py:195-560) -----------------------------------------------------------------------
def ssim_taps(filter_size=11, filter_sigma=1.5):
    """the normalised 1-D Gaussian of utils.py:101-106, float64"""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    return filt / np.sum(filt)


def _batched(t, tail):
    t = t.reshape(-1, *t.shape[-tail:]) if t.dim() > tail else t.unsqueeze(0)
    return t.contiguous()


def ssim(a, b, max_val=1.0, k1=0.01, k2=0.03, return_map=False, filter_sigma=1.5):
    """SSIM of utils.py:90-136 (filter_size 11) over a batch: a, b fp32 device tensors [H,W,3] or [n,H,W,3] ->
    float64 [n] (the mean of each view's map), and with return_map the fp32 map [n,H-10,W-10,3].  One launch for every
    view; fp64 moments; bit-identical per view whatever else is in the batch."""
    if a.shape != b.shape or a.dim() not in (3, 4):
        raise NmfHipError(f"ssim: images must have equal shapes [H,W,3] or [n,H,W,3], got {tuple(a.shape)} / {tuple(b.shape)}")
    A, B = _batched(a, 3), _batched(b, 3)
    n, H, W, Cn = A.shape
    taps = (C.c_double * 11)(*ssim_taps(11, filter_sigma))
    mean = torch.empty(n, dtype=torch.float64, device=A.device)
    smap = torch.empty((n, max(H - 10, 0), max(W - 10, 0), Cn), dtype=torch.float32, device=A.device) if return_map else None
    nbytes = int(_lib.nmf_ssim_workspace_bytes(C.c_int64(n), C.c_int32(H), C.c_int32(W), C.c_int32(Cn)))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=A.device)
    _check(_lib.nmf_ssim(_p(A, torch.float32), _p(B, torch.float32), C.c_int64(n), C.c_int32(H), C.c_int32(W), C.c_int32(Cn),
                         C.addressof(taps), C.c_double((k1 * max_val) ** 2), C.c_double((k2 * max_val) ** 2), _p(mean),
                         _p(smap), _p(ws), C.c_int64(ws.numel()), _stream()), "nmf_ssim")
    return (mean, smap) if return_map else mean


def normal_err(pred, gt, acc, return_map=False):
    """per-view normal error of renderer.py:369-389: pred, gt fp32 device normals [n, P, 3] with the views' alpha acc [n, P]
    (or one view: [P, 3] / [P]) -> float64 [n] = sum(err * acc) / sum(acc) in degrees (NaN when sum(acc) == 0), and with
    return_map the fp32 err * acc in acc's shape."""
    if pred.shape != gt.shape or pred.dim() not in (2, 3) or pred.shape[-1] != 3 or pred.shape[:-1] != acc.shape:
        raise NmfHipError(f"normal_err: shapes {tuple(pred.shape)} / {tuple(gt.shape)} / {tuple(acc.shape)}")
    n = pred.shape[0] if pred.dim() == 3 else 1
    P, G, Acc = pred.reshape(n, -1, 3).contiguous(), gt.reshape(n, -1, 3).contiguous(), acc.reshape(n, -1).contiguous()
    n_px = P.shape[1]
    out = torch.empty(n, dtype=torch.float64, device=P.device)
    emap = torch.empty_like(Acc) if return_map else None
    nbytes = int(_lib.nmf_normal_err_workspace_bytes(C.c_int64(n), C.c_int64(n_px)))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=P.device)
    _check(_lib.nmf_normal_err(_p(P, torch.float32), _p(G, torch.float32), _p(Acc, torch.float32), C.c_int64(n),
                               C.c_int64(n_px), _p(out), _p(emap), _p(ws), C.c_int64(ws.numel()), _stream()), "nmf_normal_err")
    return (out, emap.reshape(acc.shape)) if return_map else out


# ---- relighting evaluation (scripts/relighting_calc.ipynb, renderer.py:425-429; csrc/relight_eval.hip) ---------------------------
def _relight_images(what, pred, gt=None):
    """pred [H,W,3] or [n,H,W,3] (and gt of the same pixels with 4 channels), fp32 device tensors -> (pred, gt) contiguous, n, H, W"""
    if pred.dim() not in (3, 4) or pred.shape[-1] != 3 or (gt is not None and (gt.shape[:-1] != pred.shape[:-1] or gt.shape[-1] != 4)):
        raise NmfHipError(f"{what}: pred is [H,W,3] or [n,H,W,3] and gt its RGBA counterpart, got {tuple(pred.shape)}"
                          + (f" / {tuple(gt.shape)}" if gt is not None else ""))
    for t in (pred, gt):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise NmfHipError(f"{what}: fp32 device tensors (no CPU path), got {t.dtype} on {t.device}")
    P, G = _batched(pred, 3), (_batched(gt, 3) if gt is not None else None)
    return P, G, P.shape[0], P.shape[1], P.shape[2]


def relight_frame(rgb_lin, acc):
    """nmf_relight_frame: the linear HDR frame the reference stores (renderer.py:425-429) from the composited radiance rgb_lin [..., 3]
    and the opacity acc [...]: srgb_inverse(srgb_noclip(rgb_lin) + (1 - acc)), in rgb_lin's shape"""
    if rgb_lin.dim() < 2 or rgb_lin.shape[-1] != 3 or acc.shape != rgb_lin.shape[:-1]:
        raise NmfHipError(f"relight_frame: rgb_lin [..., 3] and acc [...], got {tuple(rgb_lin.shape)} / {tuple(acc.shape)}")
    L, A = rgb_lin.contiguous(), acc.contiguous()
    ptr = _p(L, torch.float32), _p(A, torch.float32)
    out = torch.empty_like(L)
    n, h, w = (L.shape[0], L.shape[1], L.shape[2]) if L.dim() == 4 else (1, 1, A.numel())
    _check(_lib.nmf_relight_frame(*ptr, n, h, w, _p(out), _stream()), "nmf_relight_frame")
    return out


def relight_ratio(pred, gt):
    """nmf_relight_ratio (relighting_calc.ipynb cell lines 232-233): pred [n,H,W,3], gt [n,H,W,4] (or one image) -> (float64 [n,3] sums
    of gt_c / max(pred_c, 1e-7) over the pixels with gt_a > 0.5 and min_c pred_c > 0.01, int64 [n] counts of those pixels)"""
    P, G, n, H, W = _relight_images("relight_ratio", pred, gt)
    sums = torch.empty((n, 3), dtype=torch.float64, device=P.device)
    count = torch.empty(n, dtype=torch.int64, device=P.device)
    ws = torch.empty(max(int(_lib.nmf_relight_ratio_workspace_bytes(n, H, W)), 16), dtype=torch.uint8, device=P.device)
    _check(_lib.nmf_relight_ratio(_p(P), _p(G), n, H, W, _p(sums), _p(count), _p(ws), ws.numel(), _stream()), "nmf_relight_ratio")
    return sums, count


def relight_adjust(pred, gt, multi):
    """nmf_relight_adjust (cell lines 243-246): -> (tp, tg fp32 in pred's shape, sqerr float64 [n]): the prediction times the per-channel
    multiplier blended onto white with gt's alpha, and gt on white, both tonemapped and clipped; sqerr = sum (tp - tg)^2 per image"""
    P, G, n, H, W = _relight_images("relight_adjust", pred, gt)
    m = [float(v) for v in np.asarray(multi, dtype=np.float32).reshape(-1)]
    if len(m) != 3:
        raise NmfHipError("relight_adjust: multi is one multiplier per channel")
    tp, tg = torch.empty_like(P), torch.empty_like(P)
    sqerr = torch.empty(n, dtype=torch.float64, device=P.device)
    ws = torch.empty(max(int(_lib.nmf_relight_adjust_workspace_bytes(n, H, W)), 16), dtype=torch.uint8, device=P.device)
    _check(_lib.nmf_relight_adjust(_p(P), _p(G), *m, n, H, W, _p(tp), _p(tg), _p(sqerr), _p(ws), ws.numel(), _stream()),
           "nmf_relight_adjust")
    return tp.reshape(pred.shape), tg.reshape(pred.shape), sqerr


# ---- material maps of the evaluation pass (renderer.py:440-463) ------------------------------------------------------
MATERIAL_MAPS = ("albedo", "roughness", "diffuse", "tint", "spec")          # the [B,15] block of nmf_material_maps, 3 columns each


def heads_edit(heads, xyz, edits):
    """nmf_heads_edit: the material edits `edits` (fp32 [K,32], nmf_amd.edit.pack; read on the host, so a host table costs no
    copy) applied IN PLACE to the head rows `heads` [n,11] of the samples at the world positions xyz [n,3] or [n,4] (xyzt rows; the
    fourth column is not read).  None or K = 0: nothing is launched.  -> heads"""
    _p(heads, torch.float32)        # refuses host tensors before the stream is asked for (there is none without a GPU)
    _p(xyz, torch.float32)
    HOST_EXT.heads_edit(heads, xyz, edits, _stream())
    return heads


def material_maps(app, normals, weight, offsets, rays, head_W, head_b, head_p, conv, acc, bg, inv=None, row_off=None, cnt=None,
                  incoming=None, brdf_weight=None, xyz=None, edits=None):
    """nmf_material_maps: the level-0 material maps of B rays from their M kept samples -> fp32 [B,15] (albedo | roughness |
    diffuse | tint | spec, 3 columns each).  app [M,24], normals [M,3], weight [M], offsets int64 [B+1], rays [B,6], head_W [11,24],
    head_b [11], head_p = (diffuse_mul, diffuse_bias, tint_bias, f0_bias, rough_bias), conv [9,3], acc [B], bg [3]; the bounce rows
    inv int32 [M], row_off int64 [Mb+1], cnt int32 [Mb], incoming / brdf_weight [R,3] (all None: no row, spec and tint are 0).
    edits (fp32 [K,32], nmf_amd.edit.pack) with xyz [M,3] or [M,4], the samples' positions: nmf_material_maps_edit, the edits applied
    to each sample's head outputs (K = 0: the bits of the call without them)."""
    _p(app, torch.float32)          # refuses host tensors before the stream is asked for (there is none without a GPU)
    if len(head_p) != 5:
        raise NmfHipError("material_maps: head_p = (diffuse_mul, diffuse_bias, tint_bias, f0_bias, rough_bias)")
    return HOST_EXT.material_maps(app, normals, weight, offsets, rays, head_W, head_b, [float(v) for v in head_p], conv, inv, row_off, cnt,
                                  incoming, brdf_weight, acc, bg, _stream(), xyz, edits)


# ---- mesh export: marching cubes over a dense volume (csrc/mesh.hip) ------------------------------------------------------
MC_INDEX_MAX = 2 ** 31 - 1          # faces are int32 indices: V and 3 F stay below


def mc_case_triangles(case_index):
    """the edge triples of one of the 256 cases (host table lookup) -> list of (e0, e1, e2); edge and corner numbering: nmf_hip.h"""
    out = (C.c_int8 * 16)()
    n = _lib.nmf_mc_case_triangles(C.c_int(int(case_index)), out)
    if n < 0:
        raise NmfHipError(f"nmf_mc_case_triangles failed: {_lib.nmf_last_error_string().decode()} [{n}]")
    return [tuple(out[3 * t:3 * t + 3]) for t in range(n)]


def mc_count(vol, level):
    """count pass -> (cases uint8 [N], vcount int32 [N], tcount int32 [N]), views of ONE workspace of nmf_mc_workspace_bytes"""
    ptr = _p(vol, torch.float32)
    if vol.dim() != 3:
        raise NmfHipError(f"marching cubes: the volume is [Gx, Gy, Gz], got {tuple(vol.shape)}")
    g = [int(v) for v in vol.shape]
    n = g[0] * g[1] * g[2]
    ws = torch.empty(max(int(_lib.nmf_mc_workspace_bytes(*g)), 16), dtype=torch.uint8, device=vol.device)
    vcount, tcount, cases = ws[:4 * n].view(torch.int32), ws[4 * n:8 * n].view(torch.int32), ws[8 * n:9 * n]
    _check(_lib.nmf_mc_count(ptr, *g, C.c_float(float(level)), _p(cases), _p(vcount), _p(tcount), _stream()), "nmf_mc_count")
    return cases, vcount, tcount


def mc_emit(vol, level, cases, vscan, tscan, n_verts, n_faces):
    """emit pass over the INCLUSIVE sums of mc_count's counts -> (verts fp32 [V, 3], faces int32 [F, 3])"""
    g = [int(v) for v in vol.shape]
    verts = torch.empty((n_verts, 3), dtype=torch.float32, device=vol.device)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=vol.device)
    _check(_lib.nmf_mc_emit(_p(vol, torch.float32), *g, C.c_float(float(level)), _p(cases, torch.uint8), _p(vscan, torch.int32),
                            _p(tscan, torch.int32), C.c_int64(n_verts), C.c_int64(n_faces), _p(verts), _p(faces), _stream()),
           "nmf_mc_emit")
    return verts, faces


def marching_cubes(vol, level):
    """Indexed marching cubes of a dense fp32 device volume [Gx, Gy, Gz] at iso-level `level` (inside: vol > level) ->
    (verts fp32 [V, 3] in lattice index units, faces int32 [F, 3], normals from inside to outside).  Vertices are welded (one per
    sign-changing lattice edge) and the order is the lattice order: two runs give identical bytes.  Count pass, in-place scan of
    the two counts (torch.cumsum: plumbing), ONE read-back of (V, F), emit pass.  An empty surface gives [0, 3] tensors."""
    if not vol.is_cuda:
        raise NmfHipError("nmf_amd operators need device tensors (no CPU path)")
    vol = vol.contiguous()
    cases, vcount, tcount = mc_count(vol, level)
    # the totals in int64 (the int32 running sums would wrap silently on a volume that must be refused)
    rb = Readback.of(vol.device).start(torch.stack([vcount.sum(), tcount.sum()]))
    torch.cumsum(vcount, 0, dtype=torch.int32, out=vcount)
    torch.cumsum(tcount, 0, dtype=torch.int32, out=tcount)
    V, F = rb.get()
    if V > MC_INDEX_MAX or 3 * F > MC_INDEX_MAX:
        raise NmfHipError(f"marching cubes: {V} vertices / {F} faces do not fit int32 face indices (V and 3 F at most 2^31 - 1)")
    return mc_emit(vol, level, cases, vcount, tcount, V, F)


# ---- camera paths: rays from a pose, the finished 8-bit frame (csrc/camera.hip; renderer.evaluation_path) ----------------------------
def depth_colour_table():
    """the default colour table of the depth panel, uint8 [256, 3] (host): the analytic "jet" in float64, s = q / 255,
    r, g, b = clip(1.5 - |4 s - 3|, |4 s - 2|, |4 s - 1|, 0, 1), byte = floor(255 c + 0.5).  The reference maps depth through OpenCV's
    COLORMAP_JET table (utils.visualize_depth_numpy), which differs from the formula by a few levels"""
    s = np.arange(256, dtype=np.float64) / 255.0
    c = np.stack([np.clip(1.5 - np.abs(4.0 * s - k), 0.0, 1.0) for k in (3.0, 2.0, 1.0)], -1)
    return np.floor(255.0 * c + 0.5).astype(np.uint8)


_depth_lut = {}


def _device_lut(device):
    key = str(device)
    if key not in _depth_lut:
        _depth_lut[key] = torch.from_numpy(depth_colour_table()).to(device)
    return _depth_lut[key]


def camera_rays(c2w, fx, fy, cx, cy, H, W, device="cuda", out=None):
    """nmf_camera_rays: the [H W, 6] rays (origin | unit direction) of the pinhole camera with camera-to-world matrix c2w (host values,
    [3, 4] or [4, 4], OpenCV axes as BlenderDataset.poses) -- the loader's construction (pixel centres at +0.5, directions @ R^T) on the
    device.  out: an fp32 device tensor of 6 H W elements to fill (one buffer for a whole path); default: a new one on `device`."""
    H, W = int(H), int(W)
    if out is None:
        if torch.device(device).type != "cuda":
            raise NmfHipError("camera_rays: nmf_amd operators need device tensors (no CPU path)")
        if H < 1 or W < 1:
            raise NmfHipError(f"camera_rays: H and W are at least 1, got {H} x {W}")
        out = torch.empty((H * W, 6), dtype=torch.float32, device=device)
    ptr = _p(out, torch.float32)
    if out.numel() != 6 * H * W:
        raise NmfHipError(f"camera_rays: out holds {out.numel()} values, {H} x {W} pixels need {6 * H * W}")
    m = np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)
    if m.shape not in ((3, 4), (4, 4)):
        raise NmfHipError(f"camera_rays: c2w is [3, 4] or [4, 4], got {m.shape}")
    pose = [float(v) for v in m[:3, :3].reshape(-1)] + [float(v) for v in m[:3, 3]]
    with torch.cuda.device(out.device):
        _check(_lib.nmf_camera_rays(*pose, float(fx), float(fy), float(cx), float(cy), H, W, ptr, _stream()), "nmf_camera_rays")
    return out.view(H * W, 6)


def frame_finish(H, W, rgb=None, depth=None, normal=None, acc=None, near_far=(0.0, 1.0), lut="jet", out=None):
    """nmf_frame_finish: the float maps of one frame (each an fp32 device tensor of H W pixels, or None) -> uint8 [H, n_panels W, 3], the
    panels side by side in the order rgb | depth | normal | acc with the reference's 8-bit conversions (include/nmf_hip.h).  lut: "jet"
    (depth_colour_table, cached per device), None (grey depth) or a uint8 [256, 3] device tensor.  out: the strip to fill."""
    H, W = int(H), int(W)
    maps = (("rgb", rgb, 3), ("depth", depth, 1), ("normal", normal, 3), ("acc", acc, 1))
    given = [t for _, t, _ in maps if t is not None]
    if not given:
        raise NmfHipError("frame_finish: no panel (rgb, depth, normal and acc are all None)")
    ptrs = []
    for name, t, c in maps:
        if t is not None:
            if not t.is_cuda:
                raise NmfHipError(f"frame_finish: {name} must be a device tensor (no CPU path)")
            if t.device != given[0].device:
                raise NmfHipError(f"frame_finish: {name} is on another device")
            if t.numel() != c * H * W:
                raise NmfHipError(f"frame_finish: {name} holds {t.numel()} values, {H} x {W} pixels need {c * H * W}")
        ptrs.append(_p(t, torch.float32))
    dev, n = given[0].device, len(given)
    if isinstance(lut, str):
        if lut != "jet":
            raise NmfHipError(f"frame_finish: unknown colour table '{lut}'")
        lut = _device_lut(dev) if depth is not None else None
    if lut is not None and (lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3) or lut.device != dev):
        raise NmfHipError("frame_finish: lut is a uint8 [256, 3] tensor on the maps' device")
    if out is None:
        out = torch.empty((H, n * W, 3), dtype=torch.uint8, device=dev)
    if out.numel() != 3 * n * H * W or out.device != dev:
        raise NmfHipError(f"frame_finish: out holds {out.numel()} bytes on {out.device}, {n} panels of {H} x {W} need {3 * n * H * W}")
    with torch.cuda.device(dev):
        _check(_lib.nmf_frame_finish(*ptrs, float(near_far[0]), float(near_far[1]), _p(lut, torch.uint8), H, W, _p(out, torch.uint8),
                                     _stream()), "nmf_frame_finish")
    return out.view(H, n * W, 3)


# ---- texture atlas of an exported mesh (csrc/atlas.hip; nmf_amd/mesh.py:bake_textures) ----------------------------------------------
def atlas_texels(verts, faces, W, T, t0=0, n=None, check_faces=True, out=None):
    """nmf_atlas_texels: the owning face (int32 [n], -1: none) and the world position (fp32 [n, 3]) of the texels t0 .. t0 + n - 1 of
    the W x W atlas with T x T squares over the mesh verts fp32 [V, 3], faces int32 [F, 3] (layout: include/nmf_hip.h,
    nmf_amd.mesh.atlas_layout).  n None: to the end of the atlas.  check_faces: one min / max reduction of the indices first; an
    index outside [0, V) is refused (NMF_ERANGE) before anything is written -- a caller that walks the atlas in chunks checks once.
    out: the (pos, face_of) tensors to fill.  -> (pos, face_of)"""
    vp, fp = _p(verts, torch.float32), _p(faces, torch.int32)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.device != verts.device:
        raise NmfHipError(f"atlas_texels: verts [V, 3] and faces [F, 3] on one device, got {tuple(verts.shape)} and {tuple(faces.shape)}")
    W, T, t0 = int(W), int(T), int(t0)
    n = W * W - t0 if n is None else int(n)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if check_faces and F > 0:
        lo, hi = (int(v) for v in torch.stack([faces.min(), faces.max()]).tolist())
        if lo < 0 or hi >= V:
            raise NmfHipError(f"nmf_atlas_texels failed: face indices {lo}..{hi} leave [0, {V}) [-2]")
    if out is None:
        out = (torch.empty((max(n, 0), 3), dtype=torch.float32, device=verts.device),
               torch.empty((max(n, 0),), dtype=torch.int32, device=verts.device))
    pos, face_of = out
    if pos.numel() != 3 * max(n, 0) or face_of.numel() != max(n, 0) or pos.device != verts.device or face_of.device != verts.device:
        raise NmfHipError(f"atlas_texels: out holds {pos.numel()} and {face_of.numel()} values, {n} texels need {3 * n} and {n}")
    with torch.cuda.device(verts.device):
        _check(_lib.nmf_atlas_texels(vp, fp, V, F, W, T, t0, n, _p(pos), _p(face_of), _stream()), "nmf_atlas_texels")
    return pos, face_of


def atlas_store(face_of, albedo, f0, roughness, normal, t0, W, albedo_tex=None, f0_tex=None, rough_tex=None, normal_tex=None):
    """nmf_atlas_store: the attributes of the texels t0 .. t0 + n - 1 (face_of int32 [n]; albedo, f0, normal fp32 [n, 3], roughness
    fp32 [n]; the input of a plane that is None may be None) quantised IN PLACE into the uint8 planes of the W x W atlas: albedo_tex,
    f0_tex, normal_tex [W, W, 3], rough_tex [W, W] (include/nmf_hip.h: sRGB albedo, linear f0 and roughness, 127 v + 128 normals;
    unowned texels get the fill values).  A plane that is None is skipped."""
    n, W, t0 = int(face_of.numel()), int(W), int(t0)
    ptrs = [_p(face_of, torch.int32)]
    for name, t, c in (("albedo", albedo, 3), ("f0", f0, 3), ("roughness", roughness, 1), ("normal", normal, 3)):
        if t is not None and (t.numel() != c * n or t.device != face_of.device):
            raise NmfHipError(f"atlas_store: {name} holds {t.numel()} values on {t.device}, {n} texels need {c * n}")
        ptrs.append(_p(t, torch.float32))
    planes = []
    for name, t, c in (("albedo_tex", albedo_tex, 3), ("f0_tex", f0_tex, 3), ("rough_tex", rough_tex, 1), ("normal_tex", normal_tex, 3)):
        if t is not None and (t.numel() != c * W * W or t.device != face_of.device):
            raise NmfHipError(f"atlas_store: {name} holds {t.numel()} bytes on {t.device}, a {W} x {W} atlas needs {c * W * W}")
        planes.append(_p(t, torch.uint8))
    with torch.cuda.device(face_of.device):
        _check(_lib.nmf_atlas_store(*ptrs, t0, n, W, *planes, _stream()), "nmf_atlas_store")


# ---- scene composition (csrc/compose.hip; nmf_amd/compose.py) -------------------------------------------------------------------------
MERGE_MAX_LISTS = 8


class MergeLists(C.Structure):
    _fields_ = [("offsets", C.c_void_p * MERGE_MAX_LISTS), ("z", C.c_void_p * MERGE_MAX_LISTS), ("dst", C.c_void_p * MERGE_MAX_LISTS),
                ("scale", C.c_float * MERGE_MAX_LISTS), ("M", C.c_int64 * MERGE_MAX_LISTS)]


def _placement_args(R, c, s):
    """host float32 blocks of a placement x_w = s R x_l + c; R may be an object with .R, .t and .s (nmf_amd.compose.Placement)"""
    if hasattr(R, "R") and hasattr(R, "t") and hasattr(R, "s"):
        R, c, s = R.R, R.t, R.s
    r = np.asarray(R, dtype=np.float64).reshape(-1)
    t = np.zeros(3) if c is None else np.asarray(c, dtype=np.float64).reshape(-1)
    if r.size != 9 or t.size != 3:
        raise NmfHipError("a placement has a 3x3 rotation and a translation of 3")
    return (C.c_float * 9)(*[float(v) for v in r]), (C.c_float * 3)(*[float(v) for v in t]), float(np.float32(s))


def rays_place(rays, R, c=None, s=1.0, inverse=False, out=None):
    """nmf_rays_place: rays fp32 [B, 6] (origin | direction) between the world and an object's frame under the placement
    x_w = s R x_l + c (R 3x3, c 3, s: host numbers, or R a nmf_amd.compose.Placement).  inverse: world -> local, o' = R^T (o - c) / s,
    d' = R^T d; otherwise local -> world, o' = s R o + c, d' = R d.  Directions are not renormalised.  -> out (a new tensor, or
    `out`, which may be `rays`)"""
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
        raise NmfHipError(f"rays_place: rays are [B, 6], got {tuple(getattr(rays, 'shape', ()))}")
    rp = _p(rays, torch.float32)
    if out is None:
        out = torch.empty_like(rays)
    if out.shape != rays.shape or out.device != rays.device:
        raise NmfHipError("rays_place: out must have the shape and device of rays")
    Rc, cc, sc = _placement_args(R, c, s)
    with torch.cuda.device(rays.device):
        _check(_lib.nmf_rays_place(rp, Rc, cc, sc, 1 if inverse else 0, int(rays.shape[0]), _p(out, torch.float32), _stream()),
               "nmf_rays_place")
    return out


def merge_rank(offsets, zs, scales, B):
    """nmf_merge_rank: K <= 8 per-ray sample lists over the same B rays (offsets[k] int64 [>= B+1], zs[k] fp32 [M_k] non-decreasing
    inside a ray, scales[k] > 0) -> (dst: a list of int64 [M_k], the place of every sample in the list merged by world depth
    scales[k] * zs[k] -- stable: ties by list index, then by original order --, offsets_m int64 [B+1])"""
    K, B = len(offsets), int(B)
    if len(zs) != K or len(scales) != K:
        raise NmfHipError("merge_rank: offsets, zs and scales are lists of one length")
    L = MergeLists()
    dst = []
    dev = offsets[0].device if K else torch.device("cuda")
    for k in range(min(K, MERGE_MAX_LISTS)):
        if offsets[k].numel() < B + 1 or zs[k].dim() != 1 or offsets[k].device != dev or zs[k].device != dev:
            raise NmfHipError(f"merge_rank: list {k} needs offsets of B + 1 = {B + 1} entries and a 1-d z on one device")
        d = torch.empty(zs[k].shape[0], dtype=torch.int64, device=dev)
        dst.append(d)
        L.offsets[k], L.z[k], L.dst[k] = _p(offsets[k], torch.int64), _p(zs[k], torch.float32), _p(d)
        L.scale[k], L.M[k] = float(scales[k]), int(zs[k].shape[0])
    offsets_m = torch.empty(B + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _check(_lib.nmf_merge_rank(K, C.byref(L), B, _p(offsets_m), _stream()), "nmf_merge_rank")
    return dst, offsets_m


def merge_scatter(dst, M_total, part=0, sigma=None, dist=None, z=None, normal=None, ray_id=None, inv=None, sigma_ratio=1.0, scale=1.0,
                  R=None, row_base=0, out=None):
    """nmf_merge_scatter: the rows of one list written IN PLACE to their places dst int64 [M_k] in the merged arrays
    out = dict(sigma, dist, z fp32 [M_total]; normal fp32 [M_total, 3]; ray_id, part, src, inv int32 [M_total]): every array present in
    `out` is written (sigma * sigma_ratio, dist, scale * z, R normal, ray_id, part, the row's index, inv + row_base or -1) and needs
    its input.  -> out"""
    out = out or {}
    M_k, M_total = int(dst.shape[0]), int(M_total)
    for name, t, c in (("sigma", sigma, 1), ("dist", dist, 1), ("z", z, 1), ("normal", normal, 3), ("ray_id", ray_id, 1), ("inv", inv, 1)):
        if t is not None and (t.numel() != c * M_k or t.device != dst.device):
            raise NmfHipError(f"merge_scatter: {name} holds {t.numel()} values on {t.device}, {M_k} rows need {c * M_k}")
    for name, t in out.items():
        c = 3 if name == "normal" else 1
        if name not in ("sigma", "dist", "z", "normal", "ray_id", "part", "src", "inv"):
            raise NmfHipError(f"merge_scatter: unknown output '{name}'")
        if t.numel() != c * M_total or t.device != dst.device:
            raise NmfHipError(f"merge_scatter: out['{name}'] holds {t.numel()} values on {t.device}, {M_total} rows need {c * M_total}")
    f, i = torch.float32, torch.int32
    Rc = _placement_args(R, None, 1.0)[0] if R is not None else None
    o = out.get
    with torch.cuda.device(dst.device):
        _check(_lib.nmf_merge_scatter(M_k, M_total, _p(dst, torch.int64), _p(sigma, f), _p(dist, f), _p(z, f), _p(normal, f), _p(ray_id, i),
                                      _p(inv, i), float(sigma_ratio), float(scale), Rc, int(part), int(row_base), _p(o("sigma"), f),
                                      _p(o("dist"), f), _p(o("z"), f), _p(o("normal"), f), _p(o("ray_id"), i), _p(o("part"), i),
                                      _p(o("src"), i), _p(o("inv"), i), _stream()), "nmf_merge_scatter")
    return out


# ---- multi-sample frames: rays of a pixel list, per-pixel accumulation, the active list (csrc/accum.hip; nmf_amd/multisample.py) ------
ACCUM_PLANES, ACCUM_TILE = 15, 256          # NMF_ACCUM_PLANES, NMF_ACCUM_TILE of include/nmf_hip.h


def accum_state_bytes(H, W):
    """nmf_accum_state_bytes: the bytes of the per-pixel state of an H x W frame (host arithmetic)"""
    n = int(_lib.nmf_accum_state_bytes(int(H), int(W)))
    if n <= 0:
        raise NmfHipError(f"accum_state_bytes: a frame is at least 1 x 1 and at most 2^31 - 1 pixels, got {H} x {W}")
    return n


def _pixel_list(pix, what, device):
    if pix is None:
        return None, 0
    if pix.dtype != torch.int32 or pix.dim() != 1 or not pix.is_cuda or pix.device != device:
        raise NmfHipError(f"{what}: pix is a 1-d int32 tensor on the device of the frame")
    return pix, int(pix.shape[0])


def camera_rays_at(c2w, fx, fy, cx, cy, H, W, jitter=(0.5, 0.5), seed=0, pix=None, device="cuda", out=None):
    """nmf_camera_rays_at: the rays of the pixels pix (int32, ascending; None: all H W) of camera_rays' camera through the point
    jitter = (jx, jy) in [0, 1]^2 of each pixel, rotated per pixel by the hash of (pixel, seed) when seed != 0 (include/nmf_hip.h).
    -> fp32 [n, 6] (out: a device tensor of at least 6 n values whose first n rows are filled and returned)"""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise NmfHipError(f"camera_rays_at: H and W are at least 1, got {H} x {W}")
    device = out.device if out is not None else (pix.device if pix is not None else torch.device(device))
    if torch.device(device).type != "cuda":
        raise NmfHipError("camera_rays_at: nmf_amd operators need device tensors (no CPU path)")
    pix, n = _pixel_list(pix, "camera_rays_at", device)
    rows = H * W if pix is None else n
    if out is None:
        out = torch.empty((rows, 6), dtype=torch.float32, device=device)
    ptr = _p(out, torch.float32)
    if out.numel() < 6 * rows:
        raise NmfHipError(f"camera_rays_at: out holds {out.numel()} values, {rows} rays need {6 * rows}")
    m = np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)
    if m.shape not in ((3, 4), (4, 4)):
        raise NmfHipError(f"camera_rays_at: c2w is [3, 4] or [4, 4], got {m.shape}")
    pose = [float(v) for v in m[:3, :3].reshape(-1)] + [float(v) for v in m[:3, 3]]
    if rows == 0:          # an empty list (its data pointer is null, which the entry point reads as "all pixels")
        return out.view(-1)[:0].view(0, 6)
    with torch.cuda.device(out.device):
        _check(_lib.nmf_camera_rays_at(*pose, float(fx), float(fy), float(cx), float(cy), H, W, float(jitter[0]), float(jitter[1]),
                                       int(seed) & 0xFFFFFFFF, _p(pix), n, ptr, _stream()), "nmf_camera_rays_at")
    return out.view(-1)[:6 * rows].view(rows, 6)


def accum_update(state, H, W, rgb_lin, acc, rgb_map, depth=None, normal=None, pix=None):
    """nmf_accum_update: one pass folded into the state (a zeroed uint8 / int32 / fp32 device tensor of accum_state_bytes) for the
    pixels pix (None: all): rgb_lin [n, 3], acc [n], rgb_map [n, 3], optionally depth [n] and normal [n, 3], indexed by list entry"""
    H, W = int(H), int(W)
    if not state.is_cuda or state.numel() * state.element_size() < accum_state_bytes(H, W):
        raise NmfHipError(f"accum_update: the state is a device tensor of {accum_state_bytes(H, W)} bytes")
    pix, n = _pixel_list(pix, "accum_update", state.device)
    rows = H * W if pix is None else n
    for name, t, c in (("rgb_lin", rgb_lin, 3), ("acc", acc, 1), ("rgb_map", rgb_map, 3), ("depth", depth, 1), ("normal", normal, 3)):
        if t is None and name in ("depth", "normal"):
            continue
        if t is None or not t.is_cuda or t.device != state.device or t.numel() != c * rows:
            raise NmfHipError(f"accum_update: {name} is a device tensor of {c * rows} values ({rows} pixels)")
    f = torch.float32
    if rows == 0:          # an empty list (its data pointer is null, which the entry point reads as "all pixels")
        return
    with torch.cuda.device(state.device):
        _check(_lib.nmf_accum_update(_p(state), H, W, _p(pix), n, _p(rgb_lin, f), _p(acc, f), _p(rgb_map, f), _p(depth, f),
                                     _p(normal, f), _stream()), "nmf_accum_update")


def accum_active(state, H, W, min_spp, max_spp, tol, out=None, n_out=None):
    """nmf_accum_active: the ascending int32 list of the pixels with count < min_spp, or count < max_spp and a standard error above tol
    -> (list [H W] of which the first n_out[0] entries are written, n_out int32 [1]); both on the device, the caller reads n_out"""
    H, W = int(H), int(W)
    if not state.is_cuda or state.numel() * state.element_size() < accum_state_bytes(H, W):
        raise NmfHipError(f"accum_active: the state is a device tensor of {accum_state_bytes(H, W)} bytes")
    if out is None:
        out = torch.empty(H * W, dtype=torch.int32, device=state.device)
    if n_out is None:
        n_out = torch.zeros(1, dtype=torch.int32, device=state.device)
    if out.numel() < H * W or n_out.numel() < 1 or out.device != state.device or n_out.device != state.device:
        raise NmfHipError(f"accum_active: out holds {H * W} int32 and n_out one, on the state's device")
    with torch.cuda.device(state.device):
        _check(_lib.nmf_accum_active(_p(state), H, W, int(min_spp), int(max_spp), float(tol), _p(out, torch.int32),
                                     _p(n_out, torch.int32), _stream()), "nmf_accum_active")
    return out, n_out


def accum_resolve(state, H, W, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False, want=("rgb_map", "acc", "depth", "normal", "se", "count")):
    """nmf_accum_resolve: the finished maps named in `want` -> dict(rgb_map [P, 3], acc [P], depth [P], normal [P, 3], se [P],
    count [P] as float): the tonemap and the background of nmf_ray_compose_fwd applied to the MEAN radiance, plain means otherwise"""
    H, W = int(H), int(W)
    if not state.is_cuda or state.numel() * state.element_size() < accum_state_bytes(H, W):
        raise NmfHipError(f"accum_resolve: the state is a device tensor of {accum_state_bytes(H, W)} bytes")
    names = ("rgb_map", "acc", "depth", "normal", "se", "count")
    if not want or set(want) - set(names):
        raise NmfHipError(f"accum_resolve: want is a non-empty choice of {names}")
    P = H * W
    out = {k: torch.empty((P, 3) if k in ("rgb_map", "normal") else (P,), dtype=torch.float32, device=state.device) for k in names if k in want}
    with torch.cuda.device(state.device):
        _check(_lib.nmf_accum_resolve(_p(state), H, W, float(bg[0]), float(bg[1]), float(bg[2]), int(bool(tonemap)), int(bool(noclip)),
                                      *[_p(out.get(k)) for k in names], _stream()), "nmf_accum_resolve")
    return out


# ---- denoised frames: the variance-guided a-trous filter over the accumulator state (csrc/denoise.hip; nmf_amd/multisample.py) ---------
DENOISE_PLANES, DENOISE_MAX_LEVELS = 19, 8          # NMF_DENOISE_PLANES, NMF_DENOISE_MAX_LEVELS of include/nmf_hip.h
DENOISE_OUTPUTS = ("rgb_map", "rgb_lin", "acc", "se")


def denoise_workspace_bytes(H, W):
    """nmf_denoise_workspace_bytes: the bytes of the filter's workspace for an H x W frame (host arithmetic)"""
    n = int(_lib.nmf_denoise_workspace_bytes(int(H), int(W)))
    if n <= 0:
        raise NmfHipError(f"denoise_workspace_bytes: a frame is at least 1 x 1 and at most 2^31 - 1 pixels, got {H} x {W}")
    return n


def _denoise_buffers(what, H, W, state, workspace):
    for name, t, need in (("state", state, accum_state_bytes), ("workspace", workspace, denoise_workspace_bytes)):
        if t is None:
            continue
        if not t.is_cuda or t.numel() * t.element_size() < need(H, W):
            raise NmfHipError(f"{what}: the {name} is a device tensor of {need(H, W)} bytes")
    if state is not None and workspace is not None and state.device != workspace.device:
        raise NmfHipError(f"{what}: the state and the workspace are on one device")


def _denoise_outputs(what, P, want, out, device):
    if not want or set(want) - set(DENOISE_OUTPUTS):
        raise NmfHipError(f"{what}: want is a non-empty choice of {DENOISE_OUTPUTS}")
    res = {}
    for k in DENOISE_OUTPUTS:
        if k not in want:
            continue
        n = 3 * P if k in ("rgb_map", "rgb_lin") else P
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.empty((P, 3) if n == 3 * P else (P,), dtype=torch.float32, device=device)
        elif not t.is_cuda or t.device != device or t.dtype != torch.float32 or t.numel() != n:
            raise NmfHipError(f"{what}: out['{k}'] is a float32 tensor of {n} values on the workspace's device")
        res[k] = t
    return res


def denoise_prepare(state, workspace, H, W):
    """nmf_denoise_prepare: fixed, the blurred variance, the depth gradient and set 0 of the workspace from the accumulator state"""
    H, W = int(H), int(W)
    _denoise_buffers("denoise_prepare", H, W, state, workspace)
    with torch.cuda.device(state.device):
        _check(_lib.nmf_denoise_prepare(_p(state), _p(workspace), H, W, _stream()), "nmf_denoise_prepare")


def denoise_level(state, workspace, H, W, step, src, k_c, k_n, k_z, eps_z, k_a):
    """nmf_denoise_level: one a-trous level of step `step` from set `src` (0 / 1) of the workspace into the other"""
    H, W = int(H), int(W)
    _denoise_buffers("denoise_level", H, W, state, workspace)
    with torch.cuda.device(state.device):
        _check(_lib.nmf_denoise_level(_p(state), _p(workspace), H, W, int(step), int(src), float(k_c), float(k_n), float(k_z),
                                      float(eps_z), float(k_a), _stream()), "nmf_denoise_level")


def denoise_finish(workspace, H, W, src, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False, want=("rgb_map",), out=None):
    """nmf_denoise_finish: the maps named in `want` from set `src` -> dict(rgb_map [P, 3], rgb_lin [P, 3], acc [P], se [P] = sqrt(Vg));
    out: tensors to fill instead of new ones, by name"""
    H, W = int(H), int(W)
    _denoise_buffers("denoise_finish", H, W, None, workspace)
    res = _denoise_outputs("denoise_finish", H * W, want, out, workspace.device)
    with torch.cuda.device(workspace.device):
        _check(_lib.nmf_denoise_finish(_p(workspace), H, W, int(src), float(bg[0]), float(bg[1]), float(bg[2]), int(bool(tonemap)),
                                       int(bool(noclip)), *[_p(res.get(k), torch.float32) for k in DENOISE_OUTPUTS], _stream()),
               "nmf_denoise_finish")
    return res


def denoise(state, H, W, levels, k_c, k_n, k_z, eps_z, k_a, bg=(1.0, 1.0, 1.0), tonemap=True, noclip=False, want=("rgb_map",),
            workspace=None, out=None):
    """nmf_denoise: prepare, `levels` levels of steps 1, 2, 4, ... and finish on the current stream -> denoise_finish's dict.
    workspace: a device tensor of denoise_workspace_bytes to reuse (default: a new one)"""
    H, W = int(H), int(W)
    if workspace is None:
        workspace = torch.empty(denoise_workspace_bytes(H, W) // 4, dtype=torch.float32, device=state.device)
    _denoise_buffers("denoise", H, W, state, workspace)
    res = _denoise_outputs("denoise", H * W, want, out, workspace.device)
    with torch.cuda.device(state.device):
        _check(_lib.nmf_denoise(_p(state), _p(workspace), H, W, int(levels), float(k_c), float(k_n), float(k_z), float(eps_z), float(k_a),
                                float(bg[0]), float(bg[1]), float(bg[2]), int(bool(tonemap)), int(bool(noclip)),
                                *[_p(res.get(k), torch.float32) for k in DENOISE_OUTPUTS], _stream()), "nmf_denoise")
    return res
