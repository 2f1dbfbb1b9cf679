"""Scene composition: several trained objects rendered under one environment, so that they occlude, shadow and reflect each other.

The reference's version is scripts/toaster_on_car.py over fields/listrf.py: densities by max, every object's features through the
material heads and BRDF of one model, a second sampler.  Here every object (a TensorNeRF, "part") keeps its own sampler, field and
shading model and works in its own frame; the glue runs on the GPU (csrc/compose.hip): rays are placed into each part's frame
(hip.rays_place), the parts' compact per-ray sample lists are merged into one depth-ordered list (hip.merge_rank, hip.merge_scatter),
ONE Composite gives the weights of the merged list, every part shades its own samples with those weights, and ONE RayCompose sums
the merged list per ray.  DESIGN.md 10.10.

    car, toaster = TensorNeRF.load("car.th"), TensorNeRF.load("toaster.th")
    scene = ComposedScene([(car, Placement.identity()), (toaster, Placement.from_spec("t=0,0,0.9;r=40,0,0;s=0.4"))])
    rgb = render_images(scene, rays, focal)

Conventions.  A placement maps a part's frame to the world, x_w = s R x_l + c, with a uniform scale.  The local origin of a ray is
the image of its world origin and directions are only rotated, so a sample at local depth z lies at world depth s z.  Where parts
overlap their optical depths add (sigma dist does not depend on s): the union behaves as the SUM of the densities, which is what a
participating medium does and what makes the opacity law acc = 1 - prod_k (1 - acc_k) hold; the reference takes the max.  There is
one environment, in the world frame; part k shades in its own frame under L_k(d) = L_w(R_k d).  bg_module=None carries part 0's
own lighting along with part 0, L_w(d) = L_0(R_0^T d).  Evaluation only.
"""
import types

import numpy as np
import torch

from . import hip, relight
from .functional import Composite, RayCompose, segment_sum
from .noise import DeviceNoise

MAX_PARTS = hip.MERGE_MAX_LISTS
ROTATION_TOL = 1e-4                  # max|R^T R - I|: the bound of nmf_env_resample and nmf_rays_place
MATERIAL_KEYS = ("albedo", "roughness", "diffuse", "tint", "spec")


class Placement:
    """local -> world similarity x_w = s R x_l + c.  rotation: a 3x3 rotation matrix, or (yaw, pitch, roll) in degrees (+z up,
    relight.rotation); translation: c; scale: uniform, s > 0.  Kept in float64 on the host."""

    def __init__(self, rotation=None, translation=(0.0, 0.0, 0.0), scale=1.0):
        if rotation is None:
            R = np.eye(3)
        else:
            R = np.asarray(rotation.detach().cpu().numpy() if isinstance(rotation, torch.Tensor) else rotation, dtype=np.float64)
            if R.shape == (3,):
                R = relight.rotation(*[float(v) for v in R])
        if R.shape != (3, 3):
            raise ValueError(f"Placement: a rotation is a 3x3 matrix or (yaw, pitch, roll), got shape {R.shape}")
        if not (np.abs(R.T @ R - np.eye(3)).max() <= ROTATION_TOL) or not np.linalg.det(R) > 0:
            raise ValueError(f"Placement: R is not a rotation (max|R^T R - I| > {ROTATION_TOL:g}, or a reflection)")
        t = np.asarray(translation.detach().cpu().numpy() if isinstance(translation, torch.Tensor) else translation,
                       dtype=np.float64).reshape(-1)
        if t.shape != (3,) or not np.isfinite(t).all():
            raise ValueError("Placement: a translation is 3 finite numbers")
        s = float(scale)
        if not (np.isfinite(s) and s > 0):
            raise ValueError(f"Placement: the scale is uniform and positive, got {scale}")
        self.R, self.t, self.s = R, t, s

    @classmethod
    def identity(cls):
        return cls()

    @classmethod
    def from_spec(cls, text):
        """"t=1.2,0,0;r=40,0,0;s=0.7": translation, rotation (yaw, pitch, roll in degrees) and scale; any subset, in any order"""
        fields = {}
        for item in str(text).split(";"):
            item = item.strip()
            if not item:
                continue
            name, eq, val = item.partition("=")
            name = name.strip()
            if name not in ("t", "r", "s") or not eq:
                raise ValueError(f"placement '{text}': unknown field '{item}' (t=x,y,z  r=yaw,pitch,roll  s=scale)")
            if name in fields:
                raise ValueError(f"placement '{text}': field '{name}' is given twice")
            try:
                nums = [float(v) for v in val.split(",")]
            except ValueError:
                raise ValueError(f"placement '{text}': field '{name}' holds '{val}', not numbers") from None
            want = 1 if name == "s" else 3
            if len(nums) != want or not np.isfinite(nums).all():
                raise ValueError(f"placement '{text}': field '{name}' takes {want} finite number{'s' if want > 1 else ''}, got '{val}'")
            fields[name] = nums
        try:
            return cls(fields.get("r"), fields.get("t", (0.0, 0.0, 0.0)), fields.get("s", [1.0])[0])
        except ValueError as e:
            raise ValueError(f"placement '{text}': field 's': {e}") from None

    def inverse(self):
        Rt = self.R.T
        return Placement(Rt, -(Rt @ self.t) / self.s, 1.0 / self.s)

    def __matmul__(self, other):
        """(P @ Q)(x) = P(Q(x))"""
        return Placement(self.R @ other.R, self.s * (self.R @ other.t) + self.t, self.s * other.s)

    def apply(self, x):
        """points [..., 3] (numpy, float64) local -> world"""
        return self.s * (np.asarray(x, dtype=np.float64) @ self.R.T) + self.t

    def is_identity(self):
        return bool(np.array_equal(self.R, np.eye(3)) and not self.t.any() and self.s == 1.0)

    def spec(self):
        """what the command line's JSON line reports"""
        return dict(rotation=[[round(float(v), 9) for v in row] for row in self.R], translation=[float(v) for v in self.t],
                    scale=self.s)

    def __repr__(self):
        return f"Placement(R={self.R.tolist()}, t={self.t.tolist()}, s={self.s})"


def _same_rotation(R):
    return bool(np.abs(R - np.eye(3)).max() <= 1e-12)


class _Images(dict):
    """images of a composed scene: the material maps are not built for compositions and say so when asked for"""

    def _refuse(self, key):
        if key in MATERIAL_KEYS:
            raise NotImplementedError(f"'{key}': material maps of a composed scene are not built (DESIGN.md 10.10)")

    def __contains__(self, key):
        self._refuse(key)
        return dict.__contains__(self, key)

    def __missing__(self, key):
        self._refuse(key)
        raise KeyError(key)


class ComposedScene(torch.nn.Module):
    """parts: [(TensorNeRF, Placement)], 1..8; bg_module: the world environment (None: part 0's own lighting carried along with part
    0); near_far: (near, far) in world units for every part, None: every part is marched over the range its AABB limits, at any
    distance from the camera.  Callable like TensorNeRF (evaluation only); renderer.render_images and evaluation_path drive it
    through their module path.  cross_reflections = False re-traces a part's bounce rays through that part alone (debugging)."""

    fused_eval_pass = False             # renderer.render_images: always the module path (no C++ pass for compositions)

    def __init__(self, parts, bg_module=None, near_far=None):
        super().__init__()
        parts = [(n, p if isinstance(p, Placement) else Placement.from_spec(p)) for n, p in parts]
        if not 1 <= len(parts) <= MAX_PARTS:
            raise ValueError(f"a composed scene has 1..{MAX_PARTS} parts, got {len(parts)}")
        from .fast_step import TrainPass
        for k, (nerf, _) in enumerate(parts):
            if not TrainPass.supported(types.SimpleNamespace(nerf=nerf)):
                raise NotImplementedError(f"part {k}: a composed scene renders models the fused pass supports (one re-trace level, a "
                                          "bg_module, a fused BRDF)")
            if nerf._material_edit_table is not None:
                raise ValueError(f"part {k} has material edits set: edits of a composition are not built (set_material_edits(None))")
        if near_far is not None:
            near_far = (float(near_far[0]), float(near_far[1]))
            if not 0 <= near_far[0] < near_far[1]:
                raise ValueError(f"near_far = {near_far}: 0 <= near < far, in world units")
        object.__setattr__(self, "parts", parts)           # (the parts stay their owners': not registered as submodules)
        self.near_far = near_far
        self.cross_reflections = True
        self._noise = None
        self._world = None                  # the world map given by the caller; None: part 0's own lighting
        self._default_world = None          # what `bg_module` hands out for part 0's lighting when R_0 != I (built on first read)
        self._local = None                  # per part: the module it shades under
        self._env_key = None
        self._march_caches = [dict() for _ in parts]
        if bg_module is not None:
            self.bg_module = bg_module

    # ---- environment -------------------------------------------------------------------------------------------------------------
    def __setattr__(self, name, value):
        if name == "bg_module":
            d = self.__dict__
            d["_world"] = None if (value is None or value is d.get("_default_world") or self._is_own_lighting(value)) else value
            d["_local"] = None
        else:
            super().__setattr__(name, value)

    def _is_own_lighting(self, module):
        nerf0, P0 = self.parts[0]
        return module is nerf0.bg_module and _same_rotation(P0.R)

    @property
    def bg_module(self):
        """the world environment.  Assigning a module replaces it (the parts' local maps are rebuilt on the next render); None, or
        the module read here before, brings part 0's own lighting back"""
        d = self.__dict__
        if d["_world"] is not None:
            return d["_world"]
        nerf0, P0 = self.parts[0]
        if _same_rotation(P0.R):
            return nerf0.bg_module
        if d["_default_world"] is None:
            d["_default_world"] = relight.rotate_env(nerf0.bg_module, P0.R)
        return d["_default_world"]

    def _environment(self):
        """-> per part the module it shades under, L_k(d) = L_w(R_k d): resampled by relight.rotate_env, or the module that already
        holds it (no resampling).  Rebuilt when the world map was replaced or rewritten in place (a light turntable)."""
        d = self.__dict__
        world = d["_world"]
        src = world if world is not None else self.parts[0][0].bg_module
        key = (id(src), src.bg_mat._version, src.brightness._version, src.mul._version)
        if d["_local"] is not None and d["_env_key"] == key:
            return d["_local"]
        R_src = np.eye(3) if world is not None else self.parts[0][1].R          # the frame `src` is expressed in
        old = d["_local"] if d["_env_key"] is not None and d["_env_key"][0] == key[0] else None
        local = []
        for k, (_, P) in enumerate(self.parts):
            Rrel = P.R.T @ R_src                                                # L_k(d) = src(R_src^T R_k d) = src(Rrel^T d)
            if _same_rotation(Rrel):
                local.append(src)
            else:
                out = old[k] if (old is not None and old[k] is not src) else None
                local.append(relight.rotate_env(src, Rrel, out=out))
        d["_local"], d["_env_key"] = local, key
        return local

    def local_env(self, k):
        """the module part k shades under"""
        return self._environment()[k]

    # ---- geometry ----------------------------------------------------------------------------------------------------------------
    @property
    def eval_batch_size(self):
        return min(n.eval_batch_size for n, _ in self.parts)

    def get_device(self):
        return self.parts[0][0].get_device()

    def world_aabb(self):
        """[2, 3] float64: the box around the parts' AABBs in the world"""
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for nerf, P in self.parts:
            a = hip.host(nerf.rf.aabb).astype(np.float64).reshape(2, 3)
            corners = np.array([[a[i][0], a[j][1], a[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
            w = P.apply(corners)
            lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
        return np.stack([lo, hi])

    def _sampler(self, k):
        """part k's sampler with this scene's marching range: a shallow view, the part's own sampler is not touched"""
        import copy
        nerf, P = self.parts[k]
        view = copy.copy(nerf.sampler)
        d = view.__dict__
        # near just above 0 and far beyond anything: the marcher clamps a ray's start to its entry into the AABB and walks nSamples
        # steps from there, so the part renders at any distance from the camera
        d["near_far"] = [1e-6, 1e30] if self.near_far is None else [self.near_far[0] / P.s, self.near_far[1] / P.s]
        d["_params_cache"] = self._march_caches[k]
        return view

    # ---- rendering ---------------------------------------------------------------------------------------------------------------
    def forward(self, rays, focal, start_mipval=None, bg_col=torch.tensor([1, 1, 1]), recur=0, override_near=None, is_train=False,
                tonemap=True, draw_debug=False, noise=None, **kw):
        if is_train:
            raise ValueError("a composed scene is evaluation only (is_train=True)")
        for k, (nerf, _) in enumerate(self.parts):
            if nerf._material_edit_table is not None:
                raise ValueError(f"part {k} has material edits set: edits of a composition are not built")
        if noise is None:
            if self._noise is None:
                self._noise = DeviceNoise(rays.device, seed=20211200)
            noise = self._noise
        with torch.no_grad():
            if recur > 0:
                return self._render(rays, focal, start_mipval, bg_col, recur, override_near, tonemap, draw_debug, noise)
            mods = []
            for m in [m for nerf, _ in self.parts for m in (nerf.rf, nerf.model.brdf, nerf.model.diffuse_module)] + self._environment():
                if hasattr(m, "begin_pass") and not any(m is o for o in mods):
                    mods.append(m)
            for m in mods:
                m.begin_pass()
            try:
                if hasattr(noise, "begin_pass"):
                    noise.begin_pass()
                return self._render(rays, focal, start_mipval, bg_col, recur, override_near, tonemap, draw_debug, noise)
            finally:
                for m in mods:
                    m.end_pass()

    def _render(self, rays, focal, start_mipval, bg_col, recur, override_near, tonemap, draw_debug, noise, only=None, local_rays=None):
        """one level.  rays: WORLD rays [B, 6].  only: the one part that takes part (cross_reflections = False); local_rays: {part:
        rays already in that part's frame} -- the bounce rays of a part are born there, and taking them as they are instead of
        through world and back keeps a single-part scene bit-identical to the part rendered alone."""
        dev = rays.device
        rays = rays.contiguous()
        B = rays.shape[0]
        env = self._environment()
        active = list(range(len(self.parts))) if only is None else [only]
        ds0 = float(self.parts[0][0].rf.distance_scale)
        local, Ss, sigmas, normals = {}, {}, {}, {}
        for k in active:
            nerf, P = self.parts[k]
            local[k] = local_rays[k] if (local_rays is not None and k in local_rays) else hip.rays_place(rays, P, inverse=True)
            S = self._sampler(k).sample_compact(local[k], focal, override_near=None if override_near is None else override_near / P.s,
                                                is_train=False, dynamic_batch_size=False, noise=noise)
            if S.b != B:
                raise RuntimeError(f"part {k}: the sampler kept {S.b} of {B} rays (an evaluation pass has no sample budget)")
            sigmas[k], _sf, _app, normals[k] = nerf.rf.query(S.xyzt, want_app=False, want_normal=True)
            Ss[k] = S
        # ---- one depth-ordered list per ray
        dst, offsets_m = hip.merge_rank([Ss[k].offsets[: B + 1] for k in active], [Ss[k].z for k in active],
                                        [self.parts[k][1].s for k in active], B)
        dst = dict(zip(active, dst))
        M = sum(Ss[k].M for k in active)
        f = dict(dtype=torch.float32, device=dev)
        merged = dict(sigma=torch.zeros(M, **f), dist=torch.zeros(M, **f), z=torch.zeros(M, **f), normal=torch.zeros((M, 3), **f),
                      ray_id=torch.zeros(M, dtype=torch.int32, device=dev), part=torch.zeros(M, dtype=torch.int32, device=dev),
                      src=torch.zeros(M, dtype=torch.int32, device=dev))
        for k in active:
            nerf, P = self.parts[k]
            S = Ss[k]
            if S.M > 0:
                hip.merge_scatter(dst[k], M, part=k, sigma=sigmas[k].contiguous(), dist=S.dist, z=S.z, normal=normals[k].contiguous(),
                                  ray_id=S.ray_id, sigma_ratio=float(nerf.rf.distance_scale) / ds0, scale=P.s, R=P.R, out=merged)
        weight = Composite.apply(merged["sigma"], merged["dist"], offsets_m, B, ds0)
        n_samples = [M]

        # ---- every part shades its own samples with the merged list's weights
        rows, inv_m, row_base = [], torch.full((M,), -1, dtype=torch.int32, device=dev), 0
        for k in active:
            nerf, P = self.parts[k]
            S = Ss[k]
            if S.M == 0:
                continue
            shaded = nerf.model.shade_compact(S, None, normals[k], torch.index_select(weight, 0, dst[k]),
                                              self._reflection(k, focal, recur, noise, n_samples), env[k], False, recur, noise,
                                              app_fn=nerf.rf.compute_appfeature)
            refl = shaded.refl_rows
            if refl is not None:
                hip.merge_scatter(dst[k], M, part=k, inv=shaded.inv, row_base=row_base, out=dict(inv=inv_m))
                rows.append(refl)
                row_base += refl.shape[0]

        # ---- background: the world environment per ray, or the caller's colour (TensorNeRF._render)
        per_ray_bg = bg_col is None
        if per_ray_bg:
            rough = -100 * torch.ones(B, device=dev) if start_mipval is None else start_mipval[:B]
            noise.skip("rand", (B,))
            noise.skip("rand", (B,))
            bg = self._world_lookup(rays, local, rough)
            if tonemap:
                bg = self.parts[0][0].tonemap(bg, noclip=True)
        else:
            bg = bg_col.to(device=dev, dtype=torch.float32).reshape(1, 3)

        lin = [] if recur == 0 else None
        refl = torch.cat(rows, 0) if rows else None
        rgb_map, acc_map, _ori = RayCompose.apply(weight, refl, merged["normal"] if M > 0 else None, bg, inv_m if refl is not None else None,
                                                  offsets_m, merged["ray_id"], rays, B, per_ray_bg, bool(tonemap), False, False,
                                                  *(() if lin is None else (lin,)))
        images = _Images(rgb_map=rgb_map, acc_map=acc_map.detach())
        if lin:
            images["rgb_lin"] = lin[0]
        if recur == 0:
            # (formed with or without draw_debug -- two segment sums: render_images' module path asks for the depth and normal
            #  panels of a camera path without it)
            images["depth"] = segment_sum(weight * merged["z"], offsets_m, merged["ray_id"], B)
            wn = segment_sum(merged["normal"] * weight[:, None], offsets_m, merged["ray_id"], B)
            images["world_normal"] = acc_map[..., None] * wn + (1 - acc_map[..., None])
            images["surf_width"] = offsets_m[1:] - offsets_m[:-1]
        stats = dict(recur=recur, whole_valid=torch.ones(B, dtype=torch.bool, device=dev), n_samples=n_samples, rays_kept=B)
        return images, stats

    def _world_lookup(self, rays, local, rough):
        """L_w along the world rays.  Part 0's own lighting is looked up in part 0's module along part 0's local directions,
        L_w(d) = L_0(R_0^T d): no resampled copy of the map is involved"""
        world = self.__dict__["_world"]
        if world is not None:
            return world(rays, rough).reshape(-1, 3)
        if rays.shape[0] == 0:
            return torch.empty((0, 3), device=rays.device)
        nerf0, P0 = self.parts[0]
        lr = local[0] if 0 in local else hip.rays_place(rays, P0, inverse=True)
        return nerf0.bg_module(lr, rough).reshape(-1, 3)

    def _reflection(self, k, focal, recur, noise, n_samples):
        """the render_reflection callback of part k's shading (TensorNeRF._render): its bounce rays, local, go into the world and
        through the whole scene again, or to part k's local environment"""
        nerf, P = self.parts[k]
        env_k = self._environment()[k]

        def render_reflection(brays, mipval, retrace):
            if retrace:
                brays = brays.contiguous()
                wrays = hip.rays_place(brays, P, inverse=False)
                ims, st = self._render(wrays, focal, mipval.reshape(-1), None, recur + 1,
                                       3 * P.s * float(hip.host(nerf.sampler.stepsize)), False, False, noise,
                                       only=None if self.cross_reflections else k, local_rays={k: brays})
                n_samples.extend(st["n_samples"])
                return ims["rgb_map"]
            noise.skip("rand", (brays.shape[0],))
            noise.skip("rand", (brays.shape[0],))
            if brays.shape[0] == 0:
                return torch.empty((0, 3), device=brays.device)
            return env_k(brays, mipval.reshape(-1)).reshape(-1, 3)

        return render_reflection
