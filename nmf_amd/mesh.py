"""Mesh export -- counterpart of the reference's scripts/export_mesh.py (dense alpha volume, then
utils.convert_sdf_samples_to_ply -> skimage.measure.marching_cubes on the host): the alpha lattice of the trained field is
triangulated on the GPU (hip.marching_cubes, csrc/mesh.hip) and every vertex can carry the field's normal and the material
heads' albedo / f0 / roughness, evaluated with the kernels the renderer uses.

    mesh = extract_mesh(nerf, resolution=512)
    write_ply("out.ply", mesh)
    write_obj("out.obj", mesh, bake_textures(nerf, mesh, size=4096))      # the same quantities per texel of a per-triangle atlas

Placement.  getDenseAlpha samples the lattice aabb[0] + idx * (aabb[1] - aabb[0]) / (G - 1), and that is where the vertices are put
(idx = the marching-cubes position in lattice index units).  The reference writes bbox[0] + idx * size / G (utils.py:179-191:
voxel = size / G), which shrinks the mesh by (G - 1) / G towards aabb[0] against the scene it was sampled from;
reference_spacing=True reproduces that placement for comparison, the default is the aligned one.
"""
import math
import os
import time
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import hip
from .modules.tonemap import SRGBTonemap

ATTRIBUTE_CHUNK = 1 << 20          # vertices per attribute query (nerf.eval_batch_size counts rays and is far too small here)


@dataclass
class Mesh:
    """verts fp32 [V,3] world positions, faces int32 [F,3] (normals point from inside to outside); with attributes per vertex:
    normals [V,3] (the field's shading normal), albedo [V,3], f0 [V,3], roughness [V].  index_verts: the positions in lattice
    index units as marching cubes wrote them; seconds: wall time per stage (density, triangulate, attributes)."""
    verts: torch.Tensor
    faces: torch.Tensor
    normals: Optional[torch.Tensor] = None
    albedo: Optional[torch.Tensor] = None
    f0: Optional[torch.Tensor] = None
    roughness: Optional[torch.Tensor] = None
    index_verts: Optional[torch.Tensor] = None
    seconds: dict = field(default_factory=dict)
    aligned_verts: Optional[torch.Tensor] = None          # where the attributes belong when verts are placed elsewhere (reference_spacing)

    @property
    def has_attributes(self):
        return self.normals is not None


def _resolution(rf, resolution):
    if resolution is None:
        return [int(g) for g in hip.host(rf.grid_size)]
    if isinstance(resolution, int):
        return [resolution] * 3
    gs = [int(g) for g in resolution]
    if len(gs) != 3:
        raise ValueError(f"resolution: None, an int or three ints, got {resolution}")
    return gs


@torch.no_grad()
def vertex_attributes(nerf, xyz):
    """normals [V,3], albedo [V,3], f0 [V,3], roughness [V] at world points xyz [V,3]: rf.compute_normals (the normal the renderer
    shades with) and the material heads over rf.compute_appfeature, with the clips of nmf_material_maps (albedo in [0, 1],
    roughness = clip(sigmoid / 2, 0.01, 1), both applied by nmf_heads_fwd), ATTRIBUTE_CHUNK points at a time."""
    outs = ([], [], [], [])
    for s in range(0, xyz.shape[0], ATTRIBUTE_CHUNK):
        p = xyz[s:s + ATTRIBUTE_CHUNK].contiguous()
        heads = nerf.model.diffuse_module.heads(nerf.rf.compute_appfeature(p))
        table = getattr(nerf, "_material_edit_table", None)
        if table is not None:                  # nerf.set_material_edits: the attributes of the edited materials
            heads = hip.heads_edit(heads.detach().contiguous(), p, table)
        for o, v in zip(outs, (nerf.rf.compute_normals(p), heads[:, 0:3], heads[:, 6:9], heads[:, 9])):
            o.append(v.detach())
    if not outs[0]:
        z = xyz.new_zeros
        return z((0, 3)), z((0, 3)), z((0, 3)), z((0,))
    return tuple(torch.cat(o).contiguous() for o in outs)


@torch.no_grad()
def extract_mesh(nerf, resolution=None, level=0.005, attributes=True, reference_spacing=False):
    """The iso-surface alpha == level of nerf's field as a Mesh.  resolution: None (rf.grid_size), an int or three ints; the volume
    is nerf.sampler.getDenseAlpha(rf, resolution), unchanged.  Vertices are placed where getDenseAlpha sampled:
    aabb[0] + idx * (aabb[1] - aabb[0]) / (G - 1).  reference_spacing=True places them as the reference does instead,
    aabb[0] + idx * (aabb[1] - aabb[0]) / G, a mesh shrunk by (G - 1) / G (module docstring); attributes are then evaluated at the
    aligned positions all the same (they belong to the surface, not to the shifted copy)."""
    rf = nerf.rf
    gs = _resolution(rf, resolution)
    dev = rf.get_device()
    sec = {}

    def lap(name, t0):
        torch.cuda.synchronize(dev)
        sec[name] = time.perf_counter() - t0
        return time.perf_counter()

    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    alpha = nerf.sampler.getDenseAlpha(rf, gs)
    t = lap("density", t)
    idx, faces = hip.marching_cubes(alpha, level)
    del alpha
    t = lap("triangulate", t)
    aabb = nerf.sampler.aabb.to(dev).float()
    G = torch.tensor(gs, dtype=torch.float32, device=dev)
    aligned = aabb[0] + idx * ((aabb[1] - aabb[0]) / (G - 1))
    verts = aabb[0] + idx * ((aabb[1] - aabb[0]) / G) if reference_spacing else aligned
    mesh = Mesh(verts=verts, faces=faces, index_verts=idx, seconds=sec, aligned_verts=aligned if reference_spacing else None)
    if attributes:
        mesh.normals, mesh.albedo, mesh.f0, mesh.roughness = vertex_attributes(nerf, aligned)
        lap("attributes", t)
    return mesh


PLY_POSITION = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
PLY_ATTRIBUTES = [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                  ("roughness", "<f4"), ("f0_r", "<f4"), ("f0_g", "<f4"), ("f0_b", "<f4")]
PLY_FACE = [("n", "u1"), ("vertex_indices", "<i4", (3,))]


def ply_header(n_verts, n_faces, attributes):
    props = PLY_POSITION + (PLY_ATTRIBUTES if attributes else [])
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_verts}"]
    lines += [f"property {'uchar' if t == 'u1' else 'float'} {name}" for name, t in props]
    lines += [f"element face {n_faces}", "property list uchar int vertex_indices", "end_header"]
    return "\n".join(lines) + "\n"


def albedo_to_8bit(albedo):
    """albedo through the sRGB tonemap, floor(clip * 255) as the PNG writers quantise -> uint8 numpy [V,3]"""
    srgb = SRGBTonemap()(albedo.float())
    return torch.floor(srgb.clip(0, 1) * 255).to(torch.uint8).cpu().numpy()


def write_ply(path, mesh):
    """Binary little-endian PLY.  Vertex: x y z float; with attributes also nx ny nz float, red green blue uchar (albedo through the
    sRGB tonemap, floor(clip * 255)), roughness f0_r f0_g f0_b float.  Face: a uchar count and three int indices.  Without
    attributes the header is the one of the reference's files (positions and faces only)."""
    V, F = int(mesh.verts.shape[0]), int(mesh.faces.shape[0])
    attrs = mesh.has_attributes
    vert = np.zeros(V, dtype=PLY_POSITION + (PLY_ATTRIBUTES if attrs else []))
    pos = mesh.verts.detach().float().cpu().numpy()
    for i, k in enumerate("xyz"):
        vert[k] = pos[:, i]
    if attrs:
        nrm, f0 = mesh.normals.detach().float().cpu().numpy(), mesh.f0.detach().float().cpu().numpy()
        rgb = albedo_to_8bit(mesh.albedo.detach())
        for i, (kn, kc, kf) in enumerate(zip(("nx", "ny", "nz"), ("red", "green", "blue"), ("f0_r", "f0_g", "f0_b"))):
            vert[kn], vert[kc], vert[kf] = nrm[:, i], rgb[:, i], f0[:, i]
        vert["roughness"] = mesh.roughness.detach().float().cpu().numpy().reshape(-1)
    face = np.zeros(F, dtype=PLY_FACE)
    face["n"] = 3
    face["vertex_indices"] = mesh.faces.detach().cpu().numpy().astype("<i4")
    with open(path, "wb") as f:
        f.write(ply_header(V, F, attrs).encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())


# ---- texture atlas: one chart per triangle, materials and normals baked per texel (csrc/atlas.hip) -----------------
ATLAS_MIN, ATLAS_MAX, ATLAS_T_MIN = 4, 16384, 4


def atlas_layout(F, size):
    """The atlas of F faces in a size x size texture -> (W, T, n, b): W = size texels per side, squares of T x T texels, n = W // T of
    them per row, b = T - 3 texel steps along a chart's two legs.  Texel t = y W + x, row y = 0 on top.  Square s = cy n + cx holds
    face 2 s in its lower half (local texels i + j <= T - 2, corners 0, 1, 2 at (0, 0), (b, 0), (0, b)) and face 2 s + 1 in its upper
    half (the same under i' = T - 1 - i, j' = T - 1 - j).  T is the largest integer with (W // T)^2 >= ceil(F / 2); below 4 a bilinear
    fetch inside a chart would reach a neighbour's texels, so such an atlas is refused.  This is the one definition of the layout:
    the kernels (include/nmf_hip.h) take W and T from here."""
    F, W = int(F), int(size)
    if F < 0:
        raise ValueError(f"atlas_layout: F = {F} is negative")
    if not ATLAS_MIN <= W <= ATLAS_MAX:
        raise ValueError(f"atlas_layout: texture size {W} is outside {ATLAS_MIN}..{ATLAS_MAX}")
    m = math.isqrt((F + 1) // 2)
    m += m * m < (F + 1) // 2                        # squares per row that hold the faces: ceil(sqrt(ceil(F / 2)))
    T = W // m if m else W                           # W // T >= m  <=>  T <= W / m
    if T < ATLAS_T_MIN:
        raise ValueError(f"atlas_layout: {F} faces in a {W} x {W} texture leave {T} x {T} texels per triangle pair, below "
                         f"{ATLAS_T_MIN}; the smallest --texture-size that fits is {ATLAS_T_MIN * m} (a lower --resolution fits as well)")
    return W, T, W // T, T - 3


def atlas_corner_texels(F, layout):
    """int64 numpy [F, 3, 2]: the texel (X, Y) of the atlas that carries corner k of face f"""
    W, T, n, b = layout
    f = np.arange(int(F), dtype=np.int64)
    s, upper = f // 2, (f % 2).astype(bool)
    local = np.array([[0, 0], [b, 0], [0, b]], dtype=np.int64)[None]                        # [1, 3, 2] (i, j)
    local = np.where(upper[:, None, None], T - 1 - local, local)
    return np.stack([s % n, s // n], -1)[:, None, :] * T + local


def atlas_uv(F, layout):
    """float32 numpy [F, 3, 2]: (u, v) of corner k of face f, the centre of its texel: u = (X + 0.5) / W, v = 1 - (Y + 0.5) / W
    (OBJ's v grows upwards, the atlas's rows downwards)"""
    W = layout[0]
    xy = atlas_corner_texels(F, layout).astype(np.float64)
    return np.stack([(xy[..., 0] + 0.5) / W, 1.0 - (xy[..., 1] + 0.5) / W], -1).astype(np.float32)


@dataclass
class Textures:
    """The baked atlas: albedo (sRGB), f0, normal (world space, 127 n + 128) uint8 [W, W, 3] and roughness uint8 [W, W], row 0 on top;
    uv float32 numpy [F, 3, 2] per face corner; layout (W, T, n, b) of atlas_layout; seconds: bake (wall) and its stages texels /
    queries / store (device time)."""
    albedo: torch.Tensor
    f0: torch.Tensor
    normal: torch.Tensor
    roughness: torch.Tensor
    uv: np.ndarray
    layout: tuple
    seconds: dict = field(default_factory=dict)


@torch.no_grad()
def bake_textures(nerf, mesh, size=4096, chunk=ATTRIBUTE_CHUNK):
    """Albedo, f0, roughness and the field's world-space normal at every owned texel of the size x size atlas of mesh (atlas_layout),
    `chunk` texels at a time: hip.atlas_texels (where each texel lies on its triangle, at the aligned positions -- where
    getDenseAlpha sampled -- also for a reference_spacing mesh), vertex_attributes over the owned ones (the renderer's kernels,
    nerf.set_material_edits included; an unowned texel costs no query), hip.atlas_store (8-bit planes).  The result does not
    depend on chunk."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"bake_textures: chunk = {chunk}")
    verts = (mesh.verts if mesh.aligned_verts is None else mesh.aligned_verts).detach().float().contiguous()
    faces = mesh.faces.detach().contiguous()
    layout = atlas_layout(faces.shape[0], size)
    W, T = layout[0], layout[1]
    dev = verts.device
    torch.cuda.synchronize(dev)
    wall = time.perf_counter()
    planes = [torch.empty((W, W, c) if c > 1 else (W, W), dtype=torch.uint8, device=dev) for c in (3, 3, 1, 3)]
    marks = []
    for t0 in range(0, W * W, chunk):
        n = min(chunk, W * W - t0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        pos, face_of = hip.atlas_texels(verts, faces, W, T, t0, n, check_faces=t0 == 0)
        ev[1].record()
        owned = torch.nonzero(face_of >= 0).squeeze(1)
        if owned.numel() == n:
            nrm, alb, f0, rgh = vertex_attributes(nerf, pos)
        else:                                        # the attributes of the owned texels, spread over the chunk's rows
            nrm, alb, f0, rgh = (v.new_zeros((n,) + tuple(v.shape[1:])).index_copy_(0, owned, v)
                                 for v in vertex_attributes(nerf, pos.index_select(0, owned)))
        ev[2].record()
        hip.atlas_store(face_of, alb, f0, rgh, nrm, t0, W, planes[0], planes[1], planes[2], planes[3])
        ev[3].record()
        marks.append(ev)
    torch.cuda.synchronize(dev)
    sec = dict(bake=time.perf_counter() - wall)
    for k, name in enumerate(("texels", "queries", "store")):
        sec[name] = sum(ev[k].elapsed_time(ev[k + 1]) for ev in marks) * 1e-3
    return Textures(albedo=planes[0], f0=planes[1], roughness=planes[2], normal=planes[3], uv=atlas_uv(faces.shape[0], layout),
                    layout=layout, seconds=sec)


TEXTURE_MAPS = (("albedo", "map_Kd"), ("f0", "map_Ks"), ("roughness", "map_Pr"), ("normal", "norm"))


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def obj_paths(path):
    """the six files of write_obj(path): obj, mtl and the four PNGs next to them, by map name"""
    path = str(path)
    root = path[:-4] if path.lower().endswith(".obj") else path
    return dict(obj=root + ".obj", mtl=root + ".mtl", **{m: f"{root}_{m}.png" for m, _ in TEXTURE_MAPS})


def write_obj(path, mesh, textures):
    """Wavefront OBJ + MTL + four PNGs: name.obj, name.mtl, name_albedo.png, name_f0.png, name_roughness.png (one channel),
    name_normal.png.  OBJ: v from mesh.verts, vn from mesh.normals (when the mesh has them), one vt per face corner (3 F of them, from
    textures.uv) and f v/vt/vn (v/vt without normals) with 1-based indices.  -> the paths (obj_paths)."""
    from .renderer import _png
    paths = obj_paths(path)
    name = os.path.basename(paths["obj"])[:-4]
    verts = _host(mesh.verts).astype(np.float32)
    faces = _host(mesh.faces).astype(np.int64)
    F = faces.shape[0]
    uv = np.asarray(textures.uv, dtype=np.float32).reshape(-1, 2)
    if uv.shape[0] != 3 * F:
        raise ValueError(f"write_obj: {uv.shape[0]} texture coordinates for {F} faces (3 per face)")
    normals = None if mesh.normals is None else _host(mesh.normals).astype(np.float32)
    for m, _ in TEXTURE_MAPS:
        _png(paths[m], _host(getattr(textures, m)).astype(np.uint8))
    W, T = textures.layout[0], textures.layout[1]
    with open(paths["mtl"], "w") as f:
        f.write(f"# {name}: materials of a per-triangle texture atlas, {W} x {W} texels, {T} x {T} per triangle pair\n"
                "# map_Kd (albedo) is sRGB; map_Ks (f0), map_Pr (roughness) and norm are linear data\n"
                "# norm is a WORLD-SPACE normal map (n = (rgb - 128) / 127), not a tangent-space one\n"
                "# charts are per triangle: sample with bilinear filtering and WITHOUT mip-maps (a coarser level mixes neighbouring charts)\n"
                "# the scalars are 1 so that a loader which multiplies a map by its scalar leaves the map as it is\n"
                "newmtl baked\nKa 0 0 0\nKd 1 1 1\nKs 1 1 1\nPr 1\nillum 2\n")
        for m, key in TEXTURE_MAPS:
            f.write(f"{key} {os.path.basename(paths[m])}\n")
    fi = faces + 1
    ti = np.arange(1, 3 * F + 1, dtype=np.int64).reshape(F, 3)
    if normals is None:
        idx, fmt = np.stack([fi, ti], -1).reshape(F, 6), "f %d/%d %d/%d %d/%d"
    else:
        idx, fmt = np.stack([fi, ti, fi], -1).reshape(F, 9), "f %d/%d/%d %d/%d/%d %d/%d/%d"
    with open(paths["obj"], "w") as f:
        f.write(f"# {verts.shape[0]} vertices, {F} faces; materials and world-space normals in the textures of {name}.mtl\n"
                f"mtllib {name}.mtl\n")
        np.savetxt(f, verts, fmt="v %.9g %.9g %.9g")
        if normals is not None:
            np.savetxt(f, normals, fmt="vn %.9g %.9g %.9g")
        np.savetxt(f, uv, fmt="vt %.9g %.9g")
        f.write("usemtl baked\n")
        np.savetxt(f, idx, fmt=fmt)
    return paths
