"""Mesh export -- counterpart of the reference's scripts/export_mesh.py (dense alpha volume, then
utils.convert_sdf_samples_to_ply -> skimage.measure.marching_cubes on the host): the alpha lattice of the trained field is
triangulated on the GPU (hip.marching_cubes, csrc/mesh.hip) and every vertex can carry the field's normal and the material
heads' albedo / f0 / roughness, evaluated with the kernels the renderer uses.

    mesh = extract_mesh(nerf, resolution=512)
    write_ply("out.ply", mesh)

Placement.  getDenseAlpha samples the lattice aabb[0] + idx * (aabb[1] - aabb[0]) / (G - 1), and that is where the vertices are put
(idx = the marching-cubes position in lattice index units).  The reference writes bbox[0] + idx * size / G (utils.py:179-191:
voxel = size / G), which shrinks the mesh by (G - 1) / G towards aabb[0] against the scene it was sampled from;
reference_spacing=True reproduces that placement for comparison, the default is the aligned one.
"""
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
    mesh = Mesh(verts=verts, faces=faces, index_verts=idx, seconds=sec)
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
