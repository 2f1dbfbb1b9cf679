"""Writes mesh_mc.npz: skimage.measure.marching_cubes (0.18.3, the routine the reference's utils.convert_sdf_samples_to_ply calls,
utils.py:181) on three 48^3 fp32 alpha volumes at level 0.005.  Needs an interpreter with scikit-image; nothing else does:
    python3.9 tests/golden/make_mesh_golden.py

Volumes: alpha = 1 - exp(-0.75 * softplus(s - 4)) on the lattice linspace(-1.5, 1.5, 48)^3, computed in float64, stored as fp32
  box      s = 40 inside the cube |x|, |y|, |z| <= 0.75, -15 outside (the S1 shape of nmf_amd/synthetic.py)
  sphere   s = 60 * (0.8 - |p|)
  torus    s = 60 * (0.25 - distance to the circle of radius 0.8 in the z = 0 plane)
Keys per volume <name>: <name>_vol [48,48,48] fp32; <name>_verts [V,3] fp32 (index units, default spacing, method 'lewiner', the
reference's default); <name>_stats float64 [8] = (V, F, Euler characteristic V - E + F, boundary edges, non-manifold edges,
connected components, signed volume, area), the last two after the reference's faces[..., ::-1] flip (utils.py:184);
<name>_lorensen float64 [4] = (V, F, signed volume, area) of method 'lorensen'.  names: the three names; level.
The script asserts what makes these volumes a fixture for ANY consistent table: both methods give the same vertex set and the
same F, no boundary and no non-manifold edges (no ambiguous cases are met).
"""
import os

import numpy as np
from skimage.measure import marching_cubes

HERE = os.path.dirname(os.path.abspath(__file__))
G, LEVEL = 48, 0.005


def alpha(s):
    sp = np.logaddexp(0.0, s - 4.0)                                              # softplus
    return (1.0 - np.exp(-0.75 * sp)).astype(np.float32)


def volumes():
    lin = np.linspace(-1.5, 1.5, G)
    x, y, z = np.meshgrid(lin, lin, lin, indexing="ij")
    box = np.where(np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z)) <= 0.75, 40.0, -15.0)
    sphere = 60.0 * (0.8 - np.sqrt(x * x + y * y + z * z))
    torus = 60.0 * (0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.8) ** 2 + z * z))
    return dict(box=alpha(box), sphere=alpha(sphere), torus=alpha(torus))


def mesh_stats(verts, faces):
    """(Euler characteristic, boundary edges, non-manifold edges, components, signed volume, area) in float64"""
    V, F = len(verts), len(faces)
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    parent = np.arange(V)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in uniq:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    comps = len({find(a) for a in range(V)})
    p = verts.astype(np.float64)[faces]
    vol = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum()
    return V - len(uniq) + F, int((cnt == 1).sum()), int((cnt > 2).sum()), comps, vol, area


def main():
    out = dict(names=np.array(["box", "sphere", "torus"]), level=np.float64(LEVEL))
    for name, vol in volumes().items():
        res = {}
        for method in ("lewiner", "lorensen"):
            verts, faces, _, _ = marching_cubes(vol, level=LEVEL, method=method)
            faces = faces[..., ::-1]                                             # utils.py:184
            res[method] = (verts.astype(np.float32), faces, mesh_stats(verts, faces))
        (v0, f0, s0), (v1, f1, s1) = res["lewiner"], res["lorensen"]
        order = lambda v: v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]             # noqa: E731
        assert v0.shape == v1.shape and np.array_equal(order(v0), order(v1)) and len(f0) == len(f1), name
        assert s0[1] == s0[2] == 0 and s1[1] == s1[2] == 0 and s0[:4] == s1[:4], (name, s0, s1)
        assert s0[4] > 0
        out[f"{name}_vol"] = vol
        out[f"{name}_verts"] = v0
        out[f"{name}_stats"] = np.array([len(v0), len(f0), *s0], dtype=np.float64)
        out[f"{name}_lorensen"] = np.array([len(v1), len(f1), s1[4], s1[5]], dtype=np.float64)
        print(name, "V", len(v0), "F", len(f0), "euler", s0[0], "components", s0[3], "volume", s0[4], s1[4], "area", s0[5], s1[5])
    path = os.path.join(HERE, "mesh_mc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
