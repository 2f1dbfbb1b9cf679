"""Mesh export on the GPU: hip.marching_cubes (csrc/mesh.hip) against the skimage fixture (tests/golden/mesh_mc.npz), property
tests on smoothed noise, sizes / determinism / streams, and extract_mesh, write_ply and the command line end to end on the S1 model."""
import json

import numpy as np
import pytest
import torch

from nmf_amd import hip
from test_hip_metrics import _s1_model
from test_mesh_cpu import GOLDEN, fixture_margins, lexsorted, mc_numpy, mesh_stats, noise_volume, read_ply

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _mc(vol, level):
    v, f = hip.marching_cubes(vol.to(DEV), level)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v, f


def _sign_changes(vol, level):
    """number of lattice edges whose ends differ in insideness, with torch ops"""
    ins = vol > level
    return int((ins[1:] != ins[:-1]).sum() + (ins[:, 1:] != ins[:, :-1]).sum() + (ins[:, :, 1:] != ins[:, :, :-1]).sum())


@pytest.mark.parametrize("name", ["box", "sphere", "torus"])
def test_marching_cubes_vs_skimage_fixture(name):
    """V, F, vertex set, manifoldness, orientation, Euler characteristic, components, signed volume and area against skimage's.
    Margins, derived on the CPU from the fixture alone (test_mesh_cpu.fixture_margins):
      position  4 x max |numpy fp32 restatement - skimage| = 4 x 3.815e-06 = 1.526e-05 lattice units (one ulp at 32..48 is 3.8e-6)
      volume    2 x the spread of skimage lewiner / lorensen / the restatement over the project's table = 2 x 0.344 % = 0.689 %
      area      2 x the same spread = 2 x 0.0487 % = 0.0974 %   (another diagonal in a cell's quads moves both, not the topology)"""
    z = np.load(GOLDEN)
    m = fixture_margins(z)
    level = float(z["level"])
    v, f = _mc(torch.from_numpy(z[f"{name}_vol"]), level)
    verts, faces = v.cpu().numpy(), f.cpu().numpy()
    V, F, euler, _, _, comps, vol, area = z[f"{name}_stats"]
    st = mesh_stats(verts, faces)
    dpos = float(np.abs(lexsorted(verts).astype(np.float64) - lexsorted(z[f"{name}_verts"]).astype(np.float64)).max()) \
        if len(verts) == V else float("nan")
    print(name, "V", len(verts), "F", len(faces), "stats", st, "max |dpos|", dpos, "margins", m, "skimage volume / area", vol, area)
    assert (len(verts), len(faces)) == (V, F)
    assert dpos <= m["position"]
    assert st[1] == 0 and st[2] == 0 and st[6] == 0        # every edge in exactly two faces, traversed once in each direction
    assert st[0] == euler and st[3] == comps
    assert st[4] > 0 and abs(st[4] - vol) <= m["volume"] * vol and abs(st[5] - area) <= m["area"] * area
    # the kernels and their numpy restatement: the same bytes
    rv, rf = mc_numpy(z[f"{name}_vol"], level)
    assert np.array_equal(verts.view(np.uint32), rv.view(np.uint32)) and np.array_equal(faces, rf)


@pytest.mark.parametrize("seed", [11, 12])
def test_marching_cubes_properties_on_smoothed_noise(seed):
    vol = noise_volume(64, seed)
    v, f = _mc(vol, 0.0)
    verts, faces = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    V = len(verts)
    assert V == _sign_changes(vol, 0.0) and len(faces) > 1000
    assert faces.min() >= 0 and faces.max() < V
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    de = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    uniq, cnt = np.unique(de, axis=0, return_counts=True)
    assert cnt.max() <= 2                                                       # every edge in at most two faces
    on_hull = ((verts == 0) | (verts == 63)).any(axis=1)
    assert (cnt == 1).any() and on_hull[uniq[cnt == 1]].all()                   # single edges only on the lattice's outer boundary
    assert mesh_stats(verts, faces)[6] == 0                                     # consistently oriented
    assert np.unique(faces).size == V                                           # every vertex is used


def test_marching_cubes_sizes_and_determinism():
    g = torch.Generator().manual_seed(5)
    vol = torch.nn.functional.interpolate(torch.randn(1, 1, 6, 8, 5, generator=g), size=(40, 56, 33), mode="trilinear",
                                          align_corners=True)[0, 0].contiguous()
    v, f = _mc(vol, 0.1)
    assert v.shape[0] == _sign_changes(vol, 0.1) and f.shape[0] > 0 and int(f.max()) < v.shape[0] and int(f.min()) >= 0
    rv, rf = mc_numpy(vol.numpy(), 0.1)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f.cpu().numpy(), rf)
    assert float(v[:, 0].max()) <= 39 and float(v[:, 1].max()) <= 55 and float(v[:, 2].max()) <= 32 and float(v.min()) >= 0
    # two runs: identical bytes; a side stream: the same result
    v2, f2 = _mc(vol, 0.1)
    assert torch.equal(v, v2) and torch.equal(f, f2)
    side = torch.cuda.Stream()
    dvol = vol.to(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v3, f3 = hip.marching_cubes(dvol, 0.1)
    side.synchronize()
    assert torch.equal(v, v3) and torch.equal(f, f3)
    # a non-contiguous view is triangulated as its values
    v4, f4 = hip.marching_cubes(dvol.transpose(0, 2), 0.1)
    assert v4.shape == v.shape and f4.shape == f.shape


def test_marching_cubes_empty_full_and_nan_volumes():
    for vol in (torch.zeros(8, 9, 10), torch.ones(8, 9, 10), torch.full((5, 5, 5), float("nan"))):
        v, f = _mc(vol, 0.5)
        assert v.shape == (0, 3) and f.shape == (0, 3)                          # no surface, nothing raised
    vol = torch.zeros(7, 7, 7)
    vol[3, 3, 3] = 1.0                                                          # one inside point: an octahedron
    v, f = _mc(vol, 0.5)
    assert v.shape == (6, 3) and f.shape == (8, 3)
    st = mesh_stats(v.cpu().numpy(), f.cpu().numpy())
    assert st[:4] == (2, 0, 0, 1) and st[6] == 0 and st[4] == pytest.approx(4 / 3 * 0.5 ** 3, rel=1e-6)
    vol[3, 3, 3] = float("nan")                                                 # a NaN counts as outside
    assert _mc(vol, 0.5)[0].shape == (0, 3)
    with pytest.raises(hip.NmfHipError):
        hip.marching_cubes(torch.zeros(1, 4, 4, device=DEV), 0.5)
    with pytest.raises(hip.NmfHipError):
        hip.marching_cubes(torch.zeros(4, 4, device=DEV), 0.5)


def _head_formulas(nerf, app):
    """albedo, f0, roughness as test_hip_material_maps._restate states them, float64 (compared within that test's 2e-5)"""
    dm = nerf.model.diffuse_module
    ps = [p.detach().double() for p in dm._head_params()]
    W, b = torch.cat(ps[0::2], 0), torch.cat(ps[1::2], 0)
    a = app.double() @ W.T + b
    albedo = torch.sigmoid(float(dm.diffuse_mul) * a[:, 0:3] + float(dm.diffuse_bias)).clip(0, 1)
    f0 = torch.sigmoid(a[:, 6:9] + float(dm.f0_bias))
    r1 = (torch.sigmoid(a[:, 9] + float(dm.roughness_bias)) * 0.5).clip(1e-2, 1)
    return albedo, f0, r1


def test_extract_mesh_on_the_s1_model(tmp_path, capsys):
    """the S1 scene is a cube of half-size 0.75 in a +-1.5 box: positions, signed volume, outward unit normals, materials,
    the reference's placement, the PLY file and the command line"""
    from nmf_amd import export_mesh
    from nmf_amd.mesh import extract_mesh, write_ply
    G = 128
    nerf, cfg = _s1_model(grid=G)
    mesh = extract_mesh(nerf)
    V, F = mesh.verts.shape[0], mesh.faces.shape[0]
    assert V > 1000 and F > 2000 and mesh.has_attributes and set(mesh.seconds) == {"density", "triangulate", "attributes"}
    h = 3.0 / (G - 1)                                                           # the lattice spacing
    p = mesh.verts.double()
    dist = (p.abs() - 0.75).abs().min(dim=1).values                             # to the nearest face plane of the cube
    assert float(p.abs().max()) <= 0.75 + h and float(dist.max()) <= h
    st = mesh_stats(mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy())
    print("S1 mesh V", V, "F", F, "stats", st, "seconds", mesh.seconds)
    assert st[1] == 0 and st[2] == 0 and st[6] == 0                             # closed and oriented: the signed volume means something
    assert abs(st[4] - 1.5 ** 3) <= h * st[5]                                   # within the discretisation: spacing x area
    n = mesh.normals.double()
    assert float((n.norm(dim=1) - 1).abs().max()) <= 1e-4
    away = (p.abs() < 0.75 - 4 * h).sum(dim=1) == 2                             # on a face, away from the cube's edges
    assert int(away.sum()) > V // 2 and bool(((n * p).sum(dim=1)[away] > 0).all())
    with torch.no_grad():
        app = nerf.rf.compute_appfeature(mesh.verts)
    albedo, f0, r1 = _head_formulas(nerf, app)
    for got, want, what in ((mesh.albedo, albedo, "albedo"), (mesh.f0, f0, "f0"), (mesh.roughness, r1, "roughness")):
        assert got.shape == want.shape and float((got.double() - want).abs().max()) <= 2e-5, what
    # positions: where getDenseAlpha sampled; the reference's placement on request
    aabb = nerf.sampler.aabb.to(DEV).float()
    size = aabb[1] - aabb[0]
    assert torch.equal(mesh.verts, aabb[0] + mesh.index_verts * (size / (G - 1)))
    ref = extract_mesh(nerf, attributes=False, reference_spacing=True)
    assert not ref.has_attributes and torch.equal(ref.faces, mesh.faces) and torch.equal(ref.index_verts, mesh.index_verts)
    assert torch.equal(ref.verts, aabb[0] + ref.index_verts * (size / G))
    # a finer, non-cubic lattice than the field's: the field's iso-surface lies within one FIELD spacing of the cube (its tables
    # have 128 points per axis) and a vertex lies on a lattice edge that straddles it, at most one (coarsest: 3 / 127) lattice spacing on
    fine = extract_mesh(nerf, resolution=[160, 128, 144], attributes=False)
    assert fine.verts.shape[0] > V and float((fine.verts.abs().max())) <= 0.75 + h + 3.0 / 127
    # PLY + command line
    write_ply(tmp_path / "m.ply", mesh)
    _, vert, face = read_ply(tmp_path / "m.ply")
    assert len(vert) == V and len(face) == F and np.array_equal(face["vertex_indices"], mesh.faces.cpu().numpy())
    assert np.array_equal(vert["x"].view(np.uint32), mesh.verts[:, 0].contiguous().cpu().numpy().view(np.uint32))
    assert np.array_equal(vert["roughness"].view(np.uint32), mesh.roughness.cpu().numpy().view(np.uint32))
    ck = str(tmp_path / "s1.th")
    nerf.save(ck, cfg["arch"])
    capsys.readouterr()
    rec = export_mesh.main(["--ckpt", ck])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert rec["output"] == str(tmp_path / "s1.ply") and line["V"] == rec["V"] == V and rec["F"] == F
    assert set(rec["seconds"]) == {"density", "triangulate", "attributes", "write"}
    _, vert2, face2 = read_ply(rec["output"])
    assert len(vert2) == V and len(face2) == F and "nx" in vert2.dtype.names
    rec = export_mesh.main(["--ckpt", ck, "--no-attributes", "--reference-spacing", "--resolution", "64", "--output",
                            str(tmp_path / "p.ply")])
    _, vert3, face3 = read_ply(tmp_path / "p.ply")
    assert vert3.dtype.names == ("x", "y", "z") and len(vert3) == rec["V"] and len(face3) == rec["F"] and 0 < rec["V"] < V
