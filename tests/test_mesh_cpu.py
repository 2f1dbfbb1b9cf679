"""Mesh export without a GPU: the generated 256-case table through nmf_mc_case_triangles (watertight by construction), argument
validation of the marching-cubes entry points, a numpy restatement of the kernels over the project's table against the skimage
fixture (tests/golden/mesh_mc.npz), the PLY writer and the command line's --help."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesh_mc.npz")
LEVEL = 0.005


# ---- the numbering of include/nmf_hip.h ------------------------------------------------------------------------------------
def corner_xyz(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e):
    axis, k = e >> 2, e & 3
    others = [a for a in range(3) if a != axis]
    c0 = ((k & 1) << others[0]) | ((k >> 1) << others[1])
    return c0, c0 | (1 << axis)


EDGES = [edge_corners(e) for e in range(12)]
FACES = [[c for c in range(8) if ((c >> axis) & 1) == side] for axis in range(3) for side in range(2)]


def face_edges(face):
    return [e for e, (a, b) in enumerate(EDGES) if a in face and b in face]


def table():
    from nmf_amd import hip
    return [hip.mc_case_triangles(c) for c in range(256)]


def crossing(case):
    return {e for e, (a, b) in enumerate(EDGES) if ((case >> a) & 1) != ((case >> b) & 1)}


def directed_edges(tris):
    return [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]


def in_a_face(a, b):
    return any(a in face_edges(f) and b in face_edges(f) for f in FACES)


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_table_uses_exactly_the_sign_changing_edges():
    tab = table()
    assert tab[0] == [] and tab[255] == []
    for case, tris in enumerate(tab):
        assert len(tris) <= 5
        used = {e for t in tris for e in t}
        assert used == crossing(case), case                                    # only sign-changing edges, and every one of them
        for t in tris:
            assert len(set(t)) == 3, (case, t)


def test_table_case_lookup_rejects_bad_arguments():
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    out = (C.c_int8 * 16)()
    assert lib.nmf_mc_case_triangles(C.c_int(256), out) < 0 and lib.nmf_mc_case_triangles(C.c_int(-1), out) < 0
    assert lib.nmf_mc_case_triangles(C.c_int(1), None) == -1
    assert lib.nmf_mc_case_triangles(C.c_int(1), out) == 1 and list(out[3:]) == [-1] * 13


def test_table_triangles_close_up_inside_the_cell():
    """every triangle edge that does not lie in a cube face is matched by its reverse (the surface has no hole inside a cell);
    the edges in cube faces, the segments, are used once"""
    for case, tris in enumerate(table()):
        de = directed_edges(tris)
        assert len(set(de)) == len(de), case
        for a, b in de:
            if in_a_face(a, b):
                assert (b, a) not in de, (case, a, b)
            else:
                assert (b, a) in de, (case, a, b)


def _face_segments(case, tris, face):
    fe = face_edges(face)
    return {(a, b) for a, b in directed_edges(tris) if a in fe and b in fe}


def test_table_neighbours_agree_on_every_shared_face():
    """for every pair of cases that can meet at a face (equal signs at the four shared corners) the two cells cut the face by the
    same segments with opposite directions: watertight by construction"""
    tab = table()
    checked = 0
    for axis in range(3):
        hi_face = [c for c in range(8) if (c >> axis) & 1]                       # the lower cell's upper face ...
        lo_face = [c ^ (1 << axis) for c in hi_face]                            # ... is the upper cell's lower face
        to_upper = {e: next(e2 for e2 in range(12) if EDGES[e2] == tuple(c ^ (1 << axis) for c in EDGES[e]))
                    for e in face_edges(hi_face)}
        by_signs = {}
        for case in range(256):
            by_signs.setdefault(tuple((case >> c) & 1 for c in lo_face), []).append(case)
        for lower in range(256):
            seg_lower = _face_segments(lower, tab[lower], hi_face)
            want = {(to_upper[b], to_upper[a]) for a, b in seg_lower}
            for upper in by_signs[tuple((lower >> c) & 1 for c in hi_face)]:
                assert _face_segments(upper, tab[upper], lo_face) == want, (axis, lower, upper)
                checked += 1
    assert checked == 3 * 256 * 16


def test_generated_header_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_table.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the kernels restated in numpy over the project's table ------------------------------------------------------------------
def interpolate_np(a, b, i, level):
    """the kernel's expression in its order, every operation rounded to fp32: i + (level - a) / (b - a)"""
    a, b, lv = a.astype(np.float32), b.astype(np.float32), np.float32(level)
    with np.errstate(all="ignore"):
        return (i.astype(np.float32) + (lv - a) / (b - a)).astype(np.float32)


def mc_numpy(vol, level, tab=None):
    """csrc/mesh.hip in numpy: -> (verts fp32 [V,3] index units, faces int32 [F,3]) in the kernels' order"""
    tab = tab or table()
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    gs = vol.shape
    ins = vol > np.float32(level)
    clamp = lambda ax: np.concatenate([np.arange(1, gs[ax]), [gs[ax] - 1]])      # noqa: E731  (the point above, repeated at the end)
    shifted = lambda arr, d: arr[np.ix_(*[clamp(ax) if d[ax] else np.arange(gs[ax]) for ax in range(3)])]      # noqa: E731
    own = [ins != shifted(ins, [ax == a for a in range(3)]) for ax in range(3)]
    count = own[0].astype(np.int64) + own[1] + own[2]
    base = (np.cumsum(count.reshape(-1)) - count.reshape(-1)).reshape(gs)
    V = int(count.sum())
    verts = np.zeros((V, 3), dtype=np.float32)
    grid = np.stack(np.meshgrid(*[np.arange(g) for g in gs], indexing="ij"), -1)
    rank = np.zeros(gs, dtype=np.int64)
    vid = []
    for ax in range(3):
        vid.append(base + rank)
        m = own[ax]
        p = grid[m].astype(np.float32)
        p[:, ax] = interpolate_np(vol[m], shifted(vol, [ax == a for a in range(3)])[m], grid[m][:, ax], level)
        verts[(base + rank)[m]] = p
        rank = rank + m
    case = np.zeros(gs, dtype=np.int64)
    for c in range(8):
        case |= shifted(ins, corner_xyz(c)).astype(np.int64) << c
    cell = np.zeros(gs, dtype=bool)
    cell[:-1, :-1, :-1] = True
    faces, keys = [], []
    flat = np.arange(vol.size).reshape(gs)
    for cs in np.unique(case[cell]):
        at = np.argwhere(cell & (case == cs))
        for t, tri in enumerate(tab[cs]):
            f = np.zeros((len(at), 3), dtype=np.int64)
            for q, e in enumerate(tri):
                o = at + np.array(corner_xyz(EDGES[e][0]))
                f[:, q] = vid[e >> 2][o[:, 0], o[:, 1], o[:, 2]]
            faces.append(f)
            keys.append(flat[at[:, 0], at[:, 1], at[:, 2]] * 8 + t)
    if not faces:
        return verts, np.zeros((0, 3), dtype=np.int32)
    faces, keys = np.concatenate(faces), np.concatenate(keys)
    return verts, faces[np.argsort(keys, kind="stable")].astype(np.int32)


def mesh_stats(verts, faces):
    """(Euler characteristic, boundary edges, non-manifold edges, components, signed volume, area, edges not traversed once in each
    direction), float64"""
    V, F = len(verts), len(faces)
    de = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    uniq, inv, cnt = np.unique(np.sort(de, axis=1), axis=0, return_inverse=True, return_counts=True)
    fwd = np.bincount(inv.reshape(-1), weights=(de[:, 0] < de[:, 1]).astype(np.float64), minlength=len(uniq))
    unbalanced = int(((cnt == 2) & (fwd != 1)).sum())
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
    return V - len(uniq) + F, int((cnt == 1).sum()), int((cnt > 2).sum()), comps, vol, area, unbalanced


def noise_volume(G, seed):
    """seeded smoothed noise [G,G,G] fp32 on the CPU, zero mean: the level-0 surface is a sponge that meets every kind of case"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(1, 1, G, G, G, generator=g)
    for _ in range(3):
        v = torch.nn.functional.avg_pool3d(torch.nn.functional.pad(v, (1,) * 6, mode="replicate"), 3, stride=1)
    v = v[0, 0]
    return ((v - v.mean()) / v.std()).contiguous()


def lexsorted(v):
    return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]


def fixture_margins(z=None):
    """What the GPU tests may deviate by, derived on the CPU from the fixture alone:
    position: 4 x the largest |numpy fp32 restatement - skimage| over the three volumes (one division's rounding apart);
    volume / area: 2 x the largest relative spread between skimage's two methods and the restatement over the project's table."""
    z = z or np.load(GOLDEN)
    tab = table()
    pos, vol, area = 0.0, 0.0, 0.0
    for name in z["names"]:
        verts, faces = mc_numpy(z[f"{name}_vol"], float(z["level"]), tab)
        st = mesh_stats(verts, faces)
        pos = max(pos, float(np.abs(lexsorted(verts).astype(np.float64) - lexsorted(z[f"{name}_verts"]).astype(np.float64)).max()))
        vols = [st[4], z[f"{name}_stats"][6], z[f"{name}_lorensen"][2]]
        areas = [st[5], z[f"{name}_stats"][7], z[f"{name}_lorensen"][3]]
        vol = max(vol, (max(vols) - min(vols)) / min(vols))
        area = max(area, (max(areas) - min(areas)) / min(areas))
    return dict(position=4 * pos, volume=2 * vol, area=2 * area)


@pytest.mark.parametrize("name", ["box", "sphere", "torus"])
def test_numpy_restatement_over_the_table_matches_skimage(name):
    """the project's table on the fixture volumes (no ambiguous case is met there): skimage's V and F, a closed oriented
    2-manifold with its Euler characteristic and component count, its vertex set, and volume / area within the margins"""
    z = np.load(GOLDEN)
    verts, faces = mc_numpy(z[f"{name}_vol"], float(z["level"]))
    V, F, euler, boundary, nonmanifold, comps, vol, area = z[f"{name}_stats"]
    st = mesh_stats(verts, faces)
    assert (len(verts), len(faces)) == (V, F)
    assert st[:4] == (euler, 0, 0, comps) and boundary == 0 and nonmanifold == 0 and st[6] == 0
    m = fixture_margins(z)
    print(name, "margins", m, "volume", st[4], vol, "area", st[5], area)
    assert np.abs(lexsorted(verts) - lexsorted(z[f"{name}_verts"])).max() <= m["position"]
    assert st[4] > 0 and abs(st[4] - vol) <= m["volume"] * vol and abs(st[5] - area) <= m["area"] * area


def test_numpy_restatement_is_watertight_on_noise():
    """smoothed noise meets the ambiguous cases: still every edge in at most two faces, single ones only on the outer boundary"""
    vol = noise_volume(24, seed=3).numpy()
    verts, faces = mc_numpy(vol, 0.0)
    assert len(faces) > 500
    st = mesh_stats(verts, faces)
    assert st[2] == 0 and st[6] == 0
    de = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    uniq, cnt = np.unique(de, axis=0, return_counts=True)
    on_hull = ((verts == 0) | (verts == 23)).any(axis=1)
    assert on_hull[uniq[cnt == 1]].all()


# ---- argument validation without a GPU ------------------------------------------------------------------------------------------
def test_marching_cubes_arguments_are_checked_without_a_gpu():
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_last_error_string.restype = C.c_char_p
    one = C.c_void_p(16)                                                        # never dereferenced: the calls fail on their arguments
    g = lambda v: C.c_int32(v)                                                  # noqa: E731
    lv = C.c_float(0.5)
    assert lib.nmf_mc_count(None, g(4), g(4), g(4), lv, one, one, one, None) == -1
    assert b"nmf_mc_count" in lib.nmf_last_error_string()
    assert lib.nmf_mc_count(one, g(4), g(4), g(4), lv, None, one, one, None) == -1
    for dims in ((1, 4, 4), (4, 4, 1025), (4, 0, 4), (-3, 4, 4)):
        assert lib.nmf_mc_count(one, *[g(v) for v in dims], lv, one, one, one, None) == -2, dims
        assert lib.nmf_mc_emit(one, *[g(v) for v in dims], lv, one, one, one, C.c_int64(1), C.c_int64(1), one, one, None) == -2
    assert lib.nmf_mc_emit(None, g(4), g(4), g(4), lv, one, one, one, C.c_int64(1), C.c_int64(1), one, one, None) == -1
    assert b"nmf_mc_emit" in lib.nmf_last_error_string()
    assert lib.nmf_mc_emit(one, g(4), g(4), g(4), lv, one, one, one, C.c_int64(1), C.c_int64(1), None, one, None) == -1
    # V or 3 F past 2^31 - 1 is refused before anything is launched
    assert lib.nmf_mc_emit(one, g(4), g(4), g(4), lv, one, one, one, C.c_int64(2 ** 31), C.c_int64(1), one, one, None) == -2
    assert lib.nmf_mc_emit(one, g(4), g(4), g(4), lv, one, one, one, C.c_int64(1), C.c_int64((2 ** 31 - 1) // 3 + 1), one, one,
                           None) == -2
    assert b"2^31" in lib.nmf_last_error_string()
    assert lib.nmf_mc_emit(one, g(4), g(4), g(4), lv, one, one, one, C.c_int64(0), C.c_int64(0), None, None, None) == 0   # empty


def test_marching_cubes_workspace_is_nine_bytes_per_lattice_point():
    from nmf_amd import hip
    lib = C.CDLL(hip.LIB_PATH)
    lib.nmf_mc_workspace_bytes.restype = C.c_int64
    f = lambda *gs: int(lib.nmf_mc_workspace_bytes(*[C.c_int32(v) for v in gs]))      # noqa: E731
    for gs in ((2, 2, 2), (48, 48, 48), (40, 56, 33), (512, 512, 512), (1024, 1024, 1024)):
        assert f(*gs) == 9 * gs[0] * gs[1] * gs[2], gs
    assert f(0, 4, 4) == f(4, -1, 4) == f(-2, -2, -2) == 0


def test_marching_cubes_has_no_cpu_fallback():
    from nmf_amd import hip
    with pytest.raises(hip.NmfHipError):
        hip.marching_cubes(torch.zeros(4, 4, 4), 0.5)


# ---- the PLY writer ---------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """the test's own reader: header lines -> numpy structured arrays (vertex, face)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii")
    lines = header.splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    elems = []
    for ln in lines[2:-1]:
        tok = ln.split()
        if tok[0] == "element":
            elems.append((tok[1], int(tok[2]), []))
        elif tok[1] == "list":
            elems[-1][2].extend([("n", types[tok[2]]), (tok[4], types[tok[3]], (3,))])
        else:
            elems[-1][2].append((tok[2], types[tok[1]]))
    out, off = {}, end
    for name, n, dt in elems:
        dt = np.dtype(dt)
        out[name] = np.frombuffer(raw, dtype=dt, count=n, offset=off)
        off += n * dt.itemsize
    assert off == len(raw)
    return header, out["vertex"], out["face"]


def _toy_mesh(attributes):
    from nmf_amd.mesh import Mesh
    g = torch.Generator().manual_seed(0)
    V, F = 7, 5
    m = Mesh(verts=torch.randn(V, 3, generator=g), faces=torch.randint(0, V, (F, 3), generator=g, dtype=torch.int32))
    if attributes:
        m.normals = torch.nn.functional.normalize(torch.randn(V, 3, generator=g), dim=-1)
        m.albedo = torch.rand(V, 3, generator=g)
        m.albedo[0] = torch.tensor([0.0, 1.0, 0.002])
        m.f0 = torch.rand(V, 3, generator=g)
        m.roughness = torch.rand(V, generator=g)
    return m


def test_write_ply_with_attributes_round_trips_bit_for_bit(tmp_path):
    from nmf_amd.mesh import write_ply
    from nmf_amd.modules.tonemap import SRGBTonemap
    m = _toy_mesh(True)
    write_ply(tmp_path / "a.ply", m)
    header, vert, face = read_ply(tmp_path / "a.ply")
    assert header == ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
                      "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
                      "property uchar blue\nproperty float roughness\nproperty float f0_r\nproperty float f0_g\nproperty float f0_b\n"
                      "element face 5\nproperty list uchar int vertex_indices\nend_header\n")
    same = lambda a, t: np.array_equal(np.asarray(a).view(np.uint32), t.numpy().view(np.uint32))      # noqa: E731
    for i, k in enumerate("xyz"):
        assert same(vert[k], m.verts[:, i].contiguous()) and same(vert["n" + k], m.normals[:, i].contiguous())
    for i, k in enumerate(("f0_r", "f0_g", "f0_b")):
        assert same(vert[k], m.f0[:, i].contiguous())
    assert same(vert["roughness"], m.roughness)
    srgb = torch.floor(SRGBTonemap()(m.albedo).clip(0, 1) * 255).to(torch.uint8).numpy()
    for i, k in enumerate(("red", "green", "blue")):
        assert np.array_equal(vert[k], srgb[:, i])
    assert (vert["red"][0], vert["blue"][0]) == (0, int(np.floor(12.92 * np.float32(0.002) * 255)))      # the linear toe, truncated
    assert (face["n"] == 3).all() and np.array_equal(face["vertex_indices"], m.faces.numpy())


def test_write_ply_positions_only_has_the_reference_layout(tmp_path):
    from nmf_amd.mesh import write_ply
    m = _toy_mesh(False)
    write_ply(tmp_path / "p.ply", m)
    header, vert, face = read_ply(tmp_path / "p.ply")
    assert header == ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
                      "element face 5\nproperty list uchar int vertex_indices\nend_header\n")
    assert vert.dtype.names == ("x", "y", "z") and os.path.getsize(tmp_path / "p.ply") == len(header) + 7 * 12 + 5 * 13
    assert np.array_equal(np.stack([vert[k] for k in "xyz"], 1).view(np.uint32), m.verts.numpy().view(np.uint32))
    assert np.array_equal(face["vertex_indices"], m.faces.numpy())


def test_export_mesh_command_line_help():
    r = subprocess.run([sys.executable, "-m", "nmf_amd.export_mesh", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--reference-spacing" in r.stdout and "--no-attributes" in r.stdout
