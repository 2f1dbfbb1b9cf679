"""The texture atlas of the mesh export without a GPU: the layout arithmetic (nmf_amd.mesh.atlas_layout / atlas_uv), its two
properties -- (P1) every texel of a used square has exactly one owner, (P2) a bilinear fetch inside a face's UV triangle reads only
texels of that face --, the agreement of UVs and texels (v flip included), write_obj, and the argument checks of the two entry points.

atlas_numpy / store_numpy restate the two kernels of csrc/atlas.hip in numpy (ownership, fp32 positions in the kernel's expression
order, the 8-bit quantisation); tests/test_hip_atlas.py compares the kernels with them."""
import os

import numpy as np
import pytest

WEIGHT_EPS = 1e-9          # a bilinear weight below this is the float64 rounding of u W - 0.5 (at most W 2^-52 < 4e-12), not a fetch
SRGB_LIMIT = np.float32(0.0031308)
FILL = dict(albedo=(0, 0, 0), f0=(0, 0, 0), roughness=0, normal=(128, 128, 128))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def atlas_numpy(verts, faces, W, T, dtype=np.float32):
    """-> (face_of int32 [W W], pos dtype [W W, 3]) of the whole atlas: the owner of texel t = y W + x and its point on the face,
    b1 = i / b, b2 = j / b, b0 = (1 - b1) - b2, p = (b0 v0 + b1 v1) + b2 v2, one rounding per operation in `dtype`"""
    verts = np.asarray(verts, dtype=dtype).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    n, b = W // T, T - 3
    t = np.arange(W * W, dtype=np.int64)
    y, x = t // W, t % W
    cx, cy = x // T, y // T
    i, j = x - cx * T, y - cy * T
    upper = i + j >= T - 1
    f = 2 * (cy * n + cx) + upper
    i, j = np.where(upper, T - 1 - i, i), np.where(upper, T - 1 - j, j)
    own = (cx < n) & (cy < n) & (f < F)
    tri = faces[np.where(own, f, 0)] if F else np.zeros((W * W, 3), dtype=np.int64)
    own &= ((tri >= 0) & (tri < V)).all(axis=1)
    tri = np.where(own[:, None], tri, 0)
    v0, v1, v2 = (verts[tri[:, k]] if V else np.zeros((W * W, 3), dtype=dtype) for k in range(3))
    b1, b2 = i.astype(dtype) / dtype(b), j.astype(dtype) / dtype(b)
    b0 = (dtype(1) - b1) - b2
    pos = (b0[:, None] * v0 + b1[:, None] * v1) + b2[:, None] * v2
    pos[~own] = 0
    return np.where(own, f, -1).astype(np.int32), pos.astype(dtype)


def srgb_f32(x):
    """modules/tonemap.py:38-49 in fp32, one rounding per operation (the power is the host's powf)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        hi = np.float32(1.055) * np.power(np.maximum(x, SRGB_LIMIT), np.float32(1.0) / np.float32(2.4)) - np.float32(0.055)
        return np.where(x > SRGB_LIMIT, hi, np.float32(12.92) * x).astype(np.float32)


def quantise(kind, v, dtype=np.float32):
    """the store's bytes of the values v of one plane (kind: albedo, f0, roughness, normal); a NaN counts as 0, the cast truncates.
    dtype float64: the quantiser Q the bake test brackets a byte with"""
    v = np.asarray(v, dtype=dtype)
    v = np.where(np.isnan(v), dtype(0), v)
    with np.errstate(all="ignore"):
        if kind == "normal":
            return np.clip(v * dtype(127) + dtype(128), 0, 255).astype(np.uint8)
        if kind == "albedo":
            if dtype == np.float32:
                v = srgb_f32(v)
            else:
                v = np.where(v > 0.0031308, 1.055 * np.power(np.maximum(v, 0.0031308), 1.0 / 2.4) - 0.055, 12.92 * v)
        return (np.clip(v, 0, 1) * dtype(255)).astype(np.uint8)


def store_numpy(face_of, albedo, f0, roughness, normal):
    """-> dict of the four uint8 planes of these texels: albedo, f0, normal [n, 3], roughness [n]; unowned texels hold FILL"""
    own = np.asarray(face_of) >= 0
    out = {}
    for kind, v in (("albedo", albedo), ("f0", f0), ("roughness", roughness), ("normal", normal)):
        q = quantise(kind, v)
        q[~own] = FILL[kind]
        out[kind] = q
    return out


def corner_texels(F, W, T):
    """the texel (X, Y) that carries corner k of face f, restated face by face -> int64 [F, 3, 2]"""
    n, b = W // T, T - 3
    out = np.zeros((F, 3, 2), dtype=np.int64)
    for f in range(F):
        s = f // 2
        ox, oy = (s % n) * T, (s // n) * T
        for k, (i, j) in enumerate(((0, 0), (b, 0), (0, b))):
            if f % 2:
                i, j = T - 1 - i, T - 1 - j
            out[f, k] = (ox + i, oy + j)
    return out


def uv_of_texels(xy, W):
    xy = np.asarray(xy, dtype=np.float64)
    return np.stack([(xy[..., 0] + 0.5) / W, 1.0 - (xy[..., 1] + 0.5) / W], -1)


def bilinear_taps(uv, W):
    """the four taps of a bilinear fetch at uv [P, 2] (float64; v grows upwards, row 0 of the atlas is on top, texel centres at
    half-integers, no wrap) -> (x [P, 4], y [P, 4], weight [P, 4])"""
    px, py = uv[:, 0] * W - 0.5, (1.0 - uv[:, 1]) * W - 0.5
    x0, y0 = np.floor(px), np.floor(py)
    fx, fy = px - x0, py - y0
    x = np.stack([x0, x0 + 1, x0, x0 + 1], -1).astype(np.int64)
    y = np.stack([y0, y0, y0 + 1, y0 + 1], -1).astype(np.int64)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1)
    return x, y, w


def bilinear_fetch(atlas, uv):
    """atlas float64 [W, W] sampled at uv [P, 2]; taps below WEIGHT_EPS are not read (they may lie outside the atlas)"""
    W = atlas.shape[0]
    x, y, w = bilinear_taps(uv, W)
    use = w > WEIGHT_EPS
    vals = atlas[np.where(use, y, 0).clip(0, W - 1), np.where(use, x, 0).clip(0, W - 1)]
    return (np.where(use, w, 0.0) * vals).sum(-1)


def barycentric_samples(rng, interior=10000, per_edge=200):
    """corners, points along the three edges, and `interior` random interior points -> float64 [P, 3], rows summing to 1"""
    e = np.linspace(0.0, 1.0, per_edge)
    z = np.zeros_like(e)
    edges = np.concatenate([np.stack([1 - e, e, z], -1), np.stack([z, 1 - e, e], -1), np.stack([e, z, 1 - e], -1)])
    return np.concatenate([np.eye(3), edges, rng.dirichlet((1.0, 1.0, 1.0), size=interior)])


def random_mesh(rng, V, F, degenerate=True):
    """verts fp32 [V, 3] in +-1.5, faces int32 [F, 3] of random indices; the last face repeats an index (zero area)"""
    verts = rng.uniform(-1.5, 1.5, size=(V, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32) if F else np.zeros((0, 3), dtype=np.int32)
    if degenerate and F:
        faces[-1, 2] = faces[-1, 1]
    return verts, faces


# ---- layout ------------------------------------------------------------------------------------------------------------------------
def test_layout_values():
    from nmf_amd.mesh import atlas_layout
    for (F, W), T in {(1, 4): 4, (3, 8): 4, (7, 16): 8, (5000, 256): 5, (6908, 512): 8, (49148, 4096): 26, (811148, 8192): 12,
                      (7, 19): 9, (0, 16): 16, (2, 16384): 16384}.items():
        lay = atlas_layout(F, W)
        assert lay == (W, T, W // T, T - 3), (F, W, lay)
        assert (W // T) ** 2 >= -(-F // 2) and (T == W or (W // (T + 1)) ** 2 < -(-F // 2))          # T fits, T + 1 does not
    with pytest.raises(ValueError, match=r"\b8\b.*--resolution"):
        atlas_layout(3, 4)
    for W in (3, 16385, 0, -4):
        with pytest.raises(ValueError):
            atlas_layout(1, W)
    with pytest.raises(ValueError):
        atlas_layout(-1, 16)
    face_of, pos = atlas_numpy(np.zeros((0, 3)), np.zeros((0, 3)), 16, 16)
    assert (face_of == -1).all() and not pos.any()


CASES = [(7, 2 * T + 1, T) for T in (4, 5, 6, 7, 8, 9, 13, 26)] + [(8, 2 * T, T) for T in (4, 13)]


@pytest.mark.parametrize("F,W,T", CASES)
def test_p1_every_texel_of_a_used_square_has_one_owner(F, W, T):
    from nmf_amd.mesh import atlas_layout
    assert atlas_layout(F, W)[:2] == (W, T)
    n = W // T
    count = np.zeros((W, W), dtype=np.int64)
    owner = np.full((W, W), -1, dtype=np.int64)
    for f in range(F):                               # face by face: the texels its half of its square gives it
        s = f // 2
        ox, oy = (s % n) * T, (s // n) * T
        for j in range(T):
            for i in range(T):
                if (i + j <= T - 2) == (f % 2 == 0):
                    count[oy + j, ox + i] += 1
                    owner[oy + j, ox + i] = f
    used = np.zeros((W, W), dtype=bool)
    for s in range(F // 2):                          # the squares with both faces (an odd F leaves the last one half used)
        used[(s // n) * T:(s // n + 1) * T, (s % n) * T:(s % n + 1) * T] = True
    assert (count[used] == 1).all() and count.max() == 1
    assert (np.bincount(owner[owner >= 0], minlength=F)[0::2] == T * (T - 1) // 2).all()
    assert (np.bincount(owner[owner >= 0], minlength=F)[1::2] == T * (T + 1) // 2).all()
    rng = np.random.default_rng(T)
    verts, faces = random_mesh(rng, 9, F)
    face_of, _ = atlas_numpy(verts, faces, W, T)
    assert np.array_equal(face_of.reshape(W, W), owner)
    if W > n * T:                                    # the left-over row and column
        assert (owner[n * T:] == -1).all() and (owner[:, n * T:] == -1).all()
    if F % 2:                                        # the upper half of the last square
        s = F // 2
        sq = owner[(s // n) * T:(s // n + 1) * T, (s % n) * T:(s % n + 1) * T]
        assert (sq == -1).sum() == T * (T + 1) // 2 and (sq == F - 1).sum() == T * (T - 1) // 2


@pytest.mark.parametrize("F,W,T", CASES)
def test_p2_a_bilinear_fetch_inside_a_chart_reads_only_its_face(F, W, T):
    from nmf_amd.mesh import atlas_layout, atlas_uv
    lay = atlas_layout(F, W)
    xy = corner_texels(F, W, T)
    uv = uv_of_texels(xy, W)
    assert np.array_equal(atlas_uv(F, lay), uv.astype(np.float32)) and atlas_uv(F, lay).dtype == np.float32
    rng = np.random.default_rng(100 + T)
    face_of, _ = atlas_numpy(*random_mesh(rng, 9, F, degenerate=False), W, T)
    owner = face_of.reshape(W, W)
    bary = barycentric_samples(rng)
    assert len(bary) >= 10000 + 3
    for f in range(F):
        x, y, w = bilinear_taps(bary @ uv[f], W)
        hit = w > WEIGHT_EPS
        assert hit.any(axis=1).all() and abs(np.where(hit, w, 0).sum(-1) - 1).max() < 1e-6
        assert (x[hit] >= 0).all() and (x[hit] < W).all() and (y[hit] >= 0).all() and (y[hit] < W).all()
        assert (owner[y[hit], x[hit]] == f).all(), f


def test_uvs_and_texels_agree():
    """a linear function g(p) = a . p + c baked at the restated texel positions comes back from a bilinear fetch at the UV of any
    barycentric point as g of that point (bilinear interpolation is exact on a linear function, gutter texels hold its
    extrapolation): the UV rule, its v flip and the texel positions describe the same map.  Margin: 4 x the largest deviation of
    the fp32 restated positions from their float64 values, x |a|_1 (the texels' own rounding; W = 16 makes the fp32 UVs exact)."""
    from nmf_amd.mesh import atlas_layout, atlas_uv
    F, W = 7, 16
    lay = atlas_layout(F, W)
    rng = np.random.default_rng(7)
    verts, faces = random_mesh(rng, 6, F, degenerate=False)
    face_of, p32 = atlas_numpy(verts, faces, W, lay[1])
    _, p64 = atlas_numpy(verts.astype(np.float64), faces, W, lay[1], dtype=np.float64)
    own = face_of >= 0
    dev = float(np.abs(p32[own].astype(np.float64) - p64[own]).max())
    a, c = rng.uniform(-2, 2, size=3), 0.37
    margin = 4 * dev * float(np.abs(a).sum())
    atlas = np.where(own, p32.astype(np.float64) @ a + c, np.nan).reshape(W, W)          # an unowned texel poisons a fetch
    uv = atlas_uv(F, lay).astype(np.float64)
    worst = 0.0
    for f in range(F):
        bary = barycentric_samples(rng, interior=2000, per_edge=50)
        got = bilinear_fetch(atlas, bary @ uv[f])
        want = (bary @ verts[faces[f]].astype(np.float64)) @ a + c
        assert np.isfinite(got).all(), f
        worst = max(worst, float(np.abs(got - want).max()))
    print("max |fetch - g|", worst, "margin", margin, "position deviation", dev)
    assert 0 < dev < 1e-6 and worst <= margin


def test_quantiser_special_values():
    """the bytes the store's rules give the special inputs, stated: albedo through sRGB (srgb(1) is 1.055f - 0.055f = 1 - 2^-24 in fp32,
    so 254 -- as mesh.albedo_to_8bit gives it), f0 / roughness linear, normals 127 v + 128"""
    lim = np.float32(0.0031308)
    vals = np.array([0.0, 1.0, -0.5, 1.5, np.nan, np.inf, -np.inf, lim, np.nextafter(lim, np.float32(0)), np.nextafter(lim, np.float32(1))],
                    dtype=np.float32)
    assert quantise("albedo", vals).tolist() == [0, 254, 0, 255, 0, 255, 0, 10, 10, 10]
    assert quantise("f0", vals).tolist() == [0, 255, 0, 255, 0, 255, 0, 0, 0, 0]
    assert quantise("roughness", vals).tolist() == [0, 255, 0, 255, 0, 255, 0, 0, 0, 0]
    assert quantise("normal", vals).tolist() == [128, 255, 64, 255, 128, 255, 0, 128, 128, 128]
    import torch
    from nmf_amd.mesh import albedo_to_8bit
    fin = np.isfinite(vals)
    assert albedo_to_8bit(torch.from_numpy(vals[fin])).tolist() == quantise("albedo", vals[fin]).tolist()


# ---- write_obj ---------------------------------------------------------------------------------------------------------------------
def parse_obj(path):
    out = dict(v=[], vt=[], vn=[], f=[], mtllib=None, usemtl=None)
    for ln in open(path):
        tok = ln.split()
        if not tok or tok[0].startswith("#"):
            continue
        if tok[0] in ("v", "vt", "vn"):
            out[tok[0]].append([float(t) for t in tok[1:]])
        elif tok[0] == "f":
            out["f"].append([[int(k) for k in t.split("/")] for t in tok[1:]])
        elif tok[0] in ("mtllib", "usemtl"):
            out[tok[0]] = tok[1]
    return out


def test_write_obj_round_trip(tmp_path):
    import torch
    from PIL import Image
    from nmf_amd.mesh import Mesh, Textures, atlas_layout, atlas_uv, write_obj
    rng = np.random.default_rng(3)
    verts = torch.tensor([[0, 0, 0], [1, 0, 0.25], [1, 1, 0], [0, 1, 0.1]], dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    normals = torch.nn.functional.normalize(torch.tensor(rng.normal(size=(4, 3)), dtype=torch.float32), dim=1)
    mesh = Mesh(verts=verts, faces=faces, normals=normals)
    lay = atlas_layout(2, 8)
    tex = Textures(albedo=rng.integers(0, 256, (8, 8, 3), dtype=np.uint8), f0=rng.integers(0, 256, (8, 8, 3), dtype=np.uint8),
                   normal=torch.from_numpy(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)),
                   roughness=rng.integers(0, 256, (8, 8), dtype=np.uint8), uv=atlas_uv(2, lay), layout=lay)
    paths = write_obj(tmp_path / "two.obj", mesh, tex)
    assert sorted(os.listdir(tmp_path)) == ["two.mtl", "two.obj", "two_albedo.png", "two_f0.png", "two_normal.png", "two_roughness.png"]
    obj = parse_obj(paths["obj"])
    assert (len(obj["v"]), len(obj["vn"]), len(obj["vt"]), len(obj["f"])) == (4, 4, 6, 2)
    assert np.array_equal(np.array(obj["v"], dtype=np.float32), verts.numpy())
    assert np.array_equal(np.array(obj["vn"], dtype=np.float32), normals.numpy())
    assert np.array_equal(np.array(obj["vt"], dtype=np.float32).reshape(2, 3, 2), atlas_uv(2, lay))
    f = np.array(obj["f"])                                                      # [F, 3 corners, (v, vt, vn)], 1-based
    assert np.array_equal(f[:, :, 0] - 1, faces.numpy()) and np.array_equal(f[:, :, 2], f[:, :, 0])
    assert np.array_equal(f[:, :, 1] - 1, np.arange(6).reshape(2, 3))
    assert obj["mtllib"] == "two.mtl" and obj["usemtl"]
    mtl = open(paths["mtl"]).read()
    keys = {ln.split()[0]: ln.split()[1] for ln in mtl.splitlines() if ln and not ln.startswith("#")}
    assert keys["newmtl"] == obj["usemtl"]
    assert (keys["map_Kd"], keys["map_Ks"], keys["map_Pr"], keys["norm"]) == ("two_albedo.png", "two_f0.png", "two_roughness.png",
                                                                             "two_normal.png")
    assert all(os.path.exists(tmp_path / keys[k]) for k in ("map_Kd", "map_Ks", "map_Pr", "norm")) and {"Kd", "Ks", "Pr"} <= set(keys)
    comments = " ".join(ln for ln in mtl.splitlines() if ln.startswith("#")).lower()
    assert "world-space" in comments and "srgb" in comments and "linear" in comments and "mip" in comments and "bilinear" in comments
    for m in ("albedo", "f0", "normal", "roughness"):
        img = Image.open(paths[m])
        want = getattr(tex, m)
        want = want.numpy() if isinstance(want, torch.Tensor) else want
        assert img.size == (8, 8) and img.mode == ("L" if m == "roughness" else "RGB") and np.array_equal(np.asarray(img), want)
    # a mesh without normals: v/vt corners; a path without the extension gets it
    paths = write_obj(tmp_path / "bare", Mesh(verts=verts, faces=faces), tex)
    obj = parse_obj(paths["obj"])
    assert paths["obj"].endswith("bare.obj") and not obj["vn"] and np.array(obj["f"]).shape == (2, 3, 2)
    with pytest.raises(ValueError):
        write_obj(tmp_path / "bad.obj", Mesh(verts=verts, faces=faces[:1]), tex)


# ---- the entry points' argument checks (no GPU: a refused call launches nothing) ------------------------------------------------------
def test_bad_arguments_are_rejected_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    import torch
    from nmf_amd import hip
    lib, one = hip._lib, 16                          # (a pointer that is never dereferenced: every call here fails on its arguments)
    err = lambda: lib.nmf_last_error_string().decode()
    ok = dict(V=4, F=2, W=8, T=8, t0=0, n=64)

    def texels(verts=one, faces=one, pos=one, face_of=one, **kw):
        a = dict(ok, **kw)
        return lib.nmf_atlas_texels(verts, faces, a["V"], a["F"], a["W"], a["T"], a["t0"], a["n"], pos, face_of, None)

    for kw in (dict(verts=None), dict(faces=None), dict(pos=None), dict(face_of=None), dict(F=-1), dict(V=-1), dict(W=3, T=3), dict(W=16385),
               dict(T=3), dict(T=9), dict(F=3), dict(W=16, T=5, F=19), dict(t0=-1), dict(n=-1), dict(n=65), dict(t0=1), dict(t0=65, n=0)):
        assert texels(**kw) == -1 and "nmf_atlas_texels" in err(), kw
    assert texels(n=0) == 0 and texels(t0=64, n=0) == 0 and texels(verts=None, faces=None, V=0, F=0, n=0) == 0

    def store(face_of=one, inputs=(one, one, one, one), planes=(one, one, one, one), t0=0, n=64, W=8):
        return lib.nmf_atlas_store(face_of, *inputs, t0, n, W, *planes, None)

    for kw in (dict(face_of=None), dict(W=3), dict(W=16385), dict(t0=-1), dict(n=-1), dict(n=65), dict(t0=60, n=5),
               dict(inputs=(None, one, one, one)), dict(inputs=(one, one, None, one)), dict(inputs=(one, one, one, None))):
        assert store(**kw) == -1 and "nmf_atlas_store" in err(), kw
    assert store(n=0) == 0 and store(planes=(None,) * 4) == 0 and store(inputs=(None,) * 4, planes=(None,) * 4) == 0
    # the wrappers refuse host tensors
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(hip.NmfHipError):
        hip.atlas_texels(v, f, 8, 8)
    with pytest.raises(hip.NmfHipError):
        hip.atlas_store(torch.zeros(64, dtype=torch.int32), torch.zeros(64, 3), torch.zeros(64, 3), torch.zeros(64), torch.zeros(64, 3), 0, 8,
                        torch.zeros(8, 8, 3, dtype=torch.uint8))
