"""The texture bake of the mesh export on the GPU: hip.atlas_texels and hip.atlas_store (csrc/atlas.hip) against their numpy
restatement (tests/test_atlas_cpu.py: same face, same position bits, same bytes), and bake_textures / write_obj / the command line
on the S1 model against the field's own queries in float64."""
import json
import os

import numpy as np
import pytest
import torch

from nmf_amd import hip
from test_atlas_cpu import FILL, atlas_numpy, parse_obj, quantise, random_mesh, store_numpy
from test_hip_mesh import _head_formulas
from test_hip_metrics import _s1_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64          # bytes of 0xA5 on either side of an output


def _guarded(nbytes):
    """a device buffer of nbytes between two guards -> (whole uint8 buffer, the uint8 view of the middle)"""
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


def _texels(verts, faces, W, T, t0, n, **kw):
    """hip.atlas_texels into guarded outputs -> (face_of int32 [n], pos fp32 [n, 3]) on the host, the guards checked"""
    pbuf, pmid = _guarded(12 * n)
    fbuf, fmid = _guarded(4 * n)
    out = (pmid.view(torch.float32).view(n, 3), fmid.view(torch.int32))
    pos, face_of = hip.atlas_texels(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV), W, T, t0, n, out=out, **kw)
    torch.cuda.synchronize()
    assert _guards_intact(pbuf) and _guards_intact(fbuf)
    return face_of.cpu().numpy(), pos.cpu().numpy()


@pytest.mark.parametrize("F,W", [(1, 4), (2, 4), (3, 8), (7, 19), (5000, 256)])
def test_atlas_texels_vs_numpy(F, W):
    """the owner of every texel and the bits of its position; the whole atlas and a range that crosses rows and is not wave-aligned"""
    from nmf_amd.mesh import atlas_layout
    _, T, _, _ = atlas_layout(F, W)
    rng = np.random.default_rng(1000 + F)
    verts, faces = random_mesh(rng, max(5, F // 2), F)
    assert F < 2 or faces[-1, 1] == faces[-1, 2]                                 # the degenerate face is there
    want_f, want_p = atlas_numpy(verts, faces, W, T)
    got_f, got_p = _texels(verts, faces, W, T, 0, W * W)
    assert np.array_equal(got_f, want_f)
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    assert (want_f >= 0).any() and ((want_f < 0).any() or (F, W) == (2, 4))
    lo, hi = (37, 1037) if W * W >= 1037 else (W * W // 5, W * W - 3)
    part_f, part_p = _texels(verts, faces, W, T, lo, hi - lo)
    assert np.array_equal(part_f, got_f[lo:hi]) and np.array_equal(part_p.view(np.uint32), got_p[lo:hi].view(np.uint32))
    # hip.atlas_texels allocates the same; n defaults to the rest of the atlas
    pos, face_of = hip.atlas_texels(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV), W, T, t0=lo)
    assert np.array_equal(face_of.cpu().numpy(), got_f[lo:]) and torch.equal(pos.cpu(), torch.from_numpy(got_p[lo:]))


def test_atlas_texels_refuses_bad_face_indices_and_sizes():
    from nmf_amd.mesh import atlas_layout
    F, W = 3, 8
    T = atlas_layout(F, W)[1]
    verts, faces = random_mesh(np.random.default_rng(5), 6, F, degenerate=False)
    dv = torch.from_numpy(verts).to(DEV)
    for bad in (6, -1):                                                          # V, and a negative index
        fb = faces.copy()
        fb[1, 1] = bad
        pbuf, pmid = _guarded(12 * W * W)
        fbuf, fmid = _guarded(4 * W * W)
        with pytest.raises(hip.NmfHipError, match=r"\[-2\]"):
            hip.atlas_texels(dv, torch.from_numpy(fb).to(DEV), W, T, out=(pmid.view(torch.float32).view(-1, 3), fmid.view(torch.int32)))
        torch.cuda.synchronize()
        assert bool((pbuf == 0xA5).all()) and bool((fbuf == 0xA5).all())         # nothing was written
        # the kernel itself never reads verts with such an index: without the wrapper's check the face's texels come out unowned
        got_f, got_p = _texels(verts, fb, W, T, 0, W * W, check_faces=False)
        want_f, want_p = atlas_numpy(verts, fb, W, T)
        assert (want_f != 1).all() and (want_f == 0).any() and (want_f == 2).any()
        assert np.array_equal(got_f, want_f) and np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    df = torch.from_numpy(faces).to(DEV)
    for kw in (dict(W=3, T=4), dict(W=8, T=3), dict(W=8, T=8), dict(W=8, T=4, t0=60, n=5), dict(W=8, T=4, t0=-1, n=4)):
        with pytest.raises(hip.NmfHipError, match=r"\[-1\]"):
            hip.atlas_texels(dv, df, **kw)
    pos, face_of = hip.atlas_texels(dv, df, 8, 4, t0=64)                         # an empty range is no error
    assert pos.shape == (0, 3) and face_of.shape == (0,)


def _safe(rng, kind, shape, lo, hi):
    """fp32 values in [lo, hi) whose float64 quantiser argument (255 srgb(a), 255 v or 127 v + 128) has its fractional part in
    [0.05, 0.95]: redrawn on the CPU until it has, so that an ulp of powf or of a product cannot move a byte"""
    def frac_ok(v):
        v = v.astype(np.float64)
        if kind == "albedo":
            x = 255.0 * np.where(v > 0.0031308, 1.055 * np.power(np.maximum(v, 0.0031308), 1.0 / 2.4) - 0.055, 12.92 * v)
        else:
            x = 127.0 * v + 128.0 if kind == "normal" else 255.0 * v
        fr = x - np.floor(x)
        return (fr >= 0.05) & (fr <= 0.95)
    v = rng.uniform(lo, hi, size=shape).astype(np.float32)
    for _ in range(200):
        bad = ~frac_ok(v)
        if not bad.any():
            return v
        v[bad] = rng.uniform(lo, hi, size=int(bad.sum())).astype(np.float32)
    raise AssertionError("no safe draw")


LIM = np.float32(0.0031308)
SPECIAL = np.array([0.0, 1.0, -0.5, 1.5, np.nan, np.inf, -np.inf, LIM, np.nextafter(LIM, np.float32(0)), np.nextafter(LIM, np.float32(1))],
                   dtype=np.float32)
SPECIAL_BYTES = dict(albedo=[0, 254, 0, 255, 0, 255, 0, 10, 10, 10],              # srgb(1) = 1.055f - 0.055f = 1 - 2^-24: 254, as albedo_to_8bit
                     f0=[0, 255, 0, 255, 0, 255, 0, 0, 0, 0], roughness=[0, 255, 0, 255, 0, 255, 0, 0, 0, 0],
                     normal=[128, 255, 64, 255, 128, 255, 0, 128, 128, 128])
PLANES = ("albedo", "f0", "roughness", "normal")


@pytest.fixture(scope="module")
def store_case():
    """a 64 x 64 atlas worth of inputs (4096 texels, 16 workgroups of groups): safe random values, the special values in the first
    texels of every channel, a fifth of the texels unowned (their inputs are NaN: they must not matter); the restated planes"""
    W = 64
    n = W * W
    rng = np.random.default_rng(42)
    face_of = np.where(rng.uniform(size=n) < 0.2, -1, rng.integers(0, 5000, size=n)).astype(np.int32)
    face_of[:len(SPECIAL)] = 7
    inp = dict(albedo=_safe(rng, "albedo", (n, 3), -0.2, 1.2), f0=_safe(rng, "f0", (n, 3), -0.2, 1.2),
               roughness=_safe(rng, "roughness", (n,), -0.2, 1.2), normal=_safe(rng, "normal", (n, 3), -1.2, 1.2))
    for k in PLANES:
        inp[k][:len(SPECIAL)] = SPECIAL[:, None] if inp[k].ndim == 2 else SPECIAL
        inp[k][face_of < 0] = np.nan
    want = store_numpy(face_of, *(inp[k] for k in PLANES))
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    return W, n, face_of, torch.from_numpy(face_of).to(DEV), dev, want


def _store(W, face_of, dev, t0, n, planes):
    sl = slice(t0, t0 + n)
    hip.atlas_store(face_of[sl], *(dev[k][sl] if planes.get(k) is not None else None for k in PLANES), t0, W,
                    albedo_tex=planes.get("albedo"), f0_tex=planes.get("f0"), rough_tex=planes.get("roughness"),
                    normal_tex=planes.get("normal"))
    torch.cuda.synchronize()


def _plane_buffers(W, offset=0):
    """the four planes, each between guards; offset 1: at an odd address (the kernel's byte path)"""
    out = {}
    for k in PLANES:
        c = 1 if k == "roughness" else 3
        buf, mid = _guarded(W * W * c + offset)
        out[k] = (buf, mid[offset:].view(W, W, c) if c > 1 else mid[offset:].view(W, W))
    return out


def test_atlas_store_vs_numpy(store_case):
    W, n, face_np, face_of, dev, want = store_case
    bufs = _plane_buffers(W)
    _store(W, face_of, dev, 0, n, {k: v[1] for k, v in bufs.items()})
    for k in PLANES:
        got = bufs[k][1].cpu().numpy().reshape(want[k].shape)
        assert _guards_intact(bufs[k][0]), k
        assert got[:len(SPECIAL)].reshape(len(SPECIAL), -1)[:, 0].tolist() == SPECIAL_BYTES[k], k           # the stated bytes
        assert np.array_equal(got, want[k]), (k, int((got != want[k]).sum()))
        assert (got[face_np < 0] == np.array(FILL[k], dtype=np.uint8)).all() and (face_np < 0).sum() > n // 10


@pytest.mark.parametrize("offset", [0, 1])
def test_atlas_store_ranges_stay_inside(store_case, offset):
    """[5, n - 7) is a multiple of 4 at neither end; [1001, 1003) lies inside one group of four; bytes outside keep their 0xA5"""
    W, n, face_np, face_of, dev, want = store_case
    for t0, t1 in ((5, n - 7), (1001, 1003), (8, 8)):
        bufs = _plane_buffers(W, offset)
        _store(W, face_of, dev, t0, t1 - t0, {k: v[1] for k, v in bufs.items()})
        for k in PLANES:
            got = bufs[k][1].cpu().numpy().reshape(want[k].shape)
            assert _guards_intact(bufs[k][0]), k
            assert np.array_equal(got[t0:t1], want[k][t0:t1]), (k, t0, t1)
            assert (got[:t0] == 0xA5).all() and (got[t1:] == 0xA5).all(), (k, t0, t1)


def test_atlas_store_skips_null_planes(store_case):
    W, n, face_np, face_of, dev, want = store_case
    for keep in (("roughness",), ("albedo", "normal")):
        bufs = _plane_buffers(W)
        _store(W, face_of, dev, 0, n, {k: bufs[k][1] for k in keep})
        for k in PLANES:
            got = bufs[k][1].cpu().numpy().reshape(want[k].shape)
            assert np.array_equal(got, want[k]) if k in keep else (got == 0xA5).all(), (keep, k)
    with pytest.raises(hip.NmfHipError):                                          # a plane without its input
        hip.atlas_store(face_of, None, None, None, None, 0, W, albedo_tex=_plane_buffers(W)["albedo"][1])
    with pytest.raises(hip.NmfHipError):                                          # a plane of another atlas size
        hip.atlas_store(face_of, dev["albedo"], None, None, None, 0, W, albedo_tex=torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV))


# ---- the bake on the S1 model --------------------------------------------------------------------------------------------------------
SIZE = 256
MARGIN = 2e-5          # what the material tests grant the heads against float64 (test_hip_mesh, test_hip_material_maps)


@pytest.fixture(scope="module")
def s1():
    """the S1 model at grid 32, its mesh, the 256 x 256 bake, and the restated owner / position of every texel"""
    from nmf_amd.mesh import bake_textures, extract_mesh
    nerf, cfg = _s1_model()
    mesh = extract_mesh(nerf)
    tex = bake_textures(nerf, mesh, size=SIZE)
    face_of, pos = atlas_numpy(mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), SIZE, tex.layout[1])
    planes = {k: getattr(tex, k).cpu().numpy().reshape(SIZE * SIZE, -1) for k in PLANES}
    return dict(nerf=nerf, cfg=cfg, mesh=mesh, tex=tex, face_of=face_of, pos=pos, planes=planes)


def test_bake_on_the_s1_model(s1):
    """every byte of the material planes brackets the float64 head formulas at the restated texel positions within the 2e-5 the
    existing material tests grant: Q(x - m) <= q <= Q(x + m); the normal plane IS the quantised rf.compute_normals there"""
    from nmf_amd.mesh import atlas_layout, atlas_uv
    nerf, mesh, tex, face_of, pos, planes = (s1[k] for k in ("nerf", "mesh", "tex", "face_of", "pos", "planes"))
    F = mesh.faces.shape[0]
    assert tex.layout == atlas_layout(F, SIZE) and np.array_equal(tex.uv, atlas_uv(F, tex.layout))
    assert {"bake", "texels", "queries", "store"} <= set(tex.seconds)
    for k in ("albedo", "f0", "normal"):
        assert getattr(tex, k).shape == (SIZE, SIZE, 3) and getattr(tex, k).dtype == torch.uint8
    assert tex.roughness.shape == (SIZE, SIZE) and tex.roughness.dtype == torch.uint8
    own = face_of >= 0
    assert own.sum() > SIZE * SIZE // 2 and (~own).sum() > 0
    p = torch.from_numpy(pos[own]).to(DEV)
    with torch.no_grad():
        app = nerf.rf.compute_appfeature(p)
        nrm = nerf.rf.compute_normals(p)
    albedo, f0, r1 = (v.cpu().numpy() for v in _head_formulas(nerf, app))
    for k, x in (("albedo", albedo), ("f0", f0), ("roughness", r1)):
        q = planes[k][own].reshape(x.shape)
        lo, hi = quantise(k, x - MARGIN, np.float64), quantise(k, x + MARGIN, np.float64)
        print(k, "bytes off the float64 byte:", int((q != quantise(k, x, np.float64)).sum()), "of", q.size,
              "outside the bracket:", int(((q < lo) | (q > hi)).sum()))
        assert ((lo <= q) & (q <= hi)).all(), k
    qn = planes["normal"][own]
    assert np.array_equal(qn, quantise("normal", nrm.cpu().numpy()))
    for k in PLANES:
        assert (planes[k][~own] == np.array(FILL[k], dtype=np.uint8)).all(), k


def test_bake_normals_are_unit_and_point_outward(s1):
    """the decoded normals (q - 128) / 127 have length 1 within sqrt(3) / 127 + 1e-4 (one truncated quantisation step per channel plus
    the 1e-4 the mesh test grants the field's normals) and point away from the cube's centre on the texels away from the cube's edges.

    The S1 cube has half-size 0.75 and the lattice spacing at grid 32 is h = 3 / 31: `more than 4 h from a cube edge` leaves
    (1 - 4 h / 0.75)^2 = 23 % of a face, so it cannot cover over half of the owned texels at this grid, whatever the bake does.  The
    normals are therefore checked on MORE texels: every one further than 1 h from an edge, a superset of the 4 h ones and
    (1 - h / 0.75)^2 = 76 % of a face (2 h would be 55 % of a face, which leaves no room for the bevel triangles along the edges:
    every triangle gets the same number of texels whatever its area).  Over half of the owned texels must qualify; the fractions
    for 1 h .. 4 h are printed."""
    face_of, pos, planes = s1["face_of"], s1["pos"], s1["planes"]
    own = face_of >= 0
    n = (planes["normal"][own].astype(np.float64) - 128.0) / 127.0
    p = pos[own].astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    print("decoded normal length", length.min(), length.max())
    assert np.abs(length - 1).max() <= np.sqrt(3) / 127 + 1e-4
    h = 3.0 / 31
    frac = {k: float(((np.abs(p) < 0.75 - k * h).sum(axis=1) == 2).mean()) for k in (1, 2, 3, 4)}
    away = (np.abs(p) < 0.75 - 1 * h).sum(axis=1) == 2
    dots = (n * p).sum(axis=1)
    print("owned texels further than k h from a cube edge:", frac, "min n.p there (k = 1)", dots[away].min())
    assert away.sum() > own.sum() // 2
    assert (dots[away] > 0).all()


def test_bake_is_deterministic_and_independent_of_chunk(s1):
    from nmf_amd.mesh import bake_textures
    nerf, mesh, tex = s1["nerf"], s1["mesh"], s1["tex"]
    for kw in (dict(), dict(chunk=1000)):
        again = bake_textures(nerf, mesh, size=SIZE, **kw)
        for k in PLANES:
            assert torch.equal(getattr(again, k), getattr(tex, k)), (kw, k)


def test_bake_carries_material_edits(s1):
    """albedo=1,0,0 in a box over the cube's +++ corner: the owned texels inside are the bytes of albedo (1, 0, 0) -- (254, 0, 0):
    srgb(1) is 1.055f - 0.055f = 1 - 2^-24 in fp32 and the cast truncates, as mesh.albedo_to_8bit gives a PLY vertex --, texels
    well outside keep their bytes, and f0 / roughness / normals are untouched everywhere"""
    from nmf_amd import edit as E
    from nmf_amd.mesh import bake_textures
    nerf, mesh, tex, face_of, pos = (s1[k] for k in ("nerf", "mesh", "tex", "face_of", "pos"))
    c, half = np.array([0.75, 0.75, 0.75]), np.array([0.4, 0.4, 0.4])
    assert E.parse_spec("albedo=1,0,0@box(0.75,0.75,0.75,0.4,0.4,0.4)").region.kind == "box"
    nerf.set_material_edits([E.parse_spec("albedo=1,0,0@box(0.75,0.75,0.75,0.4,0.4,0.4)")])
    try:
        edited = bake_textures(nerf, mesh, size=SIZE)
    finally:
        nerf.set_material_edits(None)
    own = face_of >= 0
    d = np.abs(pos.astype(np.float64) - c) - half
    inside, outside = own & (d.max(axis=1) < -1e-3), own & (d.max(axis=1) > 1e-3)
    assert inside.sum() > 500 and outside.sum() > 10000
    red = quantise("albedo", np.array([1.0, 0.0, 0.0], dtype=np.float32))
    assert red.tolist() == [254, 0, 0]
    a0, a1 = tex.albedo.cpu().numpy().reshape(-1, 3), edited.albedo.cpu().numpy().reshape(-1, 3)
    assert (a1[inside] == red).all() and np.array_equal(a1[outside], a0[outside]) and (a0[inside] != red).any()
    for k in ("f0", "roughness", "normal"):
        assert torch.equal(getattr(edited, k), getattr(tex, k)), k


def test_bake_of_a_reference_spacing_mesh_uses_the_aligned_positions(s1):
    from nmf_amd.mesh import bake_textures, extract_mesh
    nerf, tex = s1["nerf"], s1["tex"]
    ref = extract_mesh(nerf, reference_spacing=True)
    assert ref.aligned_verts is not None and torch.equal(ref.aligned_verts, s1["mesh"].verts) and s1["mesh"].aligned_verts is None
    shifted = bake_textures(nerf, ref, size=SIZE)
    for k in PLANES:
        assert torch.equal(getattr(shifted, k), getattr(tex, k)), k
    with pytest.raises(ValueError, match="--texture-size"):
        bake_textures(nerf, ref, size=64)


def test_export_mesh_command_line_with_textures(s1, tmp_path, capsys):
    from PIL import Image
    from nmf_amd import export_mesh
    from nmf_amd.mesh import atlas_layout
    nerf, cfg, mesh = s1["nerf"], s1["cfg"], s1["mesh"]
    V, F = mesh.verts.shape[0], mesh.faces.shape[0]
    ck = str(tmp_path / "s1.th")
    nerf.save(ck, cfg["arch"])
    capsys.readouterr()
    rec = export_mesh.main(["--ckpt", ck, "--resolution", "32", "--texture-size", "256"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    names = ["s1.mtl", "s1.obj", "s1_albedo.png", "s1_f0.png", "s1_normal.png", "s1_roughness.png"]
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["s1.th"])
    assert line == rec and rec["output"] == str(tmp_path / "s1.obj") and (rec["V"], rec["F"]) == (V, F)
    assert rec["texture_size"] == 256 and rec["texels_per_square"] == atlas_layout(F, 256)[1]
    assert set(rec["seconds"]) == {"density", "triangulate", "attributes", "bake", "write"}
    obj = parse_obj(rec["output"])
    assert (len(obj["v"]), len(obj["vn"]), len(obj["vt"]), len(obj["f"])) == (V, V, 3 * F, F)
    assert np.array_equal(np.array(obj["f"])[:, :, 0] - 1, mesh.faces.cpu().numpy())
    assert np.array_equal(np.array(obj["v"], dtype=np.float32), mesh.verts.cpu().numpy())
    for m in PLANES:
        img = Image.open(tmp_path / f"s1_{m}.png")
        assert img.size == (256, 256) and np.array_equal(np.asarray(img).reshape(256 * 256, -1), s1["planes"][m])
    with pytest.raises(SystemExit) as e:
        export_mesh.main(["--ckpt", ck, "--no-attributes", "--texture-size", "256"])
    assert e.value.code == 2                                                      # an argument error
    with pytest.raises(SystemExit):
        export_mesh.main(["--ckpt", ck, "--texture-size", "3"])
    rec = export_mesh.main(["--ckpt", ck, "--resolution", "32"])                  # without --texture-size: the PLY, as before
    assert rec["output"] == str(tmp_path / "s1.ply") and os.path.exists(rec["output"]) and "texture_size" not in rec
    assert set(rec["seconds"]) == {"density", "triangulate", "attributes", "write"}
