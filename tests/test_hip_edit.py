"""Material edits on the GPU: nmf_heads_edit bit for bit against the float32 restatement of nmf_amd/edit.py, nmf_material_maps_edit
against nmf_material_maps (no edits) and a float64 restatement (edits), the fused evaluation pass with edits at every recursion level
(identity and empty-region edits keep every bit; set / zero / half-space edits do what they say), the module path with the same
edits, the refusal of training calls, and the render / export_mesh command lines."""
import contextlib
import types

import numpy as np
import pytest
import torch

from conftest import Golden, assert_close
from nmf_amd import edit as E
from nmf_amd import hip
from test_hip_e2e import DEV, _fixture_rays, _full_size_model, _pin_reference_bookkeeping, _small_fused_model
from test_hip_material_maps import MAPS, _fused, _restate
from test_hip_metrics import _s1_model, _tiny_scene
from test_mesh_cpu import read_ply

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- nmf_heads_edit ------------------------------------------------------------------------------------------------------------
REGIONS = dict(all=E.Region.all(), box=E.Region.box((0.1, -0.2, 0.3), (0.6, 0.45, 0.7)),
               ellipsoid=E.Region.ellipsoid((-0.2, 0.1, 0.0), (0.9, 0.5, 0.7)))


def _single_edits():
    """all three regions x hard / soft x invert x all three targets, an operator with every entry in use"""
    A = np.array([[0.5, 0.25, -0.125], [0.1, 0.7, 0.3], [-0.2, 0.4, 0.9]])
    out = []
    for target in E.TARGETS:
        for region in REGIONS.values():
            for falloff in (0.0, 0.3):
                for invert in (False, True):
                    out.append(E.MaterialEdit(target, A if target != "roughness" else 1.5 * np.eye(3), (0.05, -0.1, 0.2), region, falloff, invert))
    return out


def _heads_and_positions(n, seed):
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.01, 1.0, (n, 11)).astype(np.float32)
    x = rng.uniform(-1.5, 1.5, (n, 4)).astype(np.float32)
    return h, x


def _run_heads_edit(h, x, stride, table):
    """-> the edited rows, with guard rows in front of and behind the buffer checked"""
    n, G = h.shape[0], 3
    guard = np.float32(-7.25)
    buf = torch.full((n + 2 * G, 11), float(guard), device=DEV)
    buf[G:G + n] = torch.from_numpy(h).to(DEV)
    rows = buf[G:G + n]
    assert rows.is_contiguous()
    xyz = torch.from_numpy(np.ascontiguousarray(x[:, :stride])).to(DEV)
    got = hip.heads_edit(rows, xyz, table)
    assert got.data_ptr() == rows.data_ptr()
    torch.cuda.synchronize()
    assert bool((buf[:G] == float(guard)).all()) and bool((buf[G + n:] == float(guard)).all()), "guard rows were written"
    return rows.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_heads_edit_is_bit_identical_to_the_float32_restatement(n):
    h, x = _heads_and_positions(n, 100 + n)
    singles = _single_edits()
    assert len(singles) == 36
    rng = np.random.default_rng(n)
    # K = 16: chained edits (every target several times, each on the result of the one before), three lists
    chains = [[singles[i] for i in rng.permutation(36)[:16]] for _ in range(3)]
    chains.append([E.MaterialEdit.scale("albedo", 0.5), E.MaterialEdit.add("albedo", 0.75)] * 8)
    changed = 0
    for stride in (3, 4):
        for edits in [[e] for e in singles] + chains:
            table = E.pack(edits, "cpu")
            assert table.shape[0] in (1, 16)
            want = E.apply_reference(h, x[:, :3], table, np.float32)
            got = _run_heads_edit(h, x, stride, table)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, stride, [e.target for e in edits], edits[0].region.kind)
            changed += int((want != h).any())
    assert changed >= 12                     # the edits do something (a single row may miss every region but `all`)
    # a device table is accepted as well (copied back once)
    got = _run_heads_edit(h, x, 4, E.pack(chains[0], DEV))
    assert np.array_equal(got.view(np.uint32), E.apply_reference(h, x, chains[0], np.float32).view(np.uint32))


def test_heads_edit_identity_and_nothing_to_do():
    h, x = _heads_and_positions(1000, 5)
    ident = [E.MaterialEdit(t, region=r, falloff=f) for t in E.TARGETS for r in REGIONS.values() for f in (0.0, 0.25)][:16]
    assert np.array_equal(_run_heads_edit(h, x, 4, E.pack(ident)).view(np.uint32), h.view(np.uint32))
    one = E.pack([E.MaterialEdit.set("albedo", 0.5)])
    assert np.array_equal(_run_heads_edit(h, x, 3, None).view(np.uint32), h.view(np.uint32))                 # K = 0
    assert np.array_equal(_run_heads_edit(h, x, 3, E.pack([])).view(np.uint32), h.view(np.uint32))
    assert _run_heads_edit(h[:0], x[:0], 4, one).shape == (0, 11)                                            # n = 0
    hip.HOST_EXT.kernel_timing_begin("", False)
    try:
        hip.heads_edit(torch.zeros(0, 11, device=DEV), torch.zeros(0, 4, device=DEV), one)
        hip.heads_edit(torch.zeros(8, 11, device=DEV), torch.zeros(8, 4, device=DEV), None)
    finally:
        launches = hip.HOST_EXT.kernel_timing_end()
    assert not launches, launches
    with pytest.raises(hip.NmfHipError, match="half extents"):
        bad = one.clone()
        bad[0, 0], bad[0, 7] = 1.0, 0.0
        hip.heads_edit(torch.zeros(8, 11, device=DEV), torch.zeros(8, 4, device=DEV), bad)


# ---- nmf_material_maps_edit ------------------------------------------------------------------------------------------------------
def _maps_case(B, per_ray, seed, lattice=False):
    """synthetic inputs of the maps: B rays with about per_ray samples each, one ray without samples, some samples with w == 0, a bounce
    row for every third sample"""
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(max(per_ray // 2, 1), per_ray * 3 // 2 + 2, (B,), generator=g)
    cnt[B // 2] = 0
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
    M = int(offsets[-1])
    u = lambda *s: torch.rand(*s, generator=g)                                                    # noqa: E731
    app = u(M, 24) * 2 - 1
    n = torch.nn.functional.normalize(u(M, 3) * 2 - 1, dim=-1)
    w = u(M) / max(per_ray, 1)
    w[::7] = 0.0
    d = torch.nn.functional.normalize(u(B, 3) * 2 - 1, dim=-1)
    rays = torch.cat([u(B, 3), d], -1)
    has = torch.zeros(M, dtype=torch.bool)
    has[::3] = True
    Mb = int(has.sum())
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[has] = torch.arange(Mb, dtype=torch.int32)
    rc = torch.randint(0, 4, (Mb,), generator=g)
    row_off = torch.cat([torch.zeros(1, dtype=torch.int64), rc.cumsum(0)])
    R = int(row_off[-1])
    ray_id = torch.repeat_interleave(torch.arange(B), cnt)
    acc = torch.zeros(B).index_add_(0, ray_id, w)
    xyzt = torch.cat([(torch.randint(-12, 13, (M, 3), generator=g) / 8.0) if lattice else (u(M, 3) * 3 - 1.5), u(M, 1)], -1)
    c = dict(app=app, normals=n, weight=w, offsets=offsets, rays=rays, head_W=u(11, 24) - 0.5, head_b=u(11) - 0.5, conv=u(9, 3),
             acc=acc, bg=torch.ones(3), inv=inv, row_off=row_off, cnt=rc.int(), incoming=u(R, 3), brdf_weight=u(R, 3), xyzt=xyzt)
    return {k: v.to(DEV).contiguous() for k, v in c.items()}, (1.3, -0.2, 0.1, -0.4, 0.3)


def _maps(c, hp, **kw):
    return hip.material_maps(c["app"], c["normals"], c["weight"], c["offsets"], c["rays"], c["head_W"], c["head_b"], hp, c["conv"], c["acc"],
                             c["bg"], c["inv"], c["row_off"], c["cnt"], c["incoming"], c["brdf_weight"], **kw)


def _restate_edit(c, hp, edits):
    """test_hip_material_maps._restate with the edits applied to the heads (apply_reference in float64): the maps in float64"""
    d = lambda k: c[k].double()                                                  # noqa: E731
    app, n, w, offsets, rays = d("app"), d("normals"), d("weight"), c["offsets"].long(), d("rays")
    a = app @ d("head_W").T + d("head_b")
    dm, db, tb, fb, rb = hp
    heads = torch.cat([torch.sigmoid(dm * a[:, 0:3] + db).clip(0, 1), torch.sigmoid(a[:, 3:6] + tb), torch.sigmoid(a[:, 6:9] + fb),
                       (torch.sigmoid(a[:, 9:11] + rb) * 0.5).clip(1e-2, 1)], 1)
    if edits is not None:
        heads = torch.from_numpy(E.apply_reference(heads.cpu().numpy(), c["xyzt"].double().cpu().numpy(), edits, np.float64)).to(app.device)
    albedo, f0, r1 = heads[:, 0:3], heads[:, 6:9], heads[:, 9:10]
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    Y = torch.stack([torch.full_like(x, 0.28209479177387814), 0.4886025119029199 * y, 0.4886025119029199 * z,
                     0.4886025119029199 * x, 1.0925484305920792 * x * y, 1.0925484305920792 * y * z,
                     0.31539156525252005 * (3 * z * z - 1), 1.0925484305920792 * x * z, 0.5462742152960396 * (x * x - y * y)], 1)
    En = Y @ d("conv").reshape(9, 3)
    inv, row_off, cnt = c["inv"].long(), c["row_off"].long(), c["cnt"].long()
    M, B, Mb = app.shape[0], offsets.shape[0] - 1, row_off.shape[0] - 1
    ray_id = torch.repeat_interleave(torch.arange(B, device=app.device), offsets[1:] - offsets[:-1])
    cos_t = (-rays[ray_id, 3:6] * n).sum(-1, keepdim=True).abs()
    Fr = f0 + (1 - f0) * (1 - cos_t).clip(0, 1) ** 5
    row_of_ray = torch.repeat_interleave(torch.arange(Mb, device=app.device), row_off[1:] - row_off[:-1])
    ec = cnt.double().clip(min=1)[row_of_ray][:, None]
    z3 = lambda: torch.zeros(Mb, 3, dtype=torch.float64, device=app.device)      # noqa: E731
    spec_rows, brdf_rows = z3().index_add_(0, row_of_ray, d("incoming") / ec), z3().index_add_(0, row_of_ray, d("brdf_weight") / ec)
    has = inv >= 0
    spec = torch.zeros(M, 3, dtype=torch.float64, device=app.device)
    brgb = torch.zeros_like(spec)
    spec[has], brgb[has] = spec_rows[inv[has]], brdf_rows[inv[has]]
    per = dict(albedo=albedo, roughness=r1.expand(-1, 3), diffuse=(1 - Fr) * albedo * En, tint=Fr * brgb, spec=spec)
    return {k: torch.zeros(B, 3, dtype=torch.float64, device=app.device).index_add_(0, ray_id, w[:, None] * X) + (1 - d("acc"))[:, None]
            for k, X in per.items()}


WIDTHS = [(3, 200), (40, 20), (100, 3)]          # lane groups of 64, 16 and 8 (mean samples per ray >= 64, >= 16, below)


@pytest.mark.parametrize("B,per_ray", WIDTHS)
def test_material_maps_edit_without_edits_has_the_bits_of_material_maps(B, per_ray):
    c, hp = _maps_case(B, per_ray, seed=B)
    avg = c["app"].shape[0] // B
    assert (avg >= 64) if per_ray == 200 else ((16 <= avg < 64) if per_ray == 20 else avg < 16)
    assert int((c["offsets"][1:] == c["offsets"][:-1]).sum()) >= 1 and int((c["weight"] == 0).sum()) >= 1
    old = _maps(c, hp)
    for kw in (dict(xyz=c["xyzt"], edits=None), dict(xyz=c["xyzt"], edits=E.pack([])), dict(xyz=c["xyzt"][:, :3].contiguous())):
        assert _same_bits(_maps(c, hp, **kw), old), kw.keys()
    # an identity edit takes the kernel with the edit in it: another instantiation, whose compiler may fuse the products and sums
    # of the SH bases (nmf_rows::sh9, not pinned) differently -- the same values to a few float32 roundings
    ident = E.pack([E.MaterialEdit(t, region=E.Region.box((0, 0, 0), (1, 1, 1)), falloff=0.25) for t in E.TARGETS])
    assert_close(_maps(c, hp, xyz=c["xyzt"], edits=ident).cpu(), old.cpu(), rtol=1e-6, atol=1e-6, what="identity edit")
    with pytest.raises(hip.NmfHipError, match="positions"):
        _maps(c, hp, edits=ident)


@pytest.mark.parametrize("B,per_ray", WIDTHS)
def test_material_maps_edit_against_the_float64_restatement(B, per_ray):
    """hard masks on lattice positions k / 8 with boundaries off the lattice (no sample can change sides in float32), soft ones too"""
    c, hp = _maps_case(B, per_ray, seed=10 + B, lattice=True)
    plain = _restate_edit(c, hp, None)
    tr = dict(mm_app0=c["app"], mm_normals0=c["normals"], mm_w0=c["weight"], mm_offsets0=c["offsets"], mm_rays0=c["rays"], mm_inv0=c["inv"],
              mm_row_off0=c["row_off"], mm_cnt0=c["cnt"], mm_incoming0=c["incoming"], mm_brdf0=c["brdf_weight"], mm_conv0=c["conv"],
              mm_acc0=c["acc"])
    ref = _restate(tr, types.SimpleNamespace(head_W=c["head_W"], head_b=c["head_b"], head_p=hp))
    for k in MAPS:                                       # the restatement of this file is the one of test_hip_material_maps.py
        assert_close(plain[k].cpu(), ref[k].cpu(), rtol=1e-12, atol=1e-12, what=k)
    edits = [E.MaterialEdit.set("albedo", (0.6, 0.05, 0.05), E.Region.box((0.5, 0, 0), (0.5625, 1.0625, 0.8125))),
             E.MaterialEdit.scale("roughness", 0.4, E.Region.sphere((0, 0, 0), 0.9), falloff=0.25),
             E.MaterialEdit.hue("albedo", 40.0, E.Region.ellipsoid((0, 0.25, 0), (1.03, 0.77, 0.51)), invert=True),
             E.MaterialEdit.add("f0", (0.2, -0.1, 0.05), E.Region.box((-0.5, 0, 0), (0.4375, 2, 2)), falloff=0.125),
             E.MaterialEdit.saturation("f0", 0.3)]
    tab = E.pack_numpy(edits).astype(np.float64)
    p = c["xyzt"][:, :3].double().cpu().numpy()
    for e, row in zip(edits, tab):
        if e.falloff == 0 and e.region.kind != "all":
            q = p - row[4:7]
            dd = (np.abs(q) - row[7:10]).max(1) if e.region.kind == "box" else (np.sqrt(((q / row[7:10]) ** 2).sum(1)) - 1) * row[7:10].min()
            assert np.abs(dd).min() > 1e-4 and (dd < 0).any() and (dd > 0).any()
    want = _restate_edit(c, hp, edits)
    got = _maps(c, hp, xyz=c["xyzt"], edits=E.pack(edits))
    got3 = _maps(c, hp, xyz=c["xyzt"][:, :3].contiguous(), edits=E.pack(edits, DEV))
    assert _same_bits(got, got3)
    for i, k in enumerate(MAPS):
        assert_close(got[:, 3 * i:3 * i + 3].cpu(), want[k].float().cpu(), rtol=1e-5, atol=2e-5, what=k)
    for k in ("albedo", "roughness", "diffuse", "tint"):
        assert float((want[k] - plain[k]).abs().max()) > 1e-3, k
    assert_close(want["spec"].cpu(), plain["spec"].cpu(), rtol=0, atol=0, what="spec does not read the heads")


# ---- the fused evaluation pass -----------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _edits(nerf, edits):
    nerf.set_material_edits(edits)
    try:
        yield
    finally:
        nerf.set_material_edits(None)


@pytest.fixture(scope="module")
def full():
    """the e2e_full_eval model, its fused pass, the fixture's rays and ONE unedited render (DeviceNoise, seed 5) every test compares to"""
    from nmf_amd.noise import DeviceNoise
    g = Golden("e2e_full_eval")
    nerf = _full_size_model(g)
    fp = _fused(nerf)
    rays, focal = _fixture_rays(g)
    rays = rays.to(DEV)

    def run(edits=None, noise=None):
        with _edits(nerf, edits):
            out = fp.render_chunk(rays, focal, noise or DeviceNoise(torch.device(DEV), seed=5), want_maps=True, want_materials=True,
                                  want_linear=True)
        return dict(rgb_map=out[0], acc_map=out[1], kept=out[2], n_samples=out[3], depth=out[4], world_normal=out[5], rgb_lin=out[7],
                    **out[6])
    return types.SimpleNamespace(g=g, nerf=nerf, fp=fp, rays=rays, focal=focal, run=run, base=run())


IMAGES = ("rgb_map", "acc_map", "depth", "world_normal", "rgb_lin") + MAPS


def test_fused_pass_identity_and_empty_region_edits_keep_every_bit(full):
    """an identity edit over `all` takes the unfused route (heads, edit, row preparation) at every level and the edit kernel of the
    maps; a box outside the aabb leaves every sample alone: all images bit-identical to the render without edits"""
    base = full.base
    assert full.fp.core().n_material_edits() == 0
    outside = E.MaterialEdit.set("albedo", (1, 0, 0), E.Region.box((9, 9, 9), (1, 1, 1)))
    assert float(full.nerf.sampler.aabb.abs().max()) < 7
    for name, edits in (("identity", [E.MaterialEdit(t) for t in E.TARGETS]), ("outside", [outside]),
                        ("outside soft", [E.MaterialEdit.scale("roughness", 0.1, E.Region.sphere((9, 9, 9), 1.0), falloff=0.5)])):
        calls = hip.HOST_EXT.call_timing_begin("")
        try:
            got = full.run(edits)
        finally:
            calls = hip.HOST_EXT.call_timing_end()
        assert calls.get("heads_edit", (0, 0))[1] >= 2 and "heads_fwd" in calls, (name, sorted(calls))      # both levels, unfused
        assert got["kept"] == base["kept"] and got["n_samples"] == base["n_samples"]
        for k in IMAGES:
            assert _same_bits(got[k], base[k]), (name, k)
    again = full.run()                                    # and without edits the pass is what it was
    assert full.fp.core().n_material_edits() == 0
    for k in IMAGES:
        assert _same_bits(again[k], base[k]), k


def test_fused_pass_albedo_and_roughness_edits(full):
    base = full.base
    acc = base["acc_map"].double()[:, None]
    k3 = torch.tensor([0.6, 0.05, 0.05], dtype=torch.float64, device=DEV)
    # albedo = k over all: the albedo map is k acc + (1 - acc) bg (white); roughness, acc and depth keep their bits
    got = full.run([E.MaterialEdit.set("albedo", (0.6, 0.05, 0.05))])
    assert_close(got["albedo"].cpu(), (k3 * acc + (1 - acc)).float().cpu(), rtol=0, atol=2e-5, what="albedo = k")
    for k in ("roughness", "acc_map", "depth"):
        assert _same_bits(got[k], base[k]), k
    assert float((got["rgb_map"] - base["rgb_map"]).abs().max()) > 1e-3
    # albedo = 0 over all: no diffuse light; the specular part is the same draw, so nothing gets brighter
    got = full.run([E.MaterialEdit.set("albedo", 0.0)])
    assert_close(got["diffuse"].cpu(), (1 - acc).expand(-1, 3).float().cpu(), rtol=0, atol=2e-5, what="diffuse without albedo")
    lin, lin0 = got["rgb_lin"], base["rgb_lin"]
    print("albedo = 0: max rgb_lin increase", float((lin - lin0).max()))
    assert bool((lin <= lin0 + 1e-5).all())
    solid = base["acc_map"] > 0.5
    darker = ((lin < lin0).any(dim=1) & solid).sum()
    print("albedo = 0: rays with acc > 0.5:", int(solid.sum()), "strictly darker:", int(darker))
    assert int(solid.sum()) > 100 and int(darker) >= 0.1 * int(solid.sum())
    # roughness = 0.3 over all: the map is 0.3 acc + (1 - acc), and the lobe and the MLP see it
    got = full.run([E.MaterialEdit.set("roughness", 0.3)])
    assert_close(got["roughness"].cpu(), (0.3 * acc + (1 - acc)).expand(-1, 3).float().cpu(), rtol=0, atol=2e-5, what="roughness = 0.3")
    assert float((got["rgb_map"] - base["rgb_map"]).abs().max()) > 1e-3
    for k in ("albedo", "acc_map", "depth"):
        assert _same_bits(got[k], base[k]), k


def test_fused_pass_half_space_edit_against_the_float64_restatement(full):
    """a box over the half x > 0 of the object (soft edge: no sample can change sides between float32 and float64): the albedo map
    equals the float64 restatement over the recorded samples (mm_xyzt0); rays whose samples all lie outside keep their bits"""
    from nmf_amd.noise import ReplayNoise
    g, nerf, fp = full.g, full.nerf, full.fp
    edit = E.MaterialEdit.set("albedo", (0.05, 0.1, 0.8), E.Region.box((1.5, 0, 0), (1.5, 4, 4)), falloff=0.1)
    outs = {}
    for name, edits in (("plain", None), ("edit", [edit])):
        pins = _pin_reference_bookkeeping(g)
        torch.manual_seed(g["noise_seed"])
        with _edits(nerf, edits):
            out = fp.render_chunk(full.rays, full.focal, ReplayNoise(DEV, None, pins=pins), want_maps=True, want_materials=True)
        outs[name] = (out[-1], pins.trace)
    maps, tr = outs["edit"]
    assert "mm_xyzt0" in tr and tr["mm_xyzt0"].shape == (tr["mm_app0"].shape[0], 4)
    core = fp.core()
    c = dict(app=tr["mm_app0"], normals=tr["mm_normals0"], weight=tr["mm_w0"], offsets=tr["mm_offsets0"], rays=tr["mm_rays0"],
             head_W=core.head_W.reshape(11, 24), head_b=core.head_b.reshape(11), conv=tr["mm_conv0"], acc=tr["mm_acc0"], inv=tr["mm_inv0"],
             row_off=tr["mm_row_off0"], cnt=tr["mm_cnt0"], incoming=tr["mm_incoming0"], brdf_weight=tr["mm_brdf0"], xyzt=tr["mm_xyzt0"])
    want = _restate_edit(c, tuple(core.head_p), [edit])
    for k in ("albedo", "roughness", "diffuse"):
        assert_close(maps[k].cpu(), want[k].float().cpu(), rtol=1e-5, atol=2e-5, what=k + " (float64 restatement)")
    x = tr["mm_xyzt0"][:, 0].double()
    offsets = tr["mm_offsets0"].long()
    B = offsets.shape[0] - 1
    ray_id = torch.repeat_interleave(torch.arange(B, device=x.device), offsets[1:] - offsets[:-1])
    far = torch.ones(B, dtype=torch.bool, device=x.device)
    far[ray_id[x > -0.1 - 1e-4]] = False                  # d = -x here; the mask is 0 for d >= falloff
    touched = torch.zeros(B, dtype=torch.bool, device=x.device)
    touched[ray_id[x > 0]] = True
    assert int(far.sum()) > 50 and int(touched.sum()) > 50
    plain = outs["plain"][0]
    assert _same_bits(maps["albedo"][far], plain["albedo"][far])
    assert float((maps["albedo"][touched] - plain["albedo"][touched]).abs().max()) > 0.05


def test_fused_pass_agrees_with_the_module_path_under_the_same_edits(full):
    """the module path evaluates the heads densely at every level and edits them there (shade_compact, Shaded.debug); a chunk that
    falls back to it inside one image shows no seam"""
    from nmf_amd.fast_step import Unsupported
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.renderer import render_images
    nerf, fp, rays, focal = full.nerf, full.fp, full.rays, full.focal
    edits = [E.MaterialEdit.set("albedo", (0.6, 0.05, 0.05), E.Region.box((0.75, 0, 0), (0.75, 4, 4)), falloff=0.1),
             E.MaterialEdit.scale("roughness", 0.4), E.MaterialEdit.add("f0", 0.3, E.Region.sphere((0, 0, 0), 0.8), invert=True)]
    fused = full.run(edits)
    with _edits(nerf, edits):
        mod = render_images(nerf, rays, focal, 4096, DeviceNoise(torch.device(DEV), seed=5), keys=MAPS, draw_debug=True)
        for k in ("albedo", "roughness", "diffuse"):
            assert_close(fused[k].cpu(), mod[k].cpu(), rtol=1e-5, atol=1e-5, what=k + " (module path)")
            assert float((fused[k] - full.base[k]).abs().max()) > 1e-2, k
        # one image, four chunks, the second one forced through the fallback
        n = rays.shape[0]
        chunk = (n + 3) // 4
        keys = ("rgb_map",) + MAPS
        whole = render_images(nerf, rays, focal, chunk, DeviceNoise(torch.device(DEV), seed=9), keys=keys)
        orig, calls = fp.render_chunk, []

        def second_falls_back(*a, **k):
            calls.append(a[0])
            if len(calls) == 2:
                raise Unsupported("forced by the test")
            return orig(*a, **k)
        fp.render_chunk = second_falls_back
        try:
            seam = render_images(nerf, rays, focal, chunk, DeviceNoise(torch.device(DEV), seed=9), keys=keys)
        finally:
            fp.render_chunk = orig
        sl = slice(chunk, 2 * chunk)
        assert len(calls) >= 4 and torch.equal(calls[1], rays[sl])          # the forced call was the second quarter of the image
        assert_close(seam["albedo"][sl].cpu(), whole["albedo"][sl].cpu(), rtol=0, atol=1e-5, what="albedo across the seam")
        assert_close(seam["roughness"][sl].cpu(), whole["roughness"][sl].cpu(), rtol=0, atol=1e-5, what="roughness across the seam")
        assert _same_bits(seam["albedo"][:chunk], whole["albedo"][:chunk])


# ---- training refuses edits ----------------------------------------------------------------------------------------------------------
def test_training_calls_refuse_edits_and_are_unchanged_afterwards():
    from nmf_amd.config import resolved_config
    from nmf_amd.noise import DeviceNoise
    from nmf_amd.trainer import Trainer
    grads = {}
    for mode in ("never", "cleared"):
        nerf, rays, focal = _small_fused_model()
        tr = Trainer(nerf, resolved_config()["params"])
        tr.optimizer.step = lambda: None
        gt = torch.rand(64, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
        if mode == "cleared":
            nerf.set_material_edits([E.MaterialEdit.scale("roughness", 0.4)])
            with pytest.raises(ValueError, match="material edits"):
                tr.step(rays, gt, focal, noise=DeviceNoise(DEV, 1), update_controllers=False, fixed_chunk=64)
            with pytest.raises(ValueError, match="material edits"):
                nerf(rays, focal, bg_col=torch.ones(3), is_train=True, ndc_ray=False, noise=DeviceNoise(DEV, 1))
            # the core itself refuses too (a caller that goes around the module)
            tr.fast._core_sync(rays.device, focal, True)
            assert tr.fast.core().n_material_edits() == 1
            with pytest.raises(ValueError, match="material edits"):
                tr.fast.core().train_forward(rays, float(focal), DeviceNoise(DEV, 1))
            nerf.set_material_edits(None)
        out = tr.step(rays, gt, focal, noise=DeviceNoise(DEV, 1), update_controllers=False, fixed_chunk=64)
        assert out["rays"] > 0 and np.isfinite(out["loss"]) and tr.fast.core().n_material_edits() == 0
        grads[mode] = ({k: p.grad.detach().clone() for k, p in nerf.named_parameters() if p.grad is not None}, out["loss"])
        assert nerf.operator_graph_forwards == 0
    (ref, loss_ref), (got, loss_got) = grads["never"], grads["cleared"]
    assert set(ref) == set(got) and len(ref) > 5
    assert loss_got == pytest.approx(loss_ref, rel=2e-5)
    for k, a in ref.items():                               # (the tolerance of the step comparisons of test_hip_e2e.py)
        rel = float((a.double() - got[k].double()).norm() / a.double().norm().clip(min=1e-30))
        assert rel <= 2e-5, (k, rel)


# ---- command lines -------------------------------------------------------------------------------------------------------------------
def test_render_command_line_with_edits(tmp_path, capsys, monkeypatch):
    from PIL import Image
    from nmf_amd import render as R
    from nmf_amd import train as T
    from nmf_amd.dataLoader import BlenderDataset
    from nmf_amd.modules.tensor_nerf import TensorNeRF
    from nmf_amd.renderer import map_to_8bit, render_images
    scene = tmp_path / "tiny"
    _tiny_scene(scene)
    monkeypatch.chdir(tmp_path)
    ck = str(tmp_path / "out.th")
    T.main(["--datadir", str(scene), "--near-far", "2.5", "7", "--iters", "3", "--grid", "16", "--bg", "16", "--eval-every", "3",
            "--test-views", "1", "--save", ck])
    ev = tmp_path / "ev"
    rec = R.main(["--ckpt", ck, "--datadir", str(scene), "--eval-dir", str(ev), "--material-maps", "--edit", "albedo=0.6,0.05,0.05"])
    assert np.isfinite(rec["psnr"])
    ds = BlenderDataset(str(scene), split="test", is_stack=True, N_vis=-1)
    nerf = TensorNeRF.load(ck, near_far=list(ds.near_far), device=DEV)
    nerf.eval()
    k3 = np.array([0.6, 0.05, 0.05])
    for i in range(3):
        acc = render_images(nerf, ds.all_rays[i].to(DEV), float(ds.fx), keys=("rgb_map", "acc_map"))["acc_map"]
        acc = acc.reshape(16, 16, 1).double().cpu().numpy()
        f = k3 * acc + (1 - acc)                                       # k acc + (1 - acc) bg, known to atol 2e-5 (the fused test above)
        png = np.asarray(Image.open(ev / "albedo" / f"{i:03d}.png")).astype(np.int64)
        lo, hi = map_to_8bit(f - 2e-5).astype(np.int64), map_to_8bit(f + 2e-5).astype(np.int64)
        assert png.shape == (16, 16, 3) and bool(((png >= lo) & (png <= hi)).all()), i
    # a camera path: runs with an edit and differs from the unedited frames
    base = ["--ckpt", ck, "--views", "1", "--res", "16", "--path", "orbit", "--frames", "2"]
    R.main(base + ["--out", str(tmp_path / "p0")])
    R.main(base + ["--out", str(tmp_path / "p1"), "--edit", "roughness*0.4"])
    R.main(base + ["--out", str(tmp_path / "p2"), "--edit", "roughness*1"])                    # an identity edit: the same bytes
    frames = lambda d: [np.asarray(Image.open(tmp_path / d / "path" / f"{k:03d}.png")) for k in range(2)]      # noqa: E731
    f0, f1, f2 = frames("p0"), frames("p1"), frames("p2")
    assert all(np.array_equal(a, b) for a, b in zip(f0, f2))
    assert any(not np.array_equal(a, b) for a, b in zip(f0, f1))
    capsys.readouterr()


def test_export_mesh_command_line_with_a_box_edit(tmp_path, capsys):
    from nmf_amd import export_mesh
    nerf, cfg = _s1_model(grid=32)
    ck = str(tmp_path / "s1.th")
    nerf.save(ck, cfg["arch"])
    export_mesh.main(["--ckpt", ck, "--output", str(tmp_path / "a.ply")])
    export_mesh.main(["--ckpt", ck, "--output", str(tmp_path / "b.ply"), "--edit", "albedo=0.9,0.1,0.1@box(0.75,0,0,0.4,2,2)~0.1",
                      "--edit", "roughness=0.05@box(0.75,0,0,0.4,2,2)~0.1"])
    _, va, fa = read_ply(tmp_path / "a.ply")
    _, vb, fb = read_ply(tmp_path / "b.ply")
    assert len(va) == len(vb) > 100 and np.array_equal(fa["vertex_indices"], fb["vertex_indices"])
    for k in ("x", "y", "z", "nx", "ny", "nz", "f0_r", "f0_g", "f0_b"):
        assert np.array_equal(va[k], vb[k]), k
    x = va["x"].astype(np.float64)
    inside, outside = x > 0.35 + 1e-3, x < 0.35 - 0.1 - 1e-3               # d = 0.35 - x on this cube (|y|, |z| <= 0.75 < 2)
    assert inside.sum() > 50 and outside.sum() > 50
    for k in ("red", "green", "blue", "roughness"):
        assert np.array_equal(va[k][outside], vb[k][outside]), k
    assert np.all(vb["roughness"][inside] == np.float32(0.05)) and np.any(va["roughness"][inside] != np.float32(0.05))
    rgb = np.stack([vb[k][inside] for k in ("red", "green", "blue")], 1)
    assert len(np.unique(rgb, axis=0)) == 1 and rgb[0, 0] > 200 and rgb[0, 1] < 120                   # one colour, red
    assert len(np.unique(np.stack([va[k][inside] for k in ("red", "green", "blue")], 1), axis=0)) > 1
    capsys.readouterr()
