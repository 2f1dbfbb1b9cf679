"""Material edits (nmf_amd/edit.py, nmf_heads_edit / nmf_material_maps_edit) without a GPU: the command-line grammar and the YAML /
JSON files, the packed table's layout, the numpy restatement (identity, float32 against float64), the argument checks of the two
C-ABI entry points, the wrappers' refusal of host tensors, and checkpoints that never see the edits."""
import argparse
import ctypes as C
import json

import numpy as np
import pytest
import torch

from nmf_amd import edit as E

U = 2.0 ** -24          # unit roundoff of float32


def _args(argv):
    ap = argparse.ArgumentParser()
    E.add_arguments(ap)
    return ap.parse_args(argv)


SPECS = [
    "albedo=0.6,0.05,0.05", "albedo=0.5", "f0*0.5,1,2", "roughness*0.4", "albedo+0.1,-0.1,0", "roughness+-0.05", "roughness=0.3",
    "albedo^sat0.25", "f0^sat1.5", "albedo^hue120", "f0^hue-30",
    "albedo=1,0,0@all", "albedo=1,0,0@box(0,0,0.2,0.3,0.3,0.2)", "f0=0.9@sphere(0.1,-0.2,0,0.5)", "roughness*2@ellipsoid(0,0,0,0.5,0.25,1)",
    "albedo=1,0,0@!all", "albedo=0.6,0.05,0.05@!box(0,0,0.2,0.3,0.3,0.2)~0.05", "f0=0.9@!sphere(0,0,0,0.5)",
    "roughness=0.02@!ellipsoid(1,1,1,0.5,0.25,1)~0.125", "albedo*1.5~0.5",
]


def test_grammar_round_trips_through_the_command_line_and_files(tmp_path):
    """every OP, every region and invert: --edit SPEC, a YAML file and a JSON file of the dataclass fields give the same table"""
    import yaml
    for spec in SPECS:
        e = E.parse_spec(spec)
        t = E.pack_numpy([e])
        assert t.shape == (1, 32) and t.dtype == np.float32
        assert np.array_equal(E.pack_numpy(E.from_args(_args(["--edit", spec]))), t), spec
        assert np.array_equal(E.pack_numpy(E.from_args(_args(["--edit", " " + spec.replace(",", " , ")]))), t), spec   # blanks are free
        for name, dump in (("e.yaml", yaml.safe_dump), ("e.json", json.dumps)):
            p = tmp_path / name
            p.write_text(dump([e.to_dict()]))
            assert np.array_equal(E.pack_numpy(E.from_args(_args(["--edit-file", str(p)]))), t), (spec, name)
    # order: the file's edits first, then the --edit ones in their order
    p = tmp_path / "two.yaml"
    p.write_text(yaml.safe_dump([E.parse_spec(s).to_dict() for s in SPECS[:2]]))
    got = E.pack_numpy(E.from_args(_args(["--edit-file", str(p), "--edit", SPECS[3], "--edit", SPECS[2]])))
    assert np.array_equal(got, E.pack_numpy([E.parse_spec(s) for s in (SPECS[0], SPECS[1], SPECS[3], SPECS[2])]))
    # what the operators mean
    assert E.parse_spec("albedo=0.6,0.05,0.05") == E.MaterialEdit.set("albedo", (0.6, 0.05, 0.05))
    assert E.parse_spec("roughness*0.4") == E.MaterialEdit.scale("roughness", 0.4)
    assert E.parse_spec("f0+0.1") == E.MaterialEdit.add("f0", 0.1)
    assert E.parse_spec("f0=0.9@!sphere(0,0,0,0.5)") == E.MaterialEdit.set("f0", 0.9, E.Region.sphere((0, 0, 0), 0.5), invert=True)
    assert E.parse_spec("albedo=1@box(0,0,0.2,0.3,0.3,0.2)~0.05") == \
        E.MaterialEdit.set("albedo", 1, E.Region.box((0, 0, 0.2), (0.3, 0.3, 0.2)), falloff=0.05)
    sat = np.asarray(E.MaterialEdit.saturation("albedo", 0.0).matrix)
    assert np.allclose(sat, np.tile(E.LUMA, (3, 1))) and np.allclose(np.asarray(E.MaterialEdit.saturation("f0", 1.0).matrix), np.eye(3))
    hue = np.asarray(E.MaterialEdit.hue("albedo", 120).matrix)
    assert np.allclose(hue @ [1, 0, 0], [0, 1, 0], atol=1e-12) and np.allclose(hue @ [1, 1, 1], [1, 1, 1]) and \
        np.allclose(hue @ hue.T, np.eye(3), atol=1e-12)


@pytest.mark.parametrize("spec,token", [
    ("tint=1", "tint"), ("colour=1", "colour"), ("albedo", "operator ''"), ("albedo%3", "%3"), ("albedo=a", "'a'"),
    ("albedo=1,2", "'1,2'"), ("roughness=1,2,3", "'1,2,3'"), ("albedo=1@cube(1)", "cube(1)"), ("albedo=1@box(1,2,3)", "'1,2,3'"),
    ("albedo=1@box(0,0,0,1,1,-1)", "box(0,0,0,1,1,-1)"), ("albedo=1@sphere(0,0,0,1", "sphere(0,0,0,1"), ("albedo=1~x", "'x'"),
    ("albedo=1~-1", "'-1'"), ("albedo=1~", "'~'"), ("albedo^sat", "^sat"), ("roughness^hue3", "^hue"), ("albedo=1e", "'1e'"),
])
def test_malformed_specs_name_the_offending_token(spec, token, capsys):
    with pytest.raises(E.EditError) as ei:
        E.parse_spec(spec)
    assert token in str(ei.value) and spec in str(ei.value)
    from nmf_amd import export_mesh, render
    for main in (render.main, export_mesh.main):           # refused by the parser, before a device or a checkpoint is touched
        with pytest.raises(SystemExit):
            main(["--ckpt", "none.th", "--edit", spec])
        assert token in capsys.readouterr().err


def test_list_limits_and_field_checks(tmp_path):
    with pytest.raises(E.EditError, match="at most 16"):
        E.pack_numpy([E.MaterialEdit("albedo")] * 17)
    assert E.pack_numpy([E.MaterialEdit("albedo")] * 16).shape == (16, 32) and E.pack_numpy([]).shape == (0, 32)
    for bad in (dict(target="tint"), dict(target="albedo", falloff=-1.0), dict(target="albedo", falloff=float("nan")),
                dict(target="f0", matrix=[[1, 0], [0, 1]]), dict(target="f0", offset=(0, float("inf"), 0)),
                dict(target="f0", region=E.Region.all(), matrix=np.full((3, 3), np.nan))):
        with pytest.raises(E.EditError):
            E.MaterialEdit(**bad)
    for bad in (dict(kind="cone"), dict(kind="box", extent=(1, 0, 1)), dict(kind="ellipsoid", extent=(1, 1, -1))):
        with pytest.raises(E.EditError):
            E.Region(**bad)
    p = tmp_path / "bad.yaml"
    p.write_text("- {target: albedo, colour: 3}\n")
    with pytest.raises(E.EditError, match="colour"):
        E.load_file(p)


def test_table_layout():
    """[K][32] fp32: kind | target | invert | falloff | c 3 | h 3 | A 9 row-major | b 3 | 10 zeros"""
    A = np.arange(1, 10, dtype=np.float64).reshape(3, 3) / 16
    e = [E.MaterialEdit("f0", A, (0.25, 0.5, 0.75), E.Region.ellipsoid((1, 2, 3), (4, 5, 6)), falloff=0.125, invert=True),
         E.MaterialEdit("roughness", 2 * np.eye(3), (0.5, 0, 0), E.Region.box((-1, -2, -3), (0.5, 0.25, 0.125))),
         E.MaterialEdit("albedo")]
    t = E.pack(e, "cpu")
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == (3, 32) and t.is_contiguous()
    want = np.zeros((3, 32), dtype=np.float32)
    want[0, :22] = [2, 1, 1, 0.125, 1, 2, 3, 4, 5, 6, *A.reshape(9), 0.25, 0.5, 0.75]
    want[1, :22] = [1, 2, 0, 0, -1, -2, -3, 0.5, 0.25, 0.125, 2, 0, 0, 0, 2, 0, 0, 0, 2, 0.5, 0, 0]
    want[2, :22] = [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(t.numpy(), want)
    assert (E.ROW, E.MAX_EDITS, E.KINDS, E.TARGETS) == (32, 16, ("all", "box", "ellipsoid"), ("albedo", "f0", "roughness"))
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "nmf_hip.h")).read()
    assert "#define NMF_EDIT_ROW 32" in hdr and "#define NMF_EDIT_MAX 16" in hdr and "#define NMF_ABI_VERSION 125" in hdr


def _heads(rng, n):
    h = rng.uniform(0.0, 1.0, (n, 11)).astype(np.float32)
    h[:, 9:] = np.clip(h[:, 9:], 0.01, 1.0)          # the heads' own range
    h[h == 0] = 0.5                                  # (a sigmoid is never 0; -0 + 0 would not keep its sign bit)
    return h


def test_identity_edit_returns_its_input_bits():
    rng = np.random.default_rng(1)
    h, x = _heads(rng, 4096), rng.uniform(-2, 2, (4096, 4)).astype(np.float32)
    regions = [E.Region.all(), E.Region.box((0, 0, 0), (1, 1, 1)), E.Region.sphere((0.5, 0, 0), 1.0), E.Region.ellipsoid((0, 0, 0), (1, 0.5, 2))]
    edits = [E.MaterialEdit(t, region=r, falloff=f, invert=i) for t in E.TARGETS for r in regions for f in (0.0, 0.5) for i in (False, True)]
    for k in range(0, len(edits), 16):
        out = E.apply_reference(h, x, edits[k:k + 16], np.float32)
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), h.view(np.uint32))
    assert np.array_equal(E.apply_reference(h, x, [], np.float32).view(np.uint32), h.view(np.uint32))


def _random_operator(rng, target):
    A = rng.uniform(-1, 1, (3, 3))
    A *= rng.uniform(0, 8, (3, 1)) / np.abs(A).sum(1, keepdims=True)          # |A| row sums in [0, 8]
    b = rng.uniform(-1, 1, 3)
    return dict(target=target, matrix=A, offset=b)


HARD_BOUND = 37 * U         # 2.2e-6
SOFT_BOUND = 2440 * U       # 1.45e-4


def test_float32_restatement_against_float64():
    """10 000 rows, one edit per target and list (an edit's input is then exact in both precisions), v in [0, 1], x and c in
    [-2, 2]^3, |A| row sums <= 8, |b| <= 1, h in [1/4, 2], falloff 0 or in [1/16, 1].  Both precisions read the same float32 table
    and inputs, so the difference is float32 rounding alone, u = 2^-24 per operation:

    operator   t = ((A0 v0 + A1 v1) + A2 v2) + b: three products and three sums, |err| <= ((1 + u)^4 - 1)(sum |A_i v_i| + |b|)
               <= 4.0001 u 9 < 37 u; the clamp is 1-Lipschitz.  Roughness (A00 v + b) has two roundings: 18 u.
    hard mask  m is 0 or 1 in both precisions unless a point changes sides, which needs |d| below the error of d (at most 358 u =
               2.1e-5, below); the test asserts in float64 that no point lies within 1e-4 of a boundary, so out = t or v and
               |err| <= 37 u = 2.2e-6 (HARD_BOUND).  The positions are lattice points k / 8 and the boundaries are off the lattice
               by construction: box centres on the lattice with half extents (j + 1/2) / 8, so |d| >= 1/16; ellipsoid centres on
               the lattice with radii s_i sqrt(n + 1/3) / 8, s_i in {1, 2}, 16 <= n <= 40: sum (k_i / s_i)^2 is a multiple of 1/4
               and n + 1/3 is at least 1/12 from one, so |r^2 - 1| >= (1/12) / 40.34, |r - 1| >= 1e-3 near the surface and
               |d| = |r - 1| min(h) >= 1e-3 * 0.5 (float32 rounding of the radii moves this by 1e-7).
    soft mask  where float64 has d / falloff > 2 both precisions clamp s to 0 (the error of d / falloff is at most 358 u 16 << 1
               anywhere: |q_i| <= 16, r <= 28, the chain below with those magnitudes) and the hard bound holds.  Elsewhere
               d <= 2, so r - 1 <= 8, r <= 9: q_i carries 2 u relative (difference, quotient), the sum of squares 7 u, r 4.5 u
               relative = 40.5 u, r - 1 another 8 u, d = (r - 1) min(h) <= 2 (48.5 u) + 2 u = 99 u (a box: 10 u); d / falloff
               <= 99 u 16 + 2 u, s = clamp(1 - .) adds u: 1587 u; m = (s s)(3 - 2 s) has |dm/ds| <= 3/2 and four roundings of
               values <= 3: 2387 u; invert adds u; out = v + m (t - v) with |t - v| <= 1: 2388 u + 37 u + 3 u roundings < 2440 u =
               1.45e-4 (SOFT_BOUND)."""
    rng = np.random.default_rng(20240611)
    n = 10000
    h = _heads(rng, n)
    lattice = (rng.integers(-16, 17, (n, 3)) / 8.0).astype(np.float32)
    free = rng.uniform(-2, 2, (n, 3)).astype(np.float32)

    def region(kind, hard):
        c = rng.integers(-16, 17, 3) / 8.0 if hard else rng.uniform(-2, 2, 3)
        if kind == "box":
            ext = (rng.integers(2, 16, 3) + 0.5) / 8.0 if hard else rng.uniform(0.25, 2, 3)
        else:
            ext = rng.integers(1, 3, 3) * np.sqrt(rng.integers(16, 41) + 1.0 / 3.0) / 8.0 if hard else rng.uniform(0.25, 2, 3)
        return E.Region(kind, c, ext)

    worst = dict(hard=0.0, soft=0.0)
    margin = np.inf
    for trial in range(8):
        for hard in (True, False):
            for invert in (False, True):
                kinds = [("all", "box", "ellipsoid")[(trial + i) % 3] for i in range(3)]
                edits = [E.MaterialEdit(region=E.Region.all() if k == "all" else region(k, hard), invert=invert,
                                        falloff=0.0 if hard else float(rng.uniform(1 / 16, 1)), **_random_operator(rng, t))
                         for t, k in zip(E.TARGETS, kinds)]
                x = lattice if hard else free
                tab = E.pack_numpy(edits)
                if hard:
                    for e, row in zip(edits, tab.astype(np.float64)):
                        if e.region.kind == "all":
                            continue
                        p = x.astype(np.float64) - row[4:7]
                        d = (np.abs(p) - row[7:10]).max(1) if e.region.kind == "box" else \
                            (np.sqrt(((p / row[7:10]) ** 2).sum(1)) - 1) * row[7:10].min()
                        margin = min(margin, float(np.abs(d).min()))
                        assert np.abs(d).min() > 1e-4, (trial, e.region)
                        assert (d < 0).any() and (d > 0).any(), "the region must split the points"
                o32, o64 = E.apply_reference(h, x, tab, np.float32), E.apply_reference(h, x, tab, np.float64)
                assert o32.dtype == np.float32 and o64.dtype == np.float64
                assert np.abs(o64 - h).max() > 0.1, "the edit must do something"
                assert np.array_equal(o32[:, 3:6], h[:, 3:6])            # the tint head is never touched
                err = float(np.abs(o32.astype(np.float64) - o64).max())
                worst["hard" if hard else "soft"] = max(worst["hard" if hard else "soft"], err)
    print(f"float32 against float64: hard {worst['hard']:.3e} (bound {HARD_BOUND:.3e}), soft {worst['soft']:.3e} (bound {SOFT_BOUND:.3e}), "
          f"smallest |d| of a hard mask {margin:.3e}")
    assert worst["hard"] <= HARD_BOUND and worst["soft"] <= SOFT_BOUND


def test_chained_edits_see_the_result_of_the_one_before():
    rng = np.random.default_rng(3)
    h, x = _heads(rng, 64), rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    a, b = E.MaterialEdit.scale("albedo", 0.5), E.MaterialEdit.add("albedo", 0.75)
    ab, ba = E.apply_reference(h, x, [a, b], np.float64), E.apply_reference(h, x, [b, a], np.float64)
    assert np.allclose(ab[:, :3], np.clip(0.5 * h[:, :3].astype(np.float64) + 0.75, 0, 1))
    assert np.allclose(ba[:, :3], 0.5 * np.clip(h[:, :3].astype(np.float64) + 0.75, 0, 1))
    r = E.apply_reference(h, x, [E.MaterialEdit.set("roughness", 0.001), E.MaterialEdit.scale("roughness", 200.0)], np.float32)
    assert np.array_equal(r[:, 9:], np.ones((64, 2), np.float32))          # clipped to the head's [0.01, 1] after each edit
    assert np.array_equal(r[:, :9], h[:, :9])


# ---- the C ABI, without a device -----------------------------------------------------------------------------------------------
def _lib():
    from nmf_amd import hip
    return hip, hip._lib


def _err(lib):
    return lib.nmf_last_error_string().decode()


def test_entry_points_are_exported_and_check_their_arguments():
    hip, lib = _lib()
    assert "nmf_heads_edit" in hip.EXPORTS and "nmf_material_maps_edit" in hip.EXPORTS and hip.version() >= 125
    ok = E.pack_numpy([E.parse_spec("albedo=1@box(0,0,0,1,1,1)~0.1"), E.parse_spec("roughness*0.5")])
    tab = lambda t: t.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    P = C.c_void_p(64)                                                            # never dereferenced: every call below is refused
    bad_h, many, nan = ok.copy(), np.tile(ok[:1], (17, 1)), ok.copy()
    bad_h[0, 8] = 0.0
    nan[1, 10] = np.nan
    neg_f, bad_kind = ok.copy(), ok.copy()
    neg_f[0, 3] = -0.5
    bad_kind[0, 0] = 3.0

    def heads_edit(heads=P, xyz=P, stride=4, n=5, t=ok, k=None):
        return lib.nmf_heads_edit(heads, xyz, stride, n, tab(t) if t is not None else None, len(t) if k is None else k, None)

    for call, code in ((lambda: heads_edit(heads=None), -1), (lambda: heads_edit(xyz=None), -1), (lambda: heads_edit(t=None, k=2), -1),
                       (lambda: heads_edit(stride=2), -1), (lambda: heads_edit(stride=5), -1), (lambda: heads_edit(n=-1), -1),
                       (lambda: heads_edit(k=-1), -1), (lambda: heads_edit(t=many), -2), (lambda: heads_edit(t=bad_h), -2),
                       (lambda: heads_edit(t=nan), -2), (lambda: heads_edit(t=neg_f), -2), (lambda: heads_edit(t=bad_kind), -2)):
        assert call() == code and "nmf_heads_edit" in _err(lib), _err(lib)
    # nothing to do: no launch, no pointer is looked at -- but the table is still checked
    assert heads_edit(heads=None, xyz=None, n=0) == 0 and heads_edit(heads=None, xyz=None, t=None, k=0) == 0
    assert heads_edit(heads=None, xyz=None, n=0, t=bad_h) == -2

    def maps_edit(B=4, M=10, Mb=2, R=5, p=P, xyz=P, stride=4, t=ok, k=None, rows=P):
        return lib.nmf_material_maps_edit(p, p, p, p, B, M, p, p, p, 1.0, 0.0, 0.0, 0.0, 0.0, p, rows, rows, rows, Mb, rows, rows, R, p, p, p,
                                          xyz, stride, tab(t) if t is not None else None, len(t) if k is None else k, None)

    for call, code in ((lambda: maps_edit(p=None), -1), (lambda: maps_edit(xyz=None), -1), (lambda: maps_edit(rows=None), -1),
                       (lambda: maps_edit(stride=6), -1), (lambda: maps_edit(B=-1), -1), (lambda: maps_edit(M=-1), -1),
                       (lambda: maps_edit(t=None, k=1), -1), (lambda: maps_edit(t=many), -2), (lambda: maps_edit(t=bad_h), -2),
                       (lambda: maps_edit(t=nan), -2), (lambda: maps_edit(Mb=11), -1)):
        assert call() == code and "nmf_material_maps_edit" in _err(lib), _err(lib)
    assert maps_edit(B=0, M=0, Mb=0, R=0, p=None, xyz=None, rows=None) == 0
    # the entry without edits keeps its prototype (tests/test_material_maps_cpu.py calls it positionally)
    assert len(lib.nmf_material_maps.argtypes) == 26 and len(lib.nmf_material_maps_edit.argtypes) == 30
    assert len(lib.nmf_heads_edit.argtypes) == 7


def test_wrappers_refuse_cpu_tensors():
    hip, _ = _lib()
    t = E.pack([E.MaterialEdit.scale("roughness", 0.5)])
    with pytest.raises(hip.NmfHipError):
        hip.heads_edit(torch.zeros(4, 11), torch.zeros(4, 3), t)
    z = torch.zeros
    with pytest.raises(hip.NmfHipError):
        hip.material_maps(z(4, 24), z(4, 3), z(4), z(3, dtype=torch.int64), z(2, 6), z(11, 24), z(11), (1.0, 0.0, 0.0, 0.0, 0.0), z(9, 3),
                          z(2), z(3), xyz=z(4, 4), edits=t)


def test_model_holds_edits_outside_its_state_and_checkpoints(tmp_path):
    """a checkpoint saved with edits set is byte-identical to one saved without; training calls refuse edits"""
    from nmf_amd.config import build_model
    nerf, cfg = build_model(grid=16, bg_resolution=16, device="cpu")
    keys = set(nerf.state_dict())
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    a, b = tmp_path / "a" / "m.th", tmp_path / "b" / "m.th"          # (torch.save writes the file's own name into the archive)
    nerf.save(str(a), dict(cfg["arch"]))
    edits = [E.parse_spec("albedo=0.6,0.05,0.05@box(0,0,0.2,0.3,0.3,0.2)~0.05"), E.parse_spec("roughness*0.4")]
    nerf.set_material_edits(edits)
    assert nerf.material_edits == edits and set(nerf.state_dict()) == keys
    assert not any("edit" in k for k in keys) and not any("edit" in n for n, _ in list(nerf.named_buffers()) + list(nerf.named_parameters()))
    nerf.save(str(b), dict(cfg["arch"]))
    assert a.read_bytes() == b.read_bytes()
    with pytest.raises(ValueError, match="material edits"):
        nerf(torch.zeros(4, 6), 100.0, is_train=True)
    with pytest.raises(E.EditError):
        nerf.set_material_edits([E.MaterialEdit("albedo")] * 17)
    assert nerf.material_edits == edits                      # a refused list changes nothing
    nerf.set_material_edits(None)
    assert nerf.material_edits == [] and nerf._material_edit_table is None and nerf.model._material_edit_table is None
