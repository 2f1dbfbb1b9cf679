"""The HIP marcher (csrc/march.hip) against the CPU oracle (`O.sample`) in the regime production runs it in: both lane
mappings, the coarse LDS mask, the occupied box, in-kernel Philox jitter and binding budgets, on the scenes and ray strata
of tests/march_cases.py (lattice planes, faces, zero and tiny direction components, grazing rays, non-cubic volumes, Philox
group edges, the last candidate step, the second trip of the persistent loops).

Every comparison is torch.equal: the marcher's contract is bit-exactness, there is no tolerance."""
import numpy as np
import pytest
import torch

import march_cases as mc
from oracle import nmf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _hip():
    from nmf_amd import hip
    return hip


def _matrix():
    out = []
    for name in mc.MATRIX_SCENES:
        shortcuts = mc.SHORTCUTS if mc.scene(name).vol is not None else ("none",)
        for lanes in ("16", "64"):
            for sh in shortcuts:
                out.append((name, lanes, sh, "eval", "none"))            # (the budget only exists in training)
                for mode in ("explicit", "philox"):
                    for budget in mc.BUDGETS:
                        out.append((name, lanes, sh, mode, budget))
    return out


@pytest.mark.parametrize("name,lanes,shortcut,mode,budget", _matrix())
def test_march_matrix_vs_oracle(name, lanes, shortcut, mode, budget, monkeypatch):
    """valid words (the words after an early exit included), counts, offsets, whole_valid, (M, b), xyzt, ray_id, step_id, z,
    dist and the dense ray_valid / z_vals equal the oracle's, for every ray group of the scene"""
    hip = _hip()
    monkeypatch.setenv("NMF_MARCH_LANES", lanes)
    sc = mc.scene(name)
    for gi, g in enumerate(mc.groups(name)):
        ref = mc.reference(name, gi, mode, budget)
        out = mc.run_marcher(hip, sc, g, mode, shortcut, ref["max_samples"])
        mc.check_march(out, ref, g, f"{name} / {g.name} rays / {lanes} lanes / {shortcut} / {mode} / budget {budget}")


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("mode", mc.MODES)
def test_march_16_lanes_with_partial_groups_of_four(B, mode, monkeypatch):
    """B not a multiple of 4: the idle rows of the last wave load ray B - 1 and must write nothing"""
    hip = _hip()
    monkeypatch.setenv("NMF_MARCH_LANES", "16")
    sc = mc.scene("lattice-random")
    full = mc.groups("lattice-random")[2]
    keeps = torch.nonzero(mc.reference("lattice-random", 2, mode)["counts"] > 0).reshape(-1)[:B].tolist()
    g = mc.Group("few", full.near, full.rays[keeps].contiguous(), [full.labels[i] for i in keeps])
    ref = mc.reference_for(sc, g, mode)
    assert int(ref["counts"].min()) > 0 or mode != "eval"
    for shortcut in mc.SHORTCUTS:
        mc.check_march(mc.run_marcher(hip, sc, g, mode, shortcut), ref, g, f"B = {B} / {shortcut} / {mode}")


@pytest.fixture(scope="module")
def wide_refs():
    cache = {}

    def get(B):
        if B not in cache:
            g = mc.wide_group(B)
            cache[B] = (g, mc.reference_for(mc.scene("lattice-random"), g, "philox"))
        return cache[B]
    return get


@pytest.mark.parametrize("B,lanes", [(16389, "64"), (65541, "16"), (16389, None)])
def test_march_second_trip_of_the_persistent_loops(B, lanes, wide_refs, monkeypatch):
    """4096 workgroups x 4 waves (x 4 rays at 16 lanes) cover 16384 (65536) rays per trip: the smallest batches with a second
    one.  Without an override 16389 rays take the 16-lane kernels (lanes_per_ray: more than 16384 rays); either mapping must
    equal the oracle."""
    hip = _hip()
    if lanes is None:
        monkeypatch.delenv("NMF_MARCH_LANES", raising=False)
    else:
        monkeypatch.setenv("NMF_MARCH_LANES", lanes)
    g, ref = wide_refs(B)
    out = mc.run_marcher(hip, mc.scene("lattice-random"), g, "philox", "coarse+box")
    mc.check_march(out, ref, g, f"B = {B} / lanes {lanes}")


def test_alpha_pack_and_coarse_mask_of_a_non_cubic_volume():
    hip = _hip()
    sc = mc.scene("noncubic")
    gx, gy, gz = sc.grid
    flat = sc.vol.reshape(-1)
    bits = hip.alpha_pack(flat.to(DEV))
    n = flat.numel()
    pad = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    pad[:n] = (flat > 0).numpy()
    want = np.packbits(pad, bitorder="little").view(np.uint32)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), want)
    coarse = hip.alpha_coarse(bits, sc.grid)
    cg = [(g + 7) // 8 for g in (gx, gy, gz)]
    padded = torch.zeros(cg[2] * 8 + 1, cg[1] * 8 + 1, cg[0] * 8 + 1)
    padded[:gz, :gy, :gx] = sc.vol[0, 0]
    ref = torch.nn.functional.max_pool3d(padded[None, None], kernel_size=9, stride=8)[0, 0].reshape(-1) > 0      # [cz][cy][cx]
    assert ref.numel() == 2 * 3 * 5 and 0 < int(ref.sum()) < ref.numel()
    words = coarse.cpu().numpy().view(np.uint32)
    got = torch.tensor([(int(words[i >> 5]) >> (i & 31)) & 1 for i in range(ref.numel())], dtype=torch.bool)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("lanes", ["16", "64"])
def test_march_fill_without_z_returns_the_other_outputs_unchanged(lanes, monkeypatch):
    hip = _hip()
    monkeypatch.setenv("NMF_MARCH_LANES", lanes)
    sc, g = mc.scene("noncubic"), mc.groups("noncubic")[2]
    ref = mc.reference("noncubic", 2, "philox")
    out = mc.run_marcher(hip, sc, g, "philox", "coarse+box", want_z=False)
    assert out["z"] is None and out["M"] > 100
    mc.check_march(out, ref, g, "want_z=False")


@pytest.mark.parametrize("voxel", [(0, 0, 0), (0, 5, 7), (12, 12, 3), (4, 6, 8)])
def test_occupied_box_contains_every_point_with_positive_alpha(voxel):
    """one set voxel in a corner, on a face, on an edge and in the interior: no probe point with O.alpha_query > 0 lies outside
    AlphaGridMask.occupied_box() -- probes on the lattice planes around the voxel, 1e-6 and fractions of a cell beside them"""
    hip = _hip()  # noqa: F841  (the mask packs its bits on the GPU)
    from nmf_amd.samplers.alphagrid import AlphaGridMask
    sc = mc.scene("lattice-one")
    vol = torch.zeros(1, 1, 13, 13, 13)
    vol[0, 0, voxel[2], voxel[1], voxel[0]] = 1
    lo, hi = AlphaGridMask(sc.aabb.to(DEV), vol.to(DEV)).occupied_box()
    axes = []
    for a in range(3):
        c = []
        for i in range(voxel[a] - 3, voxel[a] + 4):
            w = -1.5 + 0.25 * i
            c += [w, w - 1e-6, w + 1e-6, w + 0.03, w + 0.125, w + 0.22]
        c += [lo[a], hi[a], lo[a] - 1e-6, hi[a] + 1e-6]
        axes.append(torch.tensor(sorted(set(c)), dtype=torch.float32))
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    pts = pts[((pts >= sc.aabb[0]) & (pts <= sc.aabb[1])).all(-1)]
    on = O.alpha_query(vol, sc.aabb, pts) > 0
    assert int(on.sum()) >= 6 ** 3                       # (a corner voxel: one cell of six probe coordinates per axis)
    inside = ((pts.double() >= torch.tensor(lo, dtype=torch.float64)) & (pts.double() <= torch.tensor(hi, dtype=torch.float64))).all(-1)
    assert not bool((on & ~inside).any()), pts[on & ~inside][:5]
    # and the box is tight: it ends within 1.5 cells (+ rounding) of the voxel
    for a in range(3):
        assert lo[a] >= -1.5 + 0.25 * (voxel[a] - 1.5) - 1e-6 and hi[a] <= -1.5 + 0.25 * (voxel[a] + 1.5) + 1e-6
