"""The marcher cases of tests/march_cases.py are not vacuous: with the CPU oracle alone, every stratum of every scene has rays
that keep samples and rays that keep none, the lattice-plane pairs and the grazing rays decide as they are meant to, the long
scene keeps the steps on both sides of every round / Philox-group edge, and the binding budgets bind where they should.
These are conditions on the cases (seeds are chosen so that they hold), not measurements of the code under test."""
import pytest
import torch

import march_cases as mc

NON_EMPTY = [s for s in mc.MATRIX_SCENES if not mc.scene(s).empty]


def _kept_by_stratum(name, mode):
    """stratum -> list of kept counts, over all groups of the scene"""
    out = {}
    for gi, g in enumerate(mc.groups(name)):
        counts = mc.reference(name, gi, mode)["counts"]
        for s, c in zip(g.strata(), counts.tolist()):
            out.setdefault(s, []).append(c)
    return out


def test_scene_dimensions_are_the_ones_the_cases_rely_on():
    lat, lng, ncb = mc.scene("lattice-one"), mc.scene("long"), mc.scene("noncubic")
    assert (lat.N, lat.stepsize) == (42, 0.125)
    assert lng.N == 693 == 10 * 64 + 53 == 43 * 16 + 5 and abs(lng.stepsize - 0.0075) < 1e-9
    assert (ncb.N, ncb.stepsize) == (79, 0.0625) and ncb.grid == (9, 17, 33) and 9 * 17 * 33 % 32 != 0
    assert [(g + 7) // 8 for g in ncb.grid] == [2, 3, 5]
    box = mc.scene("lattice-half").occ_box()
    assert box[1][0] < 1.5 - 0.25 and box[0][2] > -1.5 + 0.1            # tight in x (upper side) and z (lower side)
    assert float(mc.philox_jitter(3, 42).max()) < 1.0 and mc.ONE_BELOW < 1.0


@pytest.mark.parametrize("name", NON_EMPTY)
@pytest.mark.parametrize("mode", ["eval", "explicit", "philox"])
def test_every_stratum_keeps_samples_on_some_rays_and_none_on_others(name, mode):
    """Exceptions: `far` keeps nothing by construction.  In eval mode with near = 0 a ray that starts inside a FULL volume
    keeps its first candidate (the origin itself, weight one), so `faces` has no empty ray there: that one combination only
    has to keep samples."""
    kept = _kept_by_stratum(name, mode)
    expected = {"primary", "far", "secondary", "faces", "parallel", "nearparallel", "grazing", "aligned"}
    assert expected <= set(kept), sorted(expected - set(kept))
    for s, counts in kept.items():
        if s == "far":
            assert max(counts) == 0
            continue
        assert max(counts) > 0, f"{name} / {mode}: no {s} ray keeps a sample"
        if (name, mode, s) == ("lattice-full", "eval", "faces") or s == "diagonal":      # (diagonals: the long-scene test below)
            continue
        assert min(counts) == 0, f"{name} / {mode}: every {s} ray keeps samples"


@pytest.mark.parametrize("name", NON_EMPTY)
def test_aligned_pairs_differ_in_their_kept_count(name):
    g = mc.groups(name)[2]
    counts = mc.reference(name, 2, "eval")["counts"]
    assert len(g.pairs) >= 8
    for i, j in g.pairs:
        assert g.labels[i] == "aligned:plane" and g.labels[j] == "aligned:moved"
        assert float((g.rays[i] - g.rays[j]).abs().max()) < 2e-6
        assert int(counts[i]) != int(counts[j]), (name, i, j)


def test_the_lattice_plane_next_to_one_voxel_keeps_nothing_and_its_neighbour_keeps_four():
    """the case the aligned stratum is about, spelled out: one set voxel at x index 4 (x = -0.5); a ray along z in the plane
    x = -0.25 (texel 5, weight exactly 0) keeps nothing, the same ray moved by 1e-6 towards the voxel keeps 4"""
    sc = mc.scene("lattice-one")
    rays = torch.tensor([[-0.25, 0.0, -1.5, 0.0, 0.0, 1.0], [-0.25 - 1e-6, 0.0, -1.5, 0.0, 0.0, 1.0]])
    g = mc.Group("x", 0.0, rays, ["aligned", "aligned"])
    assert mc.reference_for(sc, g, "eval")["counts"].tolist() == [0, 4]


@pytest.mark.parametrize("name", NON_EMPTY)
@pytest.mark.parametrize("mode", ["eval", "explicit", "philox"])
def test_grazing_rays_between_footprint_and_box_face_keep_nothing(name, mode):
    g = mc.groups(name)[2]
    counts = mc.reference(name, 2, mode)["counts"].tolist()
    by = {}
    for lab, c in zip(g.labels, counts):
        if lab.startswith("grazing:"):
            by.setdefault(lab.split(":")[1], []).append(c)
    assert max(by["between"]) == 0 and max(by["beyond"]) == 0
    assert max(by["in"]) > 0


@pytest.mark.parametrize("mode", ["explicit", "philox"])
def test_long_scene_keeps_the_steps_at_every_round_edge(mode):
    g = mc.groups("long")[2]
    rv = mc.reference("long", 2, mode)["full_rv"]
    assert rv.shape[1] == 693
    for k in mc.LONG_STEPS:
        assert bool(rv[:, k].any()), f"step {k} is kept on no ray ({mode})"
    # the last step of a Philox group (16-lane kernel: 63, 64-lane kernel: 255) kept with the next one culled
    assert bool((rv[:, 63] & ~rv[:, 64]).any()) or bool((rv[:, 255] & ~rv[:, 256]).any())
    if mode == "explicit":                               # the zero-jitter diagonals end inside the box: dist = 0 branch
        zero = [i for i, lab in enumerate(g.labels) if lab == "diagonal:zero"]
        assert bool(rv[zero, 692].any()), "step N-1 is kept on no ray"
        one = [i for i, lab in enumerate(g.labels) if lab == "diagonal:one"]
        assert bool(rv[one].any())


@pytest.mark.parametrize("name", NON_EMPTY + ["lattice-none"])
@pytest.mark.parametrize("mode", ["explicit", "philox"])
@pytest.mark.parametrize("budget,pos", [("mid", 1), ("last", 3)])
def test_binding_budgets_bind_with_the_crossing_ray_where_it_should_be(name, mode, budget, pos):
    """0 < b < B, the first dropped ray (index b) is the second / the last of its group of four rays -- in the big near = 0
    group of every scene, and in whichever other groups keep enough"""
    bound = []
    for gi, g in enumerate(mc.groups(name)):
        ref = mc.reference(name, gi, mode, budget)
        if ref["max_samples"] > 0:
            assert 0 < ref["b"] < ref["B"] and ref["b"] % 4 == pos and 0 < ref["M"] < int(ref["counts"].sum())
            assert not bool(ref["whole_valid"][ref["b"]]) and bool(ref["whole_valid"][ref["b"] - 1])
            bound.append(gi)
    assert 2 in bound, (name, mode, budget, bound)


def test_wide_groups_take_a_second_trip_of_the_persistent_loops():
    assert 16389 > 4096 * 4 and (65541 + 3) // 4 > 4096 * 4 and (16389 + 3) // 4 <= 4096 * 4
    g = mc.wide_group(16389)
    counts = mc.reference_for(mc.scene("lattice-random"), g, "philox")["counts"]
    assert int(counts[16384:].sum()) > 0 and int((counts == 0).sum()) > 100 and int((counts > 0).sum()) > 1000
