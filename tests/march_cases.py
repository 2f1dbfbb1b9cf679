"""Scenes, ray strata, jitter and CPU-oracle outputs for the marcher tests (tests/test_march_cases_cpu.py checks that the
cases are not vacuous, tests/test_hip_march.py compares the HIP marcher with them bit for bit).

Everything here runs on the CPU: the reference is oracle/nmf_oracle.py (`sample`, `alpha_query`).  The only GPU code is
`run_marcher`, which takes the `nmf_amd.hip` module from its caller.

A scene is an `O.Cfg` (it fixes the AABB, the step size and the number of candidate steps N) plus an alpha volume whose
shape is free.  The rays of a scene come in groups that share a near plane (`O.sample` takes one `near` per call); every
ray carries the name of its stratum so that a failing comparison can say which kind of ray it was."""
import functools
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

from oracle import nmf_oracle as O

FOCAL = 1111.0
SEED, OFFSET = 0x9E3779B9, 12345                    # the Philox stream of the "philox" mode
ONE_BELOW = float(np.float32(1.0) - np.float32(2.0 ** -24))      # the largest uniform the kernels can draw
LONG_STEPS = (15, 16, 63, 64, 255, 256, 511, 512)   # both sides of the 16- / 64- / 256-step rounds and Philox groups
MODES = ("eval", "explicit", "philox")
SHORTCUTS = ("none", "coarse", "coarse+box")
BUDGETS = ("none", "mid", "last")                   # -1; binding with the crossing ray inside / the last of its four


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------
def _philox4x32_10(ctr_lo, ctr_hi, seed):
    """numpy Philox4x32-10 exactly as csrc/common.hpp: counter (lo64, hi64), key = seed (lo32, hi32) -> [n, 4] uint32"""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    c = [np.asarray(ctr_lo & 0xffffffff, np.uint64), np.asarray(ctr_lo >> 32, np.uint64),
         np.full_like(np.asarray(ctr_lo, np.uint64), ctr_hi & 0xffffffff), np.full_like(np.asarray(ctr_lo, np.uint64), ctr_hi >> 32)]
    a, b = np.uint64(seed & 0xffffffff), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(0xffffffff), p1 >> np.uint64(32), p1 & np.uint64(0xffffffff)
        c = [hi1 ^ c[1] ^ a, lo1, hi0 ^ c[3] ^ b, lo0]
        a, b = (a + np.uint64(0x9E3779B9)) & np.uint64(0xffffffff), (b + np.uint64(0xBB67AE85)) & np.uint64(0xffffffff)
    return np.stack(c, -1).astype(np.uint32)


def philox_jitter(B, N, seed=SEED, offset=OFFSET):
    """The marcher's in-kernel jitter as an explicit [B, N] tensor: counter = ray * 1024 + step / 4, component step % 4,
    uniform = (bits >> 8) * 2^-24 (csrc/march.hip step_len, csrc/common.hpp u32_to_unit)."""
    ctr = np.arange(B, dtype=np.uint64)[:, None] * np.uint64(1024) + np.arange((N + 3) // 4, dtype=np.uint64)[None, :]
    o = _philox4x32_10(ctr.reshape(-1), offset, seed).reshape(B, -1)[:, :N]          # [B, ceil(N/4) * 4]: component = k & 3
    return torch.from_numpy((o >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0))


# ---- scenes ------------------------------------------------------------------------------------------------------------
@dataclass
class Scene:
    name: str
    cfg: O.Cfg
    vol: Optional[torch.Tensor]          # [1, 1, gz, gy, gx] of 0 / 1, or None (box test only)

    @property
    def aabb(self):
        return self.cfg.derived()["aabb"]

    @property
    def stepsize(self):
        return float(self.cfg.derived()["stepsize"])

    @property
    def N(self):
        return self.cfg.derived()["n_samples"]

    @property
    def grid(self):
        """(gx, gy, gz) of the alpha volume"""
        gz, gy, gx = self.vol.shape[-3:]
        return gx, gy, gz

    @property
    def empty(self):
        return self.vol is None or not bool(self.vol.any())

    def lattice_dims(self):
        """(gx, gy, gz) of the lattice the strata are built on: the alpha volume's, or 13^3 without one"""
        return self.grid if self.vol is not None else (13, 13, 13)

    def world(self, axis, i):
        """world coordinate of texel index i (any real) on `axis` (align_corners=True), float64"""
        a = self.aabb.double()
        g = self.lattice_dims()[axis]
        return float(a[0][axis]) + (float(a[1][axis]) - float(a[0][axis])) * i / (g - 1)

    def set_voxels(self):
        """[n, 3] integer (x, y, z) indices of the set voxels"""
        if self.vol is None:
            return torch.zeros(0, 3, dtype=torch.long)
        return torch.nonzero(self.vol[0, 0] > 0).flip(-1)

    def occ_box(self):
        """The box outside of which alpha_query cannot be positive, restated on the CPU: the set voxels' index range grown by
        1.5 texels (a set voxel reaches texel coordinates (i - 1, i + 1)); None when nothing is set."""
        sv = self.set_voxels()
        if sv.shape[0] == 0:
            return None
        lo = [self.world(a, float(sv[:, a].min()) - 1.5) for a in range(3)]
        hi = [self.world(a, float(sv[:, a].max()) + 1.5) for a in range(3)]
        return lo, hi


def _vol(gx, gy, gz):
    return torch.zeros(1, 1, gz, gy, gx)


@functools.lru_cache(maxsize=None)
def scene(name):
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name.startswith("lattice"):
        cfg = O.Cfg(grid=13)                                       # spacing 0.25, stepsize 0.125, N = 42
        kind = name.split("-")[1]
        v = _vol(13, 13, 13)
        if kind == "one":
            v[0, 0, 8, 6, 4] = 1                                   # (x, y, z) = (4, 6, 8)
        elif kind == "random":
            v = (torch.rand(v.shape, generator=gen) < 0.05).float()
        elif kind == "half":
            v = (torch.rand(v.shape, generator=gen) < 0.08).float()
            v[..., 9:] = 0                                         # x >= 9 empty: a tight, lopsided occupied box
            v[:, :, :2] = 0                                        # and z < 2
        elif kind == "full":
            v[:] = 1
        elif kind == "none":
            v = None
        else:
            assert kind == "empty", name
        return Scene(name, cfg, v)
    if name == "long":
        cfg = O.Cfg(grid=13, step_ratio=0.03)                      # stepsize 0.0075, N = 693 = 10 * 64 + 53 = 43 * 16 + 5
        v = (torch.rand(1, 1, 13, 13, 13, generator=gen) < 0.12).float()
        v[0, 0, 6, 6, 6] = 1                                       # the centre: where the zero-jitter diagonals end
        return Scene(name, cfg, v)
    if name == "noncubic":
        cfg = O.Cfg(grid=17, aabb=torch.tensor([[-1.0, -2.0, -0.5], [1.0, 2.0, 1.5]]))     # stepsize 0.0625, N = 79
        v = (torch.rand(_vol(9, 17, 33).shape, generator=gen) < 0.04).float()              # 5049 voxels, coarse 2 x 3 x 5
        v[:, :, 27:] = 0                                           # z >= 27 empty
        v[:, :, :, :3] = 0                                         # y < 3 empty
        return Scene(name, cfg, v)
    raise KeyError(name)


LATTICE_SCENES = ("lattice-one", "lattice-random", "lattice-half", "lattice-full", "lattice-empty", "lattice-none")
MATRIX_SCENES = LATTICE_SCENES + ("long", "noncubic")


# ---- rays --------------------------------------------------------------------------------------------------------------
@dataclass
class Group:
    name: str
    near: float
    rays: torch.Tensor                                   # [B, 6]
    labels: List[str]                                    # "stratum" or "stratum:detail" per ray
    pairs: List[Tuple[int, int]] = field(default_factory=list)     # aligned: (ray on the plane, its copy across it)

    def strata(self):
        return [s.split(":")[0] for s in self.labels]


class _Rays:
    def __init__(self):
        self.o, self.d, self.labels = [], [], []

    def add(self, o, d, label):
        self.o.append([float(v) for v in o])
        self.d.append([float(v) for v in d])
        self.labels.append(label)
        return len(self.labels) - 1

    def tensor(self):
        return torch.cat([torch.tensor(self.o, dtype=torch.float32), torch.tensor(self.d, dtype=torch.float32)], -1)


def _unit(v):
    return v / v.norm().clamp_min(1e-20)


def _rand_unit(gen):
    return _unit(torch.randn(3, generator=gen))


def _inside(sc, gen, margin=0.0):
    a = sc.aabb
    return a[0] + margin + (a[1] - a[0] - 2 * margin) * torch.rand(3, generator=gen)


def _targets(sc, gen, n):
    """n points the kept samples are likely near: positions of set voxels (points inside the box when nothing is set)"""
    sv = sc.set_voxels()
    if sv.shape[0] == 0:
        return [_inside(sc, gen, 0.2) for _ in range(n)]
    pick = sv[torch.randint(0, sv.shape[0], (n,), generator=gen)]
    return [torch.tensor([sc.world(a, float(p[a])) for a in range(3)], dtype=torch.float32) for p in pick]


def _primary(sc, gen, R):
    centre = (sc.aabb[0] + sc.aabb[1]) / 2
    tg = _targets(sc, gen, 16)
    for i in range(32):
        o = centre + _rand_unit(gen) * (3.5 + float(torch.rand(1, generator=gen)))
        t = tg[i // 2] + 0.05 * torch.randn(3, generator=gen) if i % 2 == 0 else _inside(sc, gen)
        R.add(o, _unit(t - o), "primary:hit")
    for _ in range(8):                                   # aimed 4 units beside the centre: misses the box
        u = _rand_unit(gen)
        o = centre + u * (3.5 + float(torch.rand(1, generator=gen)))
        side = _unit(torch.linalg.cross(u, _rand_unit(gen)))
        R.add(o, _unit(centre + 4.0 * side - o), "primary:miss")
    for _ in range(8):                                   # t_min clamps to far: every candidate lies beyond the box
        u = _rand_unit(gen)
        R.add(centre + 30.0 * u, -u, "far")


def _secondary(sc, gen, R):
    tg = _targets(sc, gen, 16)
    for i in range(48):
        o = _inside(sc, gen)
        d = _unit(tg[i // 3] + 0.05 * torch.randn(3, generator=gen) - o) if i % 3 == 0 else _rand_unit(gen)
        R.add(o, d, "secondary")
    a = sc.aabb
    for i in range(6):                                   # just inside a face, pointing out
        axis, hi = i % 3, i // 3
        o = _inside(sc, gen, 0.3)
        o[axis] = a[1][axis] - 0.01 if hi else a[0][axis] + 0.01
        d = 0.2 * torch.randn(3, generator=gen)
        d[axis] = 1.0 if hi else -1.0
        R.add(o, _unit(d), "secondary:leaving")


def _faces(sc, gen, R):
    a = sc.aabb
    tg = _targets(sc, gen, 18)
    i = 0
    for nfix in (1, 2, 3):
        for _ in range(6):
            o = _inside(sc, gen, 0.1)
            axes = torch.randperm(3, generator=gen)[:nfix]
            for ax in axes:
                o[ax] = a[int(torch.randint(0, 2, (1,), generator=gen))][ax]        # exactly on the face
            d = _unit(tg[i] + 0.05 * torch.randn(3, generator=gen) - o)
            R.add(o, d, "faces:in")
            R.add(o, -d, "faces:out")
            i += 1


def _parallel(sc, gen, R, values, stratum):
    """Rays with one or two direction components set to each of `values`; on such an axis the origin lies outside the AABB
    slab, inside it but outside the occupied box (where the volume leaves room), or inside both."""
    a = sc.aabb.double()
    box = sc.occ_box()
    dims = sc.lattice_dims()
    for nz in (1, 2):
        for val in values:
            for where in ("outside", "between", "inside"):
                for rep in range(2):
                    t = _targets(sc, gen, 1)[0]
                    axes = [int(x) for x in torch.randperm(3, generator=gen)[:nz]]
                    o = _inside(sc, gen)
                    for j, ax in enumerate(axes):
                        spacing = (float(a[1][ax]) - float(a[0][ax])) / (dims[ax] - 1)
                        inside = min(max(float(t[ax]) + 0.4 * (float(torch.rand(1, generator=gen)) - 0.5) * spacing,
                                         float(a[0][ax])), float(a[1][ax]))
                        if j > 0 or where == "inside":
                            o[ax] = inside
                        elif where == "outside":
                            o[ax] = float(a[1][ax]) + 0.3 if rep else float(a[0][ax]) - 0.3
                        else:
                            room_hi = float(a[1][ax]) - box[1][ax] if box else 0.0
                            room_lo = box[0][ax] - float(a[0][ax]) if box else 0.0
                            if max(room_hi, room_lo) <= 0.05:
                                o = None
                                break
                            o[ax] = (box[1][ax] + float(a[1][ax])) / 2 if room_hi >= room_lo else (box[0][ax] + float(a[0][ax])) / 2
                    if o is None:
                        continue
                    d = (t - o).double()
                    if rep:                                      # the second of each kind does not aim at a set voxel
                        d = torch.randn(3, generator=gen).double()
                    for ax in axes:
                        d[ax] = 0.0
                    d = d / d.norm().clamp_min(1e-20) if float(d.norm()) > 0 else d
                    if nz == 2 and float(d.norm()) == 0:
                        continue
                    for ax in axes:
                        d[ax] = val
                    R.add(o, d, f"{stratum}:{where}:{val!r}")


def _grazing(sc, gen, R):
    """Rays parallel to a face of the occupied box: at texel offsets inside the footprint of the outermost set voxel, between
    the footprint and the box face (no corner with a positive weight) and beyond the face."""
    sv = sc.set_voxels()
    if sv.shape[0] == 0:
        return
    a = sc.aabb
    # (offset 1: the footprint's edge, where the rounding of the texel coordinate decides -- (x - lo) * (2 / size) is not exact)
    offs = [(-0.5, "in"), (0.5, "in"), (0.75, "in"), (1.0, "edge"), (1.03125, "between"), (1.25, "between"), (1.5, "between"),
            (1.75, "beyond"), (2.5, "beyond")]
    for ax in range(3):
        b, c = (ax + 1) % 3, (ax + 2) % 3
        for sign in (1, -1):
            edge = int(sv[:, ax].max()) if sign > 0 else int(sv[:, ax].min())
            v = sv[sv[:, ax] == edge][0]
            for off, tag in offs:
                o = torch.zeros(3, dtype=torch.float64)
                o[ax] = sc.world(ax, edge + sign * off)
                o[b] = float(a[0][b])
                o[c] = sc.world(c, float(v[c]))
                d = torch.zeros(3, dtype=torch.float64)
                d[b] = 1.0
                R.add(o, d, f"grazing:{tag}")
                d2 = d.clone()                                   # the same line tilted inside the plane of constant `ax`
                d2[c] = 0.25
                o2 = o.clone()
                o2[c] = o[c] - 0.25 * (sc.world(b, float(v[b])) - float(a[0][b]))
                R.add(o2, d2 / d2.norm(), f"grazing:{tag}")


def _eval_counts(sc, rays, near):
    """kept samples per ray in eval mode (the oracle)"""
    if rays.shape[0] == 0:
        return torch.zeros(0, dtype=torch.long)
    cfg = O.Cfg(**{**sc.cfg.__dict__, "max_samples": -1})
    return O.sample(rays, FOCAL, cfg, sc.vol, O.Noise(), False, override_near=near)[1].sum(1)


def _aligned(sc, gen, R, pairs, cap=48):
    """Axis-parallel rays that start on a face of the AABB and run inside a lattice plane of the alpha volume (both other
    origin coordinates are lattice coordinates, one row of planes outside the box included): in eval mode with near = 0 every
    sample lies on lattice planes, where a corner weight is zero or a rounding error away from it.  Each ray comes with copies moved by +-1e-6 across
    the plane; only the pairs whose kept counts differ are kept -- the oracle decides which planes matter for this volume."""
    a = sc.aabb.double()
    dims = sc.lattice_dims()
    cand_o, cand_d, meta = [], [], []
    for b in range(3):
        p, q = (b + 1) % 3, (b + 2) % 3
        for sign in (1, -1):
            for ip in range(-1, dims[p] + 1):
                for iq in range(-1, dims[q] + 1):
                    o = [0.0, 0.0, 0.0]
                    o[b] = float(a[0][b]) if sign > 0 else float(a[1][b])
                    o[p], o[q] = sc.world(p, ip), sc.world(q, iq)
                    d = [0.0, 0.0, 0.0]
                    d[b] = float(sign)
                    for shift_axis, shift in ((None, 0.0), (p, 1e-6), (p, -1e-6), (q, 1e-6), (q, -1e-6)):
                        oo = list(o)
                        if shift_axis is not None:
                            oo[shift_axis] += shift
                        cand_o.append(oo)
                        cand_d.append(d)
                    meta.append((b, sign, ip, iq))
    rays = torch.cat([torch.tensor(cand_o, dtype=torch.float32), torch.tensor(cand_d, dtype=torch.float32)], -1)
    cnt = _eval_counts(sc, rays, 0.0).reshape(-1, 5)
    decisive = torch.nonzero((cnt[:, 1:] != cnt[:, :1]).any(1)).reshape(-1)
    if decisive.shape[0] > cap:
        decisive = decisive[torch.linspace(0, decisive.shape[0] - 1, cap).long()]
    for ci in decisive.tolist():
        base = R.add(rays[5 * ci, :3], rays[5 * ci, 3:], "aligned:plane")
        for j in range(1, 5):
            if int(cnt[ci, j]) != int(cnt[ci, 0]):
                pairs.append((base, R.add(rays[5 * ci + j, :3], rays[5 * ci + j, 3:], "aligned:moved")))


def _diagonals(sc, gen, R):
    """near-diagonal rays from the corners; the first eight are exact diagonals (label zero: an all-zero jitter row keeps
    their last candidate step inside the box), the next eight take jitter rows of 1 - 2^-24"""
    a = sc.aabb
    for i in range(64):
        corner = torch.tensor([a[(i >> k) & 1][k] for k in range(3)])
        d = (a[0] + a[1]) - 2 * corner
        if i >= 8:
            d = d + 0.12 * float(d.norm()) * torch.randn(3, generator=gen)
        R.add(corner, _unit(d), "diagonal:zero" if i < 8 else ("diagonal:one" if i < 16 else "diagonal"))


@functools.lru_cache(maxsize=None)
def groups(scene_name):
    sc = scene(scene_name)
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, scene_name)))
    out = []
    R = _Rays()
    _primary(sc, gen, R)
    out.append(Group("primary", float(sc.cfg.near_far[0]), R.tensor(), R.labels))
    R = _Rays()
    _secondary(sc, gen, R)
    out.append(Group("secondary", 3 * sc.stepsize, R.tensor(), R.labels))          # override_near of the re-traced rays
    R, pairs = _Rays(), []
    _secondary(sc, gen, R)
    _faces(sc, gen, R)
    _parallel(sc, gen, R, (0.0, -0.0), "parallel")
    _parallel(sc, gen, R, (1e-13, -1e-13, 1e-11, -1e-11, 1e-7, -1e-7), "nearparallel")
    _grazing(sc, gen, R)
    if not sc.empty:
        _aligned(sc, gen, R, pairs)
    if scene_name == "long":
        _diagonals(sc, gen, R)
    out.append(Group("zero", 0.0, R.tensor(), R.labels, pairs))
    return tuple(out)


def wide_group(B):
    """B secondary rays in the lattice-random scene (more than one trip of the persistent count kernels)"""
    sc = scene("lattice-random")
    gen = torch.Generator().manual_seed(B)
    a = sc.aabb
    o = a[0] + (a[1] - a[0]) * torch.rand(B, 3, generator=gen)
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    sv = sc.set_voxels()
    t = torch.stack([a[0][k] + (a[1][k] - a[0][k]) * sv[torch.randint(0, sv.shape[0], (B,), generator=gen), k].float() / 12
                     for k in range(3)], -1)
    aimed = torch.arange(B) % 3 == 0
    d[aimed] = torch.nn.functional.normalize(t - o, dim=-1)[aimed]
    return Group("wide", 3 * sc.stepsize, torch.cat([o, d], -1), ["wide"] * B)


# ---- jitter ------------------------------------------------------------------------------------------------------------
def explicit_jitter(group, N):
    """random uniforms; all-zero rows and rows of 1 - 2^-24 on rays 1 and 2 and on the labelled diagonals"""
    B = group.rays.shape[0]
    U = torch.rand(B, N, generator=torch.Generator().manual_seed(7 + B))
    for r, lab in enumerate(group.labels):
        if lab == "diagonal:zero" or r == 1:
            U[r] = 0.0
        elif lab == "diagonal:one" or r == 2:
            U[r] = ONE_BELOW
    return U


def jitter_of(group, N, mode):
    if mode == "eval":
        return None
    return explicit_jitter(group, N) if mode == "explicit" else philox_jitter(group.rays.shape[0], N)


# ---- the oracle's outputs ----------------------------------------------------------------------------------------------
def pack_words(rv):
    """[B, N] bool -> [B, ceil(N / 64)] int64: bit k of word j = step 64 j + k (the marcher's valid words)"""
    B, N = rv.shape
    W = (N + 63) // 64
    pad = np.zeros((B, W * 64), dtype=np.uint8)
    pad[:, :N] = rv.numpy()
    return torch.from_numpy(np.packbits(pad.reshape(B, W, 64), axis=-1, bitorder="little").view(np.uint64).reshape(B, W).view(np.int64).copy())


def pick_budget(counts, kind):
    """max_samples that binds with 0 < b < B: the cumulative count of a ray j that keeps samples, so that j is the first
    dropped ray.  kind 'mid': j is the second of its group of four rays; 'last': the fourth.  None if there is no such ray."""
    cum = counts.cumsum(0)
    total = int(cum[-1]) if counts.numel() else 0
    want = 1 if kind == "mid" else 3
    cands = [j for j in range(1, counts.shape[0]) if j % 4 == want and int(counts[j]) > 0 and int(cum[j]) < total
             and int(cum[j - 1]) > 0]
    if not cands:
        return None
    return int(cum[cands[len(cands) // 2]])


def _oracle(sc, group, jitter, max_samples):
    cfg = O.Cfg(**{**sc.cfg.__dict__, "max_samples": max_samples})
    is_train = jitter is not None
    noise = O.Noise([("rand", jitter)]) if is_train else O.Noise()
    return O.sample(group.rays, FOCAL, cfg, sc.vol, noise, is_train, override_near=group.near)


def reference_for(sc, group, mode, budget="none"):
    """Everything the marcher pipeline returns, from O.sample: the packed valid words and counts of ALL rays (the count pass
    knows no budget), then offsets, whole_valid, (M, b) and the compacted / dense outputs under the budget."""
    jit = jitter_of(group, sc.N, mode)
    xyz, rv, n, z, dists, wv = _oracle(sc, group, jit, -1)
    B = group.rays.shape[0]
    counts = rv.sum(1)
    ref = dict(words=pack_words(rv), counts=counts, max_samples=-1, full_rv=rv)
    if budget != "none" and mode != "eval":
        ref["max_samples"] = pick_budget(counts, budget) or -1
        if ref["max_samples"] > 0:
            xyz, rv, n, z, dists, wv = _oracle(sc, group, jit, ref["max_samples"])
    b = int(wv.sum())
    M = int(xyz.shape[0])
    cum = counts.cumsum(0)
    offsets = torch.cat([torch.where(wv, cum - counts, torch.full_like(cum, M)), torch.tensor([M])])
    ref.update(xyz=xyz, ray_valid=rv, z_vals=z, dists=dists, whole_valid=wv, b=b, M=M, offsets=offsets, B=B)
    return ref


@functools.lru_cache(maxsize=None)
def reference(scene_name, group_index, mode, budget="none"):
    return reference_for(scene(scene_name), groups(scene_name)[group_index], mode, budget)


# ---- the marcher (GPU; `hip` is the nmf_amd.hip module) ---------------------------------------------------------------------
def run_marcher(hip, sc, group, mode, shortcut="none", max_samples=-1, want_z=True, dev="cuda"):
    """count -> scan -> fill -> dense as the sampler runs them.  shortcut: 'none' | 'coarse' (the LDS mask) | 'coarse+box' (and
    AlphaGridMask.occupied_box()); mode 'philox' draws the jitter in the kernel (jitter=None, seed / offset set)."""
    aabb = sc.aabb
    is_train = mode != "eval"
    jit = explicit_jitter(group, sc.N).to(dev).contiguous() if mode == "explicit" else None
    seed, offset = (SEED, OFFSET) if mode == "philox" else (0, 0)
    bits = coarse = box = None
    if sc.vol is not None:
        bits = hip.alpha_pack(sc.vol.to(dev).reshape(-1))
        if shortcut != "none":
            coarse = hip.alpha_coarse(bits, sc.grid)
        if shortcut == "coarse+box":
            from nmf_amd.samplers.alphagrid import AlphaGridMask
            box = AlphaGridMask(aabb.to(dev), sc.vol.to(dev)).occupied_box()
    p = hip.march_params(aabb, (1.0 / (aabb[1] - aabb[0]) * 2).numpy(), sc.stepsize, group.near, sc.cfg.near_far[1], FOCAL, sc.N,
                         sc.grid if sc.vol is not None else None, is_train, seed=seed, offset=offset, occ_box=box)
    rays = group.rays.to(dev).contiguous()
    valid, counts = hip.march_count(p, rays, jit, bits, coarse)
    offsets, wv, totals = hip.march_scan(counts, max_samples if is_train else -1)
    M, b = [int(v) for v in totals.cpu()]
    xyzt, ray_id, step_id, z, dist = hip.march_fill(p, rays, b, M, jit, valid, offsets, want_z)
    rv, zd = hip.march_dense(p, rays, b, jit, valid)
    return dict(words=valid.cpu(), counts=counts.cpu(), offsets=offsets.cpu(), whole_valid=wv.bool().cpu(), M=M, b=b,
                xyz=xyzt.cpu(), ray_id=ray_id.cpu(), step_id=step_id.cpu(), z=None if z is None else z.cpu(), dist=dist.cpu(),
                ray_valid=rv.cpu(), z_vals=zd.cpu())


def _names(group, rows):
    rows = sorted(set(int(r) for r in rows))
    return ", ".join(f"ray {r} [{group.labels[r]}]" for r in rows[:6]) + (f" and {len(rows) - 6} more" if len(rows) > 6 else "")


def check_march(out, ref, group, what=""):
    """every output of the pipeline against the oracle, bit for bit; a mismatch names the rays (and their strata)"""
    B, b = ref["B"], ref["b"]
    bad = torch.nonzero((out["words"] != ref["words"]).any(1)).reshape(-1)
    assert bad.numel() == 0, f"{what}: valid words differ on {_names(group, bad)}"
    assert torch.equal(out["counts"].long(), ref["counts"]), f"{what}: counts"
    assert (out["M"], out["b"]) == (ref["M"], b), f"{what}: (M, b) = {(out['M'], out['b'])}, oracle {(ref['M'], b)}"
    assert torch.equal(out["whole_valid"], ref["whole_valid"]), f"{what}: whole_valid"
    assert torch.equal(out["offsets"], ref["offsets"]), f"{what}: offsets"
    rv = ref["ray_valid"]
    ri, si = torch.where(rv)
    assert torch.equal(out["ray_valid"], rv), f"{what}: dense ray_valid"
    assert torch.equal(out["ray_id"].long(), ri) and torch.equal(out["step_id"].long(), si), f"{what}: ray_id / step_id"
    for k, want in (("z_vals", ref["z_vals"]), ("xyz", ref["xyz"]), ("z", ref["z_vals"][rv]), ("dist", ref["dists"][rv])):
        if out[k] is None:
            continue
        same = out[k] == want                            # (no NaNs here: equal bits up to the sign of zero ...
        if not torch.equal(out[k], want) or not torch.equal(torch.signbit(out[k]), torch.signbit(want)):      # ... which is compared too)
            rows = torch.nonzero(~same.reshape(same.shape[0], -1).all(1)).reshape(-1)
            rays_bad = rows if k == "z_vals" else ri[rows]
            steps = "" if k == "z_vals" else f" steps {sorted(set(si[rows].tolist()))[:8]}"
            raise AssertionError(f"{what}: {k} differs on {_names(group, rays_bad)}{steps}")
