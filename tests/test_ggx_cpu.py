"""The GGX ray sampler and the Fresnel mix (csrc/ggx.hip) without a GPU: constructed inputs, float64 references PER RAY, a per-ray
yardstick kappa, fp32 restatements, and the margins that tests/test_hip_ggx.py holds the kernels to -- with the tests that show the
margins are tighter than tests/test_hip_parity.py and not blind.

Reference.  sample_rays / mix below restate oracle.ggx_sample / oracle.ggx_prob (brdf_samplers/ggx.py:61-268) and the Fresnel-Schlick
mix (models/microfacet.py:595-613) per ray on the compact ray list, in torch, in the dtype of their inputs; float64 is the reference,
adjoints by autograd on per-ray leaves.  The structure is the reference's: a = 1 / (1 + Vs.z) is detached, sign and frame choice are
constants, clamp passes the gradient on the closed side (torch.clamp; dual.hpp d_clipmin / d_clip say the same).
test_per_ray_definition_is_the_oracle holds the fp32 form to oracle.ggx_sample on the padded [rows, m] layout.

What is computed in fp32 first: u = fmod(sobol[j] + off * 0.25f, 1) in np.float32 (load_ray, ggx.hip:113-114; exact in IEEE), and the
one predicate on an fp32 input, |N.z| < 0.999f (ggx.hip:58).  Every predicate on a computed value is decided in float64 and the inputs
keep it CLEAR = 1e-3 away from its threshold or exactly on it (test_every_gate_is_clear_or_exact); inputs are constructed: a row (V, N,
r, off) is redrawn and a ray takes another table entry j until that holds.  No ray is left out of any comparison.  Two places where
CLEAR cannot be an absolute distance, and what holds instead:
  * Vs.z >= 0.999 (ggx.hip:63): the band [0.999, 1] is 1e-3 wide.  Rays on that side keep Vs.z >= 0.9995 (CLEAR / 2, > 2000 fp32
    steps of Vs.z); rays on the other side keep Vs.z <= 0.998.
  * the clips inside ggx_prob (li.z^2 at 1e-6, the two logs at EPS, r at EPS; ggx.hip:88-94): no gradient flows through ggx_prob and a
    clip is continuous, so either side gives the same value to rounding; their thresholds are themselves far below 1e-3.  Sampler
    batches keep li.z^2 >= 1e-6 + CLEAR and 4 lo.z >= CLEAR; the ggx_prob batches enter every clipped side on purpose.  The one
    discontinuity, li.z > 0, is an fp32 input there (decided on the fp32 value) and CLEAR away inside the sampler (it is the sign gate).
The zero-normal rows are exact instead of clear: tangent = bitangent = Vs = H = 0, a == 1, dot(wi, N) == 0, L = V / |V|.

Yardstick.  kappa of an element = the largest change of the float64 reference under K = 8 seeded relative perturbations of +-2^-23 of
the fp32 inputs (four random sign patterns and their negations; sampler: V, N, r, u1, u2; mix: V, L, f0, diffuse, inc, brdf, d_rows;
ggx_prob: li, lo, h, r).  Normalised error of element i = |got - ref| / (kappa_i + 2^-23 scale_i), scale_i the largest |ref| of the
quantity on that ray.  Margin per metric and batch = 8 x the largest normalised error of the fp32 restatement (the same definition in
torch float32 with float32 autograd, taking its own decisions), at least 1: the suites' floor of 2^-23 x scale in these units.  It binds
only where the restatement is (nearly) exact; the test prints where.

u1 ladder, compared forward only: a ray whose float64 1 - P1^2 - P2^2 is below CLEAR.  On the lower azimuth half that is 1 - u1, so
the rungs 0.999 (1 - float32(0.999) = 0.99999e-3), 1 - 2^-12 and 1 - 2^-24 are forward-only there: 96 rays of the `strata` batch, 12
of the batches of 255 - 257.  The last is below EPS: w3 is the clipped sqrt(EPS), its gradient zero in the reference and an fp32 coin
toss in any fp32 code -- the ill-defined corner, nothing to fix.  On the upper half P2 carries Vs.z <= 0.923 (a ladder row keeps a in
[0.52, 0.8]) and 1 - P1^2 - P2^2 stays above CLEAR: all seven rungs are compared in full there, as are 0, 0.5, 0.9 and 0.98 on the
lower half.  On forward-only rays the adjoints must be finite.

Strata and the line of csrc/ggx.hip each enters (test_batches_enter_the_branches_they_are_named_for counts them, >= 64 rays each in
the `strata` batch; the batches of 1, 255, 256, 257 rays take rows of every stratum in turn and print what they hold):
    general, r in [0.01, 0.5]         :58 z_up, :63 cross branch, :67 both halves, :81 both signs
    nz_on   N.z == float32(0.999)     :58 `<` false -> x_up           nz_below  one float less -> z_up
    pole    N = (0, 0, +-1)           :58 x_up                        zero      N = 0: :32 clip in every nrm, :81 sgn = -1
    vs_hi   r <= 0.05, V near N       :63 T1 = x_up (Vs.z >= 0.9995)  r_lo / r_hi  r == 0.01 / 0.5
    lower / upper                     :68, :71 (only the upper half scales P2 by Vs.z)
    ladder  off = 0, table entries with u1 in {0, .5, .9, .98, .999, 1 - 2^-12, 1 - 2^-24} x both halves   :66 rr = 0, :72 clip
    wrap    off in [0.9, 1)           :113-114 fmodf wraps            last entry of the 1024-entry table: a ladder ray
    flipped dot(wi, N) < 0            :81-82
    mix: anti L == -V (:224 n2 == 0, :250 s = 0, Fr = 1), same L == V on axis rows (:229 om_raw == 0, the closed side of :246),
         f0 / diffuse rows of 0 and 1, rows of 1 and of M_MAX rays, dV asked for or not (:254)
    ggx_prob: back li.z < 0 and zero li.z == +-0 (:95 -> exactly 0), grazing li.z^2 < 1e-6 (:91), tiny_lo (:94 second log), r_eps (:88-89)

Measured (test_restatement_ratios_and_margins prints them; they depend on the host's float32 sin / cos / log, so the margins are computed
where the tests run): largest normalised error of the restatement -> margin, `strata` batch (2104 rays; mix 821, ggx_prob 576), x86 CPU
    L 1.84 -> 14.7   half 1.84 -> 14.7   diff 1.84 -> 14.7   lpdf 2.68 -> 21.4   mipval 3.24 -> 25.9   origin 1.52 -> 12.1
    dN  dL 13.8 -> 111   rays 11.5 -> 92    both 19.2 -> 154         mix contrib 0.63 -> 5.0   d_inc 0.86 -> 6.9   d_brdf 0.87 -> 7.0
    dr  dL 31.5 -> 252   rays 16.0 -> 128   both 15.3 -> 122             dL 2.02 -> 16.1   d_f0 0.65 -> 5.2   d_diff 0.74 -> 5.9   dV 2.15 -> 17.2
    dV  dL 7.2 -> 57.8   rays 5.7 -> 45.8   both 9.1 -> 72.8         ggx_prob 5.23 -> 41.9
The batches of 255 - 257 rays: forward 0.9 - 4.8, adjoints 2.2 - 19.  The floor of 1 binds only in the one-ray batch (dr, and contrib /
d_brdf / d_diff of the mix, ggx_prob: restatement below 0.1).  On the ray of median kappa the margins allow 5e-6 in L (the fp32 test:
1.2e-5 on 99.5 % of the rays, 1e-4 on all), 3e-5 .. 2e-4 in the adjoints (3e-2 .. 1e-1), 2e-8 .. 4e-7 in the mix (1.5e-5 .. 3e-3).

The margins are not blind (test_broken_restatements_miss_their_margins; largest normalised error / margin on the stratum named):
    Vs.z factor of P2 dropped          L, upper azimuth half                  6.1e+05
    a not detached                     dN 2.4e+05   dr 7.0e+04, general rows
    sign flip ignored in the adjoint   dN 5.6e+04   dV 1.3e+05, flipped rays
    x_up where z_up belongs            half 5.0e+05   dN 965, nz_below
    5e-3 d_rays[0:3] dropped           dN 1.0e+03   dr 800, general rows, d_rays alone
    Fresnel dV without -dd H           dV 1.5e+05       mix dL without s hd H    dL 1.3e+06
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import nmf_oracle as O

F32, F64 = np.float32, np.float64
EPS = float(np.finfo(F32).eps)
FLOOR = 2.0 ** -23
CLEAR = 1e-3
K = 8                                       # perturbations per kappa
M_MAX = 14                                  # most rays of a row: a ladder row has 7 rungs x 2 azimuth halves
N_TABLE = 1024
TH = F32(0.999)                             # the constant ggx.hip compares fp32 values with
VS_HI = 0.999 + CLEAR / 2
RUNGS = (0.0, 0.5, 0.9, 0.98, 0.999, 1.0 - 2.0 ** -12, 1.0 - 2.0 ** -24)
LADDER_U2 = ((0.11, 0.27, 0.41), (0.86, 0.91, 0.97))     # lower / upper azimuth half for every a in [0.52, 0.8]
N_LADDER = len(RUNGS) * 2 * 3
RAY_COUNTS = (1, 255, 256, 257)
BATCHES = tuple(f"r{n}" for n in RAY_COUNTS) + ("strata",)
ROW_STRATA = {"general": 96, "nz_on": 24, "nz_below": 24, "pole": 24, "zero": 24, "vs_hi": 40, "r_lo": 24, "r_hi": 24, "ladder": 32,
              "wrap": 24, "graze": 64}
FWD = ("L", "half", "diff", "lpdf", "mipval", "origin")
ADJ = ("dN", "dr", "dV")
VARIANTS = ("dL", "rays", "both")           # which of the two adjoints the backward is given
MIX_ROW_STRATA = {"general": 48, "cnt1": 64, "cntm": 6, "f0_0": 16, "f0_1": 16, "diff_0": 16, "diff_1": 16, "anti": 16, "same": 18}
MIX_METRICS = ("contrib", "d_inc", "d_brdf", "dL", "d_f0", "d_diff", "dV")
PROB_STRATA = ("general", "back", "zero", "grazing", "tiny_lo", "r_eps")


def _ro(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def _t(a, dt=torch.float64):
    return torch.from_numpy(np.array(a)).to(dt)               # (a copy: the shared inputs are read-only)


def _unit32(v):
    v = np.asarray(v, dtype=F64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


# ---- the definition, per ray, in the dtype of its inputs ----------------------------------------------------------------------------
def _nz(v):
    return v / (v * v).sum(-1, keepdim=True).clip(min=EPS).sqrt()           # oracle.normalize


def _dot(a, b):
    return (a * b).sum(-1)


def sample_rays(V, N, r, u1, u2, up_is_z, fault=None):
    """oracle.ggx_sample + the glue of models/microfacet.py:377-456 for R independent rays: V, N [R,3], r, u1, u2 [R], up_is_z [R] bool
    (|N.z| < 0.999f, decided on the fp32 input).  fault: a break built in on purpose (test_broken_restatements_miss_their_margins).
    -> namespace of L, half, diff [R,3], lpdf [R] and the gate values vsz, a, w3sq, dwn, llz, ndv"""
    dt = V.dtype
    one = torch.ones((), dtype=dt)
    z_up = torch.tensor([0.0, 0.0, 1.0], dtype=dt).expand_as(N)
    x_up = torch.tensor([-1.0, 0.0, 0.0], dtype=dt).expand_as(N)
    up = torch.where(up_is_z[:, None], z_up, x_up)
    t = _nz(torch.linalg.cross(up, N))
    b = _nz(torch.linalg.cross(N, t))
    Vl = torch.stack([_dot(t, V), _dot(b, V), _dot(N, V)], -1)
    Vs = _nz(torch.stack([r * Vl[:, 0], r * Vl[:, 1], Vl[:, 2]], -1))
    z = Vs[:, 2]
    T1 = torch.where((z < 0.999)[:, None], _nz(torch.linalg.cross(Vs, z_up)), x_up)
    T2 = _nz(torch.linalg.cross(T1, Vs))
    a = (1 / (1 + (z if fault == "a" else z.detach())).clip(min=1e-8)).clip(max=1e4)
    lower = u2 < a
    rr = u1.sqrt()
    phi = torch.where(lower, u2 / a * math.pi, (u2 - a) / (1 - a) * math.pi + math.pi)
    phi = torch.remainder(phi, 100 * math.pi)                                # safemath.safe_trig_helper
    P1 = rr * phi.cos()
    P2 = rr * phi.sin() * (one if fault == "p2" else torch.where(lower, one, z))
    w3sq = 1 - P1 * P1 - P2 * P2
    Ns = P1[:, None] * T1 + P2[:, None] * T2 + w3sq.clip(min=EPS).sqrt()[:, None] * Vs
    Hl = _nz(torch.stack([Ns[:, 0] * r, Ns[:, 1] * r, Ns[:, 2]], -1))
    H = t * Hl[:, 0:1] + b * Hl[:, 1:2] + N * Hl[:, 2:3]
    wi = _nz(2.0 * _dot(V, H)[:, None] * H - V)
    dwn = _dot(wi, N)
    sign = torch.where(dwn > 0, one, -one)[:, None]
    L = wi.detach() * sign + (wi - wi.detach()) if fault == "sign" else wi * sign
    Ll = torch.stack([_dot(t, L), _dot(b, L), _dot(N, L)], -1)
    with torch.no_grad():
        lpdf = O.ggx_prob(Ll, Vl, Hl, r).clip(min=EPS).log().reshape(-1)
    H2 = _nz((V + L) / 2)
    half = torch.stack([_dot(t, H2), _dot(b, H2), _dot(N, H2)], -1)
    return SimpleNamespace(L=L, half=half, diff=Ll, lpdf=lpdf, vsz=z.detach(), a=a.detach(), w3sq=w3sq.detach(), dwn=dwn.detach(),
                           llz=Ll[:, 2].detach(), ndv=Vl[:, 2].detach(), lower=lower)


def mix(V, L, f0, diffuse, inc, brdf, ec, fault=None):
    """models/microfacet.py:595-613 per ray: H = normalize((V + L) / 2), F = f0 + (1 - f0) clip(1 - |V.H|, 0, 1)^5,
    contrib = (F Li brdf + (1 - F) diffuse) / max(count, 1).  fault "direct": V reaches d = -V.H only through H; "proj": H = h / |h| with
    |h| held constant (no projection term)"""
    h = (V + L) / 2
    n = (h * h).sum(-1, keepdim=True).clip(min=EPS).sqrt()
    H = h / (n.detach() if fault == "proj" else n)
    c = (-((V.detach() if fault == "direct" else V) * H).sum(-1, keepdim=True)).abs()
    Fr = f0 + (1 - f0) * (1 - c).clip(0, 1) ** 5
    return (Fr * inc * brdf + (1 - Fr) * diffuse) / ec[:, None]


# ---- inputs of the sampler -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table():
    """the [1024, 2] table in the place of the Sobol points: uniform fp32 draws, the last 42 entries the u1 ladder x both azimuth halves
    x three u2 each (a ladder row has off = 0, so u is the entry itself)"""
    tab = np.random.default_rng(3).uniform(0.0, 1.0, (N_TABLE, 2)).astype(F32)
    tab[tab >= 1] = 0.5
    lad = [(u1, u2) for u1 in RUNGS for half in (0, 1) for u2 in LADDER_U2[half]]
    tab[N_TABLE - N_LADDER:] = np.asarray(lad, dtype=F64).astype(F32)
    assert tab[-1, 0] == F32(1.0 - 2.0 ** -24) and tab[N_TABLE - N_LADDER, 0] == 0
    tab.setflags(write=False)
    return tab


def ladder_entry(rung, half, c):
    return N_TABLE - N_LADDER + (rung * 2 + half) * 3 + c % 3


def _ring(z, th):
    s = math.sqrt(1.0 - float(z) ** 2)
    return [s * math.cos(th), s * math.sin(th), float(z)]


def draw_row(stratum, k, attempt):
    """row k of a stratum, the attempt-th draw of it -> V [3], N [3], r, off [2] in float32"""
    sid = list(ROW_STRATA).index(stratum)
    rng = np.random.default_rng([41, sid, k, attempt])
    V = _unit32(rng.standard_normal(3))
    r = F32(rng.uniform(0.01, 0.5))
    off = rng.uniform(0.0, 1.0, 2).astype(F32)
    N = None
    if stratum in ("nz_on", "nz_below"):
        z = TH if stratum == "nz_on" else np.nextafter(TH, F32(0))
        N = np.asarray(_ring(z, rng.uniform(0, 2 * math.pi)), dtype=F64).astype(F32)
        N[2] = z
        if k % 2:
            N = -N
    elif stratum == "pole":
        N = np.array([0, 0, 1 if k % 2 else -1], dtype=F32)
    elif stratum == "zero":
        N = np.zeros(3, dtype=F32)
    if N is None:                                           # the normal around the view direction, facing it (as bounce prep leaves it)
        spread = {"vs_hi": 0.2, "graze": 3.0, "ladder": 2.0}.get(stratum, 0.8)
        N = _unit32(V.astype(F64) + spread * rng.standard_normal(3))
        if float(np.dot(V.astype(F64), N.astype(F64))) < 0:
            N = -N
    elif N.any():                                           # a view direction on the given normal's side
        V = _unit32(N.astype(F64) + 0.8 * rng.standard_normal(3))
        if float(np.dot(V.astype(F64), N.astype(F64))) < 0:
            V = -V
    if stratum == "vs_hi":
        r = F32(rng.uniform(0.01, 0.05))
    elif stratum == "r_lo":
        r = F32(0.01)
    elif stratum == "r_hi":
        r = F32(0.5)
    elif stratum == "ladder":
        r = F32(rng.uniform(0.25, 0.5))
        off[:] = 0
    elif stratum == "wrap":
        off = rng.uniform(0.9, 1.0, 2).astype(F32)
    return V, N, r, off


def row_count(stratum, k):
    return M_MAX if stratum == "ladder" else 1 + (5 * k + 2) % 8          # 1 .. 8 mixed, 4.5 on average


def _u_of(tab, off, rows, js):
    """load_ray, ggx.hip:113-114, in fp32"""
    o = off[rows] * F32(0.25)
    return np.fmod(tab[js, 0] + o[:, 0], F32(1)).astype(F32), np.fmod(tab[js, 1] + o[:, 1], F32(1)).astype(F32)


def _gates64(V, N, r, off, rows, js):
    up = np.abs(N[rows, 2]) < TH
    u1, u2 = _u_of(table(), off, rows, js)
    with torch.no_grad():
        s = sample_rays(_t(V[rows]), _t(N[rows]), _t(r[rows]), _t(u1), _t(u2), torch.from_numpy(up))
    return s, u1, u2


def gate_report(V, N, r, off, rows, js, ladder_ray):
    """-> (bad [R] bool, namespace of the float64 gate values): which rays miss the clearance this module promises"""
    s, u1, u2 = _gates64(V, N, r, off, rows, js)
    zero = ~N[rows].any(axis=1)
    vsz, a, w3sq, dwn, llz, ndv = (x.numpy() for x in (s.vsz, s.a, s.w3sq, s.dwn, s.llz, s.ndv))
    bad = ~((vsz <= 0.999 - CLEAR) | (vsz >= VS_HI))
    bad |= np.abs(u2.astype(F64) - a) < CLEAR
    bad |= np.abs(dwn) < CLEAR
    bad |= (w3sq < CLEAR) & ~ladder_ray
    bad |= llz ** 2 < 1e-6 + CLEAR
    bad |= 4 * ndv < CLEAR
    exact = zero & (vsz == 0) & (a == 1) & (dwn == 0) & (llz == 0) & (ndv == 0)
    bad &= ~exact
    bad |= zero & ~exact
    return bad, SimpleNamespace(vsz=vsz, a=a, u2=u2, u1=u1, w3sq=w3sq, dwn=dwn, llz=llz, ndv=ndv, zero=zero, lower=s.lower.numpy())


def _plan(name):
    """[(stratum, k, count)] of a batch"""
    if name == "strata":
        return [(s, k, row_count(s, k)) for s, n in ROW_STRATA.items() for k in range(n)]
    R = int(name[1:])
    if R == 1:
        return [("general", 0, 1)]
    plan, total, k = [], 0, 0
    names = list(ROW_STRATA)
    while total < R:
        s = names[k % len(names)]
        c = min(row_count(s, 100 + k), R - total)
        plan.append((s, 100 + k, c))
        total += c
        k += 1
    return plan


@functools.lru_cache(maxsize=None)
def sampler_inputs(name):
    """V, N, x [Mb,3], r [Mb], off [Mb,2], cnt [Mb] int32, sobol [1024,2], row_of_ray, j_of_ray [R] int32, row_off [Mb+1] int64, the
    adjoints dL [R,3] and d_rays [R,6], and per ray: stratum, rung (-1 off the ladder), fwd_only, up_is_z, u1, u2 and the gate values g"""
    plan = _plan(name)
    Mb = len(plan)
    cnt = np.array([c for _, _, c in plan], dtype=np.int32)
    rows = np.repeat(np.arange(Mb), cnt)
    loc = np.arange(len(rows)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    R = len(rows)
    ladder_row = np.array([s == "ladder" for s, _, _ in plan])
    ladder_ray = ladder_row[rows]
    rung = np.where(ladder_ray, loc % len(RUNGS), -1)
    half = loc // len(RUNGS)
    row_try, ray_try = np.zeros(Mb, dtype=np.int64), np.zeros(R, dtype=np.int64)
    plan_k = np.array([k for _, k, _ in plan], dtype=np.int64)
    V, N, off, r = np.zeros((Mb, 3), F32), np.zeros((Mb, 3), F32), np.zeros((Mb, 2), F32), np.zeros(Mb, F32)
    stale = np.ones(Mb, dtype=bool)
    for _ in range(200):
        for i in np.nonzero(stale)[0]:
            V[i], N[i], r[i], off[i] = draw_row(plan[i][0], plan[i][1], int(row_try[i]))
        rng_j = (np.arange(R) * 7919 + ray_try * 104729 + np.repeat(np.arange(Mb), cnt) * 31 + sum(map(ord, name))) % (N_TABLE - N_LADDER)
        js = np.where(ladder_ray, N_TABLE - N_LADDER + (np.maximum(rung, 0) * 2 + half % 2) * 3 + (plan_k[rows] + ray_try) % 3, rng_j)
        bad, g = gate_report(V, N, r, off, rows, js, ladder_ray)
        if ladder_ray.any():                                # a ladder row keeps a in [0.52, 0.8]: LADDER_U2 then sits on its side
            bad |= ladder_ray & ((g.a < 0.52) | (g.a > 0.8))
        if not bad.any():
            break
        ray_try[bad] += 1                                   # another table entry for the ray; a row whose own gates fail, or whose ray
        row_gate = ~((g.vsz <= 0.999 - CLEAR) | (g.vsz >= VS_HI)) | (4 * g.ndv < CLEAR) | ladder_ray & ((g.a < 0.52) | (g.a > 0.8)) | g.zero
        redraw = np.zeros(Mb, dtype=bool)                   # found no entry in seven tries, is drawn again
        redraw[rows[bad & ((ray_try > 6) | row_gate)]] = True
        row_try[redraw] += 1
        ray_try[redraw[rows]] = 0
        stale = redraw
    else:
        raise AssertionError(f"{name}: the inputs did not come clear")
    rng = np.random.default_rng([43, sum(map(ord, name))])
    stratum = np.array([s for s, _, _ in plan])[rows]
    return _ro(SimpleNamespace(
        name=name, R=R, Mb=Mb, V=V, N=N, r=r, off=off, cnt=cnt, x=rng.standard_normal((Mb, 3)).astype(F32), sobol=table(),
        row_of_ray=rows.astype(np.int32), j_of_ray=js.astype(np.int32), row_off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64),
        dL=rng.standard_normal((R, 3)).astype(F32), d_rays=rng.standard_normal((R, 6)).astype(F32), stratum=stratum, rung=rung,
        fwd_only=g.w3sq < CLEAR, up_is_z=np.abs(N[rows, 2]) < TH, u1=g.u1, u2=g.u2, g=g, ladder_ray=ladder_ray))


# ---- float64 reference, kappa, restatement of the sampler -------------------------------------------------------------------------
def _signs(seed, shapes):
    """K sign patterns per input: K / 2 random ones and their negations, so every input moves both ways"""
    rng = np.random.default_rng(seed)
    half = [[rng.choice([-1.0, 1.0], size=s) for s in shapes] for _ in range(K // 2)]
    return half + [[-p for p in pat] for pat in half]


def run_sampler(i, dt, fault=None, scale=None):
    """forward and the three backward variants on per-ray leaves in dtype dt (float64: the reference; float32: the restatement) ->
    dict of float64 numpy arrays over FWD and `metric/variant` for ADJ x VARIANTS.  scale: five relative factors [R, ...] on V, N, r,
    u1, u2 (kappa)"""
    rows = i.row_of_ray
    ins = [i.V[rows].astype(F64), i.N[rows].astype(F64), i.r[rows].astype(F64), i.u1.astype(F64), i.u2.astype(F64)]
    if scale is not None:
        ins = [a * s for a, s in zip(ins, scale)]
    V, N, r = (_t(a, dt).requires_grad_(True) for a in ins[:3])
    u1, u2 = _t(ins[3], dt), _t(ins[4], dt)
    up = torch.from_numpy(np.array(i.up_is_z) if fault != "frame" else np.abs(i.N[rows, 2]) < np.nextafter(TH, F32(0)))
    s = sample_rays(V, N, r, u1, u2, up, fault)
    x = _t(i.x[rows], dt)
    origin = x + s.L * 5e-3
    lp = s.lpdf
    out = {"L": s.L, "half": s.half, "diff": s.diff, "lpdf": lp, "mipval": -_t(np.maximum(i.cnt[rows], 1), dt).log() - lp, "origin": origin}
    dL, dq = _t(i.dL, dt), _t(i.d_rays, dt)
    through_rays = (s.L * dq[:, 3:6]).sum() + (0.0 if fault == "origin" else (origin * dq[:, 0:3]).sum())
    for v, loss in zip(VARIANTS, ((s.L * dL).sum(), through_rays, (s.L * dL).sum() + through_rays)):
        gV, gN, gr = torch.autograd.grad(loss, [V, N, r], retain_graph=True)
        out["dN/" + v], out["dr/" + v], out["dV/" + v] = gN, gr, gV
    return {k: v.detach().double().numpy() for k, v in out.items()}


def normalised(got, ref, kap):
    """|got - ref| / (kappa + 2^-23 x the largest |ref| of the quantity on the ray) per element; 0 / 0 = 0, a non-finite value or an
    error where the reference and its sensitivity are exactly zero = inf"""
    got, ref, kap = (np.asarray(a, dtype=F64).reshape(len(ref), -1) for a in (got, ref, kap))
    den = kap + FLOOR * np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(err == 0, 0.0, err / den)
    return np.where(np.isfinite(out), out, np.inf)


def _kappa(ref, runs):
    return {m: np.max([np.abs(p[m] - ref[m]) for p in runs], axis=0) for m in ref}


def compared(i, metric):
    """the rays of a batch on which a metric is compared: all of them in the forward direction, all but fwd_only in the adjoints"""
    return np.ones(i.R, dtype=bool) if metric in FWD else ~i.fwd_only


def worst(got, ref, kap, keep):
    n = normalised(got, ref, kap)[keep]
    return float(n.max()) if n.size else 0.0


def margins_of(own):
    return {m: max(8 * v, 1.0) for m, v in own.items()}


@functools.lru_cache(maxsize=None)
def sampler_case(name):
    """(inputs, float64 reference, kappa, the restatement's largest normalised error per metric, margins) of a batch, computed once"""
    i = sampler_inputs(name)
    ref = run_sampler(i, torch.float64)
    shapes = [(i.R, 3), (i.R, 3), (i.R,), (i.R,), (i.R,)]
    kap = _kappa(ref, [run_sampler(i, torch.float64, scale=[1 + FLOOR * s for s in pat]) for pat in _signs([47, i.R], shapes)])
    res = run_sampler(i, torch.float32)
    own = {m: worst(res[m], ref[m], kap[m], compared(i, m.split("/")[0])) for m in ref}
    return i, ref, kap, own, margins_of(own)


# ---- the mix ----------------------------------------------------------------------------------------------------------------------
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F32)


def _mix_plan(name):
    if name == "strata":
        plan = []
        for s, n in MIX_ROW_STRATA.items():
            for k in range(n):
                plan.append((s, k, {"cnt1": 1, "cntm": M_MAX, "anti": 4 + k % 3, "same": 4 + k % 3}.get(s, row_count("general", k))))
        return plan
    R = int(name[1:])
    plan, total, k = [], 0, 0
    names = list(MIX_ROW_STRATA)
    while total < R:
        s = names[k % len(names)] if R > 1 else "general"
        c = min({"cnt1": 1, "cntm": M_MAX}.get(s, row_count("general", k)), R - total)
        plan.append((s, 50 + k, c))
        total += c
        k += 1
    return plan


def _mix_gates(V, L):
    h = (V.astype(F64) + L.astype(F64)) / 2
    n2 = (h * h).sum(-1)
    H = h / np.sqrt(np.maximum(n2, EPS))[:, None]
    return n2, np.abs((V.astype(F64) * H).sum(-1))


@functools.lru_cache(maxsize=None)
def mix_inputs(name):
    """V, f0, diffuse, d_rows [Mb,3], cnt [Mb], row_of_ray [R], row_off, and per ray L, inc, brdf [R,3]; stratum per ray"""
    plan = _mix_plan(name)
    Mb = len(plan)
    cnt = np.array([c for _, _, c in plan], dtype=np.int32)
    rows = np.repeat(np.arange(Mb), cnt)
    R = len(rows)
    rng = np.random.default_rng([53, sum(map(ord, name))])
    V = _unit32(rng.standard_normal((Mb, 3)))
    f0, diffuse = rng.uniform(0, 1, (Mb, 3)).astype(F32), rng.uniform(0, 1, (Mb, 3)).astype(F32)
    for t, (s, k, _) in enumerate(plan):
        if s == "same":
            V[t] = AXES[k % 6]
        if s in ("f0_0", "f0_1"):
            f0[t] = float(s[-1])
        if s in ("diff_0", "diff_1"):
            diffuse[t] = float(s[-1])
    stratum = np.array([s for s, _, _ in plan])[rows]
    L = _unit32(rng.standard_normal((R, 3)))
    fixed = np.isin(stratum, ("anti", "same"))
    L[stratum == "anti"] = -V[rows][stratum == "anti"]
    L[stratum == "same"] = V[rows][stratum == "same"]
    for attempt in range(100):
        n2, c = _mix_gates(V[rows], L)
        bad = ~fixed & ((n2 < CLEAR) | (c < CLEAR) | (c > 1 - CLEAR))
        if not bad.any():
            break
        L[bad] = _unit32(np.random.default_rng([59, attempt]).standard_normal((int(bad.sum()), 3)))
    else:
        raise AssertionError("mix inputs did not come clear")
    return _ro(SimpleNamespace(name=name, R=R, Mb=Mb, V=V, f0=f0, diffuse=diffuse, cnt=cnt, row_of_ray=rows.astype(np.int32),
                               row_off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), L=L,
                               inc=rng.uniform(0, 2, (R, 3)).astype(F32), brdf=rng.uniform(0, 1, (R, 3)).astype(F32),
                               d_rows=rng.standard_normal((Mb, 3)).astype(F32), stratum=stratum, fwd_only=np.zeros(R, dtype=bool)))


def run_mix(i, dt, fault=None, scale=None):
    rows = i.row_of_ray
    ins = [i.V[rows], i.L, i.f0[rows], i.diffuse[rows], i.inc, i.brdf, i.d_rows[rows]]
    ins = [a.astype(F64) * (1 if scale is None else s) for a, s in zip(ins, scale or [1] * 7)]
    V, L, f0, diffuse, inc, brdf = (_t(a, dt).requires_grad_(True) for a in ins[:6])
    contrib = mix(V, L, f0, diffuse, inc, brdf, _t(np.maximum(i.cnt[rows], 1), dt), fault)
    g = torch.autograd.grad((contrib * _t(ins[6], dt)).sum(), [inc, brdf, L, f0, diffuse, V])
    out = dict(zip(MIX_METRICS, (contrib,) + g))
    return {k: v.detach().double().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def mix_case(name):
    i = mix_inputs(name)
    ref = run_mix(i, torch.float64)
    kap = _kappa(ref, [run_mix(i, torch.float64, scale=[1 + FLOOR * s for s in pat]) for pat in _signs([61, i.R], [(i.R, 3)] * 7)])
    res = run_mix(i, torch.float32)
    own = {m: worst(res[m], ref[m], kap[m], np.ones(i.R, dtype=bool)) for m in ref}
    return i, ref, kap, own, margins_of(own)


# ---- ggx_prob alone -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prob_inputs(name):
    """li, lo, h [R,3], r [R] in the local frame (z = normal); stratum per ray.  `strata`: 96 rays of each of PROB_STRATA"""
    R = 96 * len(PROB_STRATA) if name == "strata" else int(name[1:])
    rng = np.random.default_rng([67, R])
    stratum = np.array([PROB_STRATA[k % len(PROB_STRATA)] if R > 1 else "general" for k in range(R)])
    up = lambda n: _unit32(rng.standard_normal((n, 3)) * [1, 1, 0.5] + [0, 0, 1.2])      # noqa: E731
    li, lo = up(R), up(R)
    li[:, 2], lo[:, 2] = np.maximum(np.abs(li[:, 2]), F32(0.05)), np.maximum(np.abs(lo[:, 2]), F32(0.05))
    r = rng.uniform(0.01, 0.5, R).astype(F32)
    k = np.arange(R) // len(PROB_STRATA)
    s = stratum == "back"
    li[s, 2] = -li[s, 2]
    s = stratum == "zero"
    li[s, 2] = np.where(k[s] % 2 == 0, F32(0.0), F32(-0.0))
    s = stratum == "grazing"
    li[s, 2] = (10.0 ** rng.uniform(-9, -3.05, int(s.sum()))).astype(F32)
    s = stratum == "tiny_lo"
    lo[s, 2] = np.choose(k[s] % 4, [F32(1e-9), F32(0.0), F32(-0.3), F32(2.9e-8)])
    s = stratum == "r_eps"
    r[s] = np.choose(k[s] % 4, [F32(EPS), F32(0.0), F32(EPS / 2), F32(2 * EPS)])
    h = _unit32(li.astype(F64) + lo.astype(F64))
    h[(stratum == "r_eps") & (k % 8 >= 4)] = [0, 0, 1]       # the normal itself: q == 1, (1 + lam) invD below EPS
    return _ro(SimpleNamespace(name=name, R=R, li=li, lo=lo, h=h, r=r, stratum=stratum))


def run_prob(i, dt, scale=None):
    ins = [a.astype(F64) * (1 if scale is None else s) for a, s in zip((i.li, i.lo, i.h, i.r), scale or [1] * 4)]
    return {"prob": O.ggx_prob(*(_t(a, dt) for a in ins)).reshape(-1).double().numpy()}


@functools.lru_cache(maxsize=None)
def prob_case(name):
    i = prob_inputs(name)
    ref = run_prob(i, torch.float64)
    kap = _kappa(ref, [run_prob(i, torch.float64, [1 + FLOOR * s for s in pat]) for pat in _signs([71, i.R], [(i.R, 3)] * 3 + [(i.R,)])])
    own = {"prob": worst(run_prob(i, torch.float32)["prob"], ref["prob"], kap["prob"], np.ones(i.R, dtype=bool))}
    return i, ref, kap, own, margins_of(own)


# ---- what tests/test_hip_parity.py allows the same quantity ---------------------------------------------------------------------------
def parity_tolerance(metric, big):
    """big: the largest |reference| of the quantity in the batch.  Sampler: the bound 99.5 % (99 %) of the rays must meet there"""
    m = metric.split("/")[0]
    if m in ("L", "half", "diff", "lpdf", "mipval", "origin"):
        return 2e-6 + 1e-5 * big
    if m in ADJ:
        return 1e-3 * big
    if m == "contrib":
        return 1e-6 + 1e-5 * big                               # (of the row sums; a row's largest ray is no larger)
    return 2e-5 * big                                          # the mix adjoints: atol alone, rtol 2e-4 comes on top there


def median_ray_allowance(ref, kap, margin, keep):
    """the absolute error the margin allows on the ray whose kappa (largest over the quantity's elements) is the batch's median"""
    ref, kap = (np.asarray(a).reshape(len(ref), -1)[keep] for a in (ref, kap))
    k = kap.max(axis=1)
    at = np.argsort(k)[len(k) // 2]
    return margin * (k[at] + FLOOR * np.abs(ref[at]).max())


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def _population(i):
    g = i.g
    pop = {s: int((i.stratum == s).sum()) for s in ROW_STRATA}
    pop.update(z_up=int(i.up_is_z.sum()), x_up=int((~i.up_is_z).sum()), vs_lo=int((g.vsz < 0.999).sum()), vs_hi_side=int((g.vsz >= 0.999).sum()),
               lower=int(g.lower.sum()), upper=int((~g.lower).sum()), upper_scaled=int((~g.lower & (g.vsz < 0.98) & ~g.zero).sum()),
               flipped=int((g.dwn < 0).sum()), kept=int((g.dwn > 0).sum()), fwd_only=int(i.fwd_only.sum()),
               wrapped=int(((i.sobol[i.j_of_ray] + i.off[i.row_of_ray] * F32(0.25)) >= 1).any(axis=1).sum()))
    for q, u in enumerate(RUNGS):
        for half in (0, 1):
            sel = (i.rung == q) & (g.lower == (half == 0))
            pop[f"rung{q}/{'lower' if half == 0 else 'upper'}"] = (int(sel.sum()), int((sel & i.fwd_only).sum()))
    return pop


def test_batches_enter_the_branches_they_are_named_for():
    for name in BATCHES:
        i = sampler_inputs(name)
        pop = _population(i)
        print(name, "R", i.R, "Mb", i.Mb, pop)
        assert i.R == (int(name[1:]) if name != "strata" else i.cnt.sum()) and i.row_off[-1] == i.R and len(i.j_of_ray) == i.R
        assert (np.diff(i.row_of_ray) >= 0).all() and i.row_of_ray.max() == i.Mb - 1 and 0 <= i.j_of_ray.min() and i.j_of_ray.max() < N_TABLE
        assert np.array_equal(np.bincount(i.row_of_ray, minlength=i.Mb), i.cnt) and i.cnt.min() >= 1 and i.cnt.max() <= M_MAX
    i = sampler_inputs("strata")
    pop = _population(i)
    assert 2000 <= i.R <= 6000
    for s in ROW_STRATA:
        assert pop[s] >= 64, (s, pop[s])
    for s in ("z_up", "x_up", "vs_lo", "vs_hi_side", "lower", "upper", "upper_scaled", "flipped", "kept", "wrapped"):
        assert pop[s] >= 64, (s, pop[s])
    assert set(i.cnt.tolist()) >= set(range(1, 9)) | {M_MAX} and i.j_of_ray.max() == N_TABLE - 1
    rows = i.row_of_ray
    on, below = i.stratum == "nz_on", i.stratum == "nz_below"
    assert (np.abs(i.N[rows, 2])[on] == TH).all() and not i.up_is_z[on].any()
    assert (np.abs(i.N[rows, 2])[below] == np.nextafter(TH, F32(0))).all() and i.up_is_z[below].all()
    assert (np.abs(i.N[rows][i.stratum == "pole"]) == [0, 0, 1]).all() and not i.N[rows][i.stratum == "zero"].any()
    assert {-1.0, 1.0} == set(i.N[rows, 2][i.stratum == "pole"].tolist())
    assert (i.r[rows][i.stratum == "r_lo"] == F32(0.01)).all() and (i.r[rows][i.stratum == "r_hi"] == F32(0.5)).all()
    assert i.r.min() >= F32(0.01) and i.r.max() <= F32(0.5)
    assert (i.g.vsz[i.stratum == "vs_hi"] >= 0.999).mean() > 0.9
    for q, u in enumerate(RUNGS):                            # every rung on both halves, with exactly the rung's u1
        assert (i.u1[i.rung == q] == F32(u)).all()
        for half in ("lower", "upper"):
            assert pop[f"rung{q}/{half}"][0] >= 32, (q, half)
    # lower half: 1 - P1^2 - P2^2 = 1 - u1, below CLEAR from the rung 0.999 on (1 - float32(0.999) = 0.99999e-3); upper half: all in full
    assert all(pop[f"rung{q}/lower"][1] == (0 if q < 4 else pop[f"rung{q}/lower"][0]) and pop[f"rung{q}/upper"][1] == 0 for q in range(7))
    assert pop["rung6/lower"][1] == pop["rung6/lower"][0] and (i.g.w3sq[(i.rung == 6) & i.g.lower] < EPS).all()
    assert (i.fwd_only <= i.ladder_ray).all()                # off the ladder nothing is compared forward only
    for name in BATCHES[1:4]:                                # the batches around one block hold every row stratum too
        assert set(sampler_inputs(name).stratum.tolist()) == set(ROW_STRATA)
    m = mix_inputs("strata")
    for s in MIX_ROW_STRATA:
        assert (m.stratum == s).sum() >= 64, s
    rows = m.row_of_ray
    assert (m.L[m.stratum == "anti"] == -m.V[rows][m.stratum == "anti"]).all() and (m.L[m.stratum == "same"] == m.V[rows][m.stratum == "same"]).all()
    assert (m.cnt[rows][m.stratum == "cnt1"] == 1).all() and (m.cnt[rows][m.stratum == "cntm"] == M_MAX).all()
    for s, col in (("f0_0", m.f0), ("f0_1", m.f0), ("diff_0", m.diffuse), ("diff_1", m.diffuse)):
        assert (col[rows][m.stratum == s] == float(s[-1])).all()
    p = prob_inputs("strata")
    assert all((p.stratum == s).sum() >= 64 for s in PROB_STRATA)
    assert (p.li[p.stratum == "back", 2] < 0).all() and (p.li[p.stratum == "zero", 2] == 0).all()
    assert (p.li[p.stratum == "grazing", 2].astype(F64) ** 2 < 1e-6).all() and (p.li[p.stratum == "grazing", 2] > 0).all()
    assert (4 * p.lo[p.stratum == "tiny_lo", 2].astype(F64) < EPS).all() and (p.r[p.stratum == "r_eps"] <= F32(2 * EPS)).all()


@pytest.mark.parametrize("name", BATCHES)
def test_every_gate_is_clear_or_exact(name):
    i = sampler_inputs(name)
    bad, g = gate_report(i.V, i.N, i.r, i.off, i.row_of_ray, i.j_of_ray, i.ladder_ray)
    assert not bad.any() and np.array_equal(g.u1, i.u1) and np.array_equal(g.u2, i.u2)
    live = ~g.zero
    d = {"Vs.z below": (0.999 - g.vsz[live & (g.vsz < 0.999)]).min(initial=np.inf), "Vs.z above": (g.vsz[g.vsz >= 0.999] - 0.999).min(initial=np.inf),
         "u2 - a": np.abs(g.u2.astype(F64) - g.a)[live].min(initial=np.inf), "dot(wi, N)": np.abs(g.dwn[live]).min(initial=np.inf),
         "w3^2 off the ladder": g.w3sq[~i.ladder_ray].min(initial=np.inf), "li.z^2 - 1e-6": (g.llz[live] ** 2 - 1e-6).min(initial=np.inf),
         "4 lo.z": 4 * g.ndv[live].min(initial=np.inf)}
    print(name, {k: float(v) for k, v in d.items()}, "zero-normal rays", int(g.zero.sum()))
    assert all(v >= CLEAR for k, v in d.items() if k != "Vs.z above") and d["Vs.z above"] >= CLEAR / 2 - 1e-12
    assert (g.vsz[g.zero] == 0).all() and (g.a[g.zero] == 1).all() and (g.dwn[g.zero] == 0).all()
    # the fp32 restatement takes every decision the way float64 does
    with torch.no_grad():
        s = sample_rays(_t(i.V[i.row_of_ray], torch.float32), _t(i.N[i.row_of_ray], torch.float32), _t(i.r[i.row_of_ray], torch.float32),
                        _t(i.u1, torch.float32), _t(i.u2, torch.float32), torch.from_numpy(np.array(i.up_is_z)))
    assert np.array_equal(s.lower.numpy(), g.lower) and np.array_equal(s.vsz.numpy() < TH, g.vsz < 0.999)
    assert np.array_equal(s.dwn.numpy() > 0, g.dwn > 0)
    m = mix_inputs(name)
    n2, c = _mix_gates(m.V[m.row_of_ray], m.L)
    anti, same = m.stratum == "anti", m.stratum == "same"
    assert (n2[anti] == 0).all() and (c[anti] == 0).all() and (n2[same] == 1).all() and (c[same] == 1).all()
    rest = ~(anti | same)
    assert n2[rest].min(initial=1) >= CLEAR and c[rest].min(initial=1) >= CLEAR and c[rest].max(initial=0) <= 1 - CLEAR


def test_per_ray_definition_is_the_oracle():
    """sample_rays in float32 on the expanded rows against oracle.ggx_sample on the padded [rows, m] layout with the same u: every
    element inside the margin of the batch (the two differ in the association of a few dot products only)"""
    i, ref, kap, own, mg = sampler_case("strata")
    u1, u2 = np.zeros((i.Mb, M_MAX), dtype=F32), np.zeros((i.Mb, M_MAX), dtype=F32)
    loc = np.arange(i.R) - i.row_off[:-1][i.row_of_ray]
    u1[i.row_of_ray, loc], u2[i.row_of_ray, loc] = i.u1, i.u2
    mask = torch.from_numpy(np.arange(M_MAX)[None] < i.cnt[:, None])
    N = torch.from_numpy(i.N.copy()).requires_grad_(True)
    L, basisT, lp = O.ggx_sample(torch.from_numpy(u1), torch.from_numpy(u2), torch.from_numpy(i.V.copy()), N,
                                 torch.from_numpy(i.r.copy()).reshape(-1, 1), mask)
    (gN,) = torch.autograd.grad((L * torch.from_numpy(i.dL.copy())).sum(), [N])
    every = np.ones(i.R, dtype=bool)
    print("oracle.ggx_sample in float32: L", worst(L.detach().numpy(), ref["L"], kap["L"], every), "lpdf", worst(lp.numpy(), ref["lpdf"], kap["lpdf"], every))
    assert worst(L.detach().numpy(), ref["L"], kap["L"], every) <= mg["L"]
    assert worst(lp.numpy(), ref["lpdf"], kap["lpdf"], every) <= mg["lpdf"]
    # its row gradient = the sum of the per-ray adjoints, within the sum of what the margin allows each ray (rows without a
    # forward-only ray)
    allow = mg["dN/dL"] * (kap["dN/dL"] + FLOOR * np.abs(ref["dN/dL"]).max(axis=1, keepdims=True))
    rows64, rows_allow = np.zeros((i.Mb, 3)), np.zeros((i.Mb, 3))
    np.add.at(rows64, i.row_of_ray, ref["dN/dL"])
    np.add.at(rows_allow, i.row_of_ray, allow)
    clean = np.ones(i.Mb, dtype=bool)
    clean[i.row_of_ray[i.fwd_only]] = False
    assert (np.abs(gN.numpy() - rows64)[clean] <= rows_allow[clean] + 1e-30).all()


def test_restatement_ratios_and_margins():
    for name in BATCHES:
        for what, case in (("sampler", sampler_case), ("mix", mix_case), ("ggx_prob", prob_case)):
            i, ref, kap, own, mg = case(name)
            for m in own:
                floor = "  (floor)" if mg[m] == 1.0 else ""
                print(f"{what} {name} {m}: restatement {own[m]:.3g} margin {mg[m]:.3g}{floor}")
                assert np.isfinite(own[m]) and mg[m] >= 8 * own[m] and np.isfinite(ref[m]).all(), (what, name, m)


def test_zero_normal_rows_and_exact_corners():
    """N = 0: L = V / |V|, local vectors 0, lpdf = log EPS, adjoints of N and r exactly zero in float64 and in float32;  u1 == 0:
    the sampled half vector is the stretched view direction whatever u2;  L == -V: Fr = 1, contrib = inc brdf / count, dL = dV = 0"""
    i, ref, kap, own, mg = sampler_case("strata")
    z = i.stratum == "zero"
    V = i.V[i.row_of_ray][z].astype(F64)
    assert np.allclose(ref["L"][z], V / np.linalg.norm(V, axis=1, keepdims=True), rtol=1e-15) and not ref["half"][z].any()
    assert np.allclose(ref["lpdf"][z], math.log(EPS)) and not ref["dr/both"][z].any() and not ref["dN/both"][z].any()
    res = run_sampler(i, torch.float32)
    assert all(np.isfinite(v).all() for v in res.values())
    m, mref, _, _, _ = mix_case("strata")
    a = m.stratum == "anti"
    want = m.inc[a].astype(F64) * m.brdf[a].astype(F64) / m.cnt[m.row_of_ray][a][:, None]
    assert np.allclose(mref["contrib"][a], want, rtol=1e-15) and not mref["dL"][a].any() and not mref["dV"][a].any()
    s = m.stratum == "same"
    assert not mref["dL"][s].any() and not mref["dV"][s].any()           # om_raw == 0: the closed side passes 5 om^4 = 0
    p, pref, _, _, _ = prob_case("strata")
    assert (pref["prob"][np.isin(p.stratum, ("back", "zero"))] == 0).all() and (pref["prob"][p.stratum == "grazing"] > 0).all()


def test_margins_are_not_looser_than_the_fp32_tests():
    """on the ray of median kappa, the absolute error the margin allows is below what tests/test_hip_parity.py allows the quantity"""
    for name in BATCHES[1:]:
        for what, case in (("sampler", sampler_case), ("mix", mix_case)):
            i, ref, kap, own, mg = case(name)
            for m in own:
                keep = compared(i, m.split("/")[0]) if what == "sampler" else np.ones(i.R, dtype=bool)
                allowed = median_ray_allowance(ref[m], kap[m], mg[m], keep)
                old = parity_tolerance(m, float(np.abs(ref[m]).max()))
                print(f"{what} {name} {m}: allows {allowed:.3e} on the median ray, the fp32 test {old:.3e}")
                assert allowed < old, (what, name, m, allowed, old)


def _miss(run, case, fault, metric, stratum_of):
    i, ref, kap, own, mg = case("strata")
    got = run(i, torch.float32, fault=fault)
    keep = stratum_of(i) & (compared(i, metric.split("/")[0]) if metric.split("/")[0] in FWD + ADJ else True)
    assert keep.sum() >= 64
    return worst(got[metric], ref[metric], kap[metric], keep) / mg[metric]


BREAKS = (
    ("Vs.z factor of P2 dropped", run_sampler, sampler_case, "p2", "L", lambda i: ~i.g.lower & ~i.g.zero & (i.g.vsz < 0.98), "upper half"),
    ("a not detached", run_sampler, sampler_case, "a", "dN/dL", lambda i: np.isin(i.stratum, ("general", "r_hi", "wrap")), "general rows"),
    ("a not detached", run_sampler, sampler_case, "a", "dr/dL", lambda i: np.isin(i.stratum, ("general", "r_hi", "wrap")), "general rows"),
    ("sign flip ignored in the adjoint", run_sampler, sampler_case, "sign", "dN/both", lambda i: (i.g.dwn < 0), "flipped rays"),
    ("sign flip ignored in the adjoint", run_sampler, sampler_case, "sign", "dV/both", lambda i: (i.g.dwn < 0), "flipped rays"),
    ("x_up frame just below 0.999", run_sampler, sampler_case, "frame", "half", lambda i: i.stratum == "nz_below", "nz_below"),
    ("x_up frame just below 0.999", run_sampler, sampler_case, "frame", "dN/dL", lambda i: i.stratum == "nz_below", "nz_below"),
    ("5e-3 d_rays[0:3] dropped", run_sampler, sampler_case, "origin", "dN/rays", lambda i: i.stratum == "general", "general rows"),
    ("5e-3 d_rays[0:3] dropped", run_sampler, sampler_case, "origin", "dr/rays", lambda i: i.stratum == "general", "general rows"),
    ("Fresnel dV without -dd H", run_mix, mix_case, "direct", "dV", lambda i: np.isin(i.stratum, ("general", "cnt1", "cntm")), "general rows"),
    ("mix dL without s hd H", run_mix, mix_case, "proj", "dL", lambda i: np.isin(i.stratum, ("general", "cnt1", "cntm")), "general rows"),
)


def test_broken_restatements_miss_their_margins():
    for label, run, case, fault, metric, stratum_of, where in BREAKS:
        f = _miss(run, case, fault, metric, stratum_of)
        print(f"{label}: {metric} on the {where}: {f:.3g} x margin")
        assert f > 1.0, (label, metric, f)
