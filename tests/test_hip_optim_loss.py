"""The kernels that close every training step on the GPU -- k_adam and k_multi_copy (csrc/adam.hip), the loss kernels (csrc/loss.hip) --
against the float64 references and within the bounds of tests/test_optim_loss_cpu.py, at the sizes where their control flow changes: the
second and third pass of every grid-stride loop, the hand-over from the float4 loop to the scalar tail, slot tables that span two and
three launches, the scalar path of misaligned pointers, both lerp branches, fp64 slots of more than one element.

Adam runs through hip.adam_step on hand-built AdamSlot tables whose arrays lie in one buffer each, every array between two guard regions
of 64 elements (Arena), so pointers and alignment are the test's.  Every step is checked per element from the device's own fp32 state
against E_p / E_m / E_v; the copies and the backward kernels are checked bit for bit; the forward reductions against float64 within the
bound of their summation shape, and on one-hot tensors (one element at the first / last index of every pass) against the exactly known
result, which is what notices a single dropped or doubled element.

The bounds rest on these flags of csrc/build.sh: -fno-fast-math and hipcc's default correctly rounded fp32 divide / sqrt (Adam's quotient
and root carry one rounding each), no denormal flush (the 2^-149 terms), default fp contraction (a fused multiply-add removes a rounding).
Worst device-to-bound ratios on the MI355X (printed by every test):

    Adam m / v / p (correctly rounded divide and sqrt, denormals kept, contraction on; no denormal moment was flushed to zero)
      float4 path, 11 sizes up to 2 097 159           0.985  0.790  0.986
      scalar path (bits of the float4 path)           0.985  0.787  0.987
      mixed launch, 2 160 000 + fp64 + misaligned     0.999  0.788  0.991
      40 / 41 / 80 / 81 slots                         0.875  0.711  0.974
      54 hyperparameter sets x 6 regimes              0.955  0.720  0.977
      chained, 4 steps                                0.789  0.712  0.942
      non-finite gradients' neighbours                0.842  0.616  0.747
      FusedAdam, 45 parameters, 3 steps               0.836  0.635  0.971
    reductions (fp32 adds, then float atomics in any order: the bound of the summation shape)
      l1_mean_fwd 0.0040   loss_mix_fwd 0.0017   sqerr_fwd 0.0102   loss_head 0.0501
    copies, backward kernels, one-hot sums: equal bits.

A scratch build with one line changed turns these red while every test of test_hip_parity.py that reaches the two files stays green:
`i += stride + 1` in adam_slot's float4 loop (float4 sizes beyond one pass, the mixed launch), `slots[0 + i]` in nmf_adam_step (41, 80, 81
slots, the hyperparameter grid, FusedAdam), a cap of 255 workgroups in blocks_for under a stride that still assumes 256 (l1 / mix forward
and backward at every size).
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nmf_amd import hip
from test_optim_loss_cpu import (F32, F64, HEAD_RAYS, HYPERS, L1_SETS, REGIMES, SQERR_RAYS, adam_ref, head_const_f32, head_ref, hyper,
                                 l1_bwd_f32, l1_inputs, l1_ref, make_mixed, make_state, mix_ref, one_hot_positions, prints,
                                 random_hyper, ratios, same_bits, sqerr_bwd_f32, sqerr_inputs, sqerr_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ZERO = list(REGIMES).index("all_zero")


class Arena:
    """one device buffer that holds many arrays, each between two guard regions of 64 of its elements; mis: bytes off 16-byte alignment"""
    FILL = 0xA5

    def __init__(self):
        self.parts, self.size, self.dev = [], 0, None

    def add(self, arr, mis=0):
        arr = np.ascontiguousarray(arr)
        guard = 64 * arr.itemsize
        off = -(-(self.size + guard) // 16) * 16 + mis
        self.parts.append((off, arr))
        self.size = off + arr.nbytes + guard
        return len(self.parts) - 1

    def upload(self):
        self.host = np.full(self.size + 16, self.FILL, np.uint8)
        self.data = np.zeros(self.host.size, bool)
        for off, a in self.parts:
            self.host[off:off + a.nbytes] = np.frombuffer(a.tobytes(), np.uint8)
            self.data[off:off + a.nbytes] = True
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, i):
        return self.dev.data_ptr() + self.parts[i][0]

    def download(self):
        after = self.dev.cpu().numpy()
        assert np.array_equal(after[~self.data], self.host[~self.data]), "a guard region was written"
        return [np.frombuffer(after[off:off + a.nbytes].tobytes(), a.dtype) for off, a in self.parts]


def case(p, g, m, v, h, mis=(0, 0, 0, 0), which=None):
    return SimpleNamespace(p=p, g=g, m=m, v=v, h=h, mis=mis, which=which)


def mixed_case(n, h, rng, mis=(0, 0, 0, 0)):
    p, g, m, v, which = make_mixed(n, h.weight_decay, rng)
    return case(p, g, m, v, h, mis, which)


def run_adam(cases):
    """one hip.adam_step over the cases' slots -> [(p', m', v')]; the gradients and every guard region must be unchanged"""
    arenas = [Arena() for _ in range(4)]
    for c in cases:
        for a, x, mis in zip(arenas, (c.p, c.g, c.m, c.v), c.mis):
            a.add(x, mis)
    for a in arenas:
        a.upload()
    slots = (hip.AdamSlot * len(cases))()
    for i, c in enumerate(cases):
        s, h = slots[i], c.h
        s.param, s.grad, s.exp_avg, s.exp_avg_sq = (a.ptr(i) for a in arenas)
        s.numel, s.is_f64 = c.p.size, int(c.p.dtype == F64)
        s.beta1, s.beta2, s.eps, s.weight_decay, s.step_size, s.bc2_sqrt = (h.beta1, h.beta2, h.eps, h.weight_decay, h.step_size,
                                                                            h.bc2_sqrt)
    hip.adam_step(slots, len(cases))
    torch.cuda.synchronize()
    P, G, M, V = (a.download() for a in arenas)
    assert all(same_bits(g, c.g) for g, c in zip(G, cases)), "a gradient was written"
    return list(zip(P, M, V))


def hold(cases, outs, what):
    """every element of every slot against its bound; all-zero elements keep their bits"""
    worst, flushed = dict.fromkeys("pmv", 0.0), 0
    for i, (c, got) in enumerate(zip(cases, outs)):
        ref = adam_ref(c.p, c.g, c.m, c.v, c.h, f64_slot=c.p.dtype == F64)
        flushed += sum(int(((x == 0) & (np.abs(r) >= 2.0 ** -148)).sum()) for x, r in zip(got[1:], ref[1:3])) if c.p.dtype == F32 else 0
        r = ratios(got, ref)
        for k in r:
            worst[k] = max(worst[k], r[k])
        assert max(r.values()) <= 1.0, (what, i, c.p.size, vars(c.h), r, f"{flushed} moments flushed to zero")
        if c.which is not None:
            z = c.which == ZERO
            assert all(same_bits(a[z], b[z]) for a, b in zip(got, (c.p, c.m, c.v))), (what, i, "all-zero elements changed")
    prints(f"{what}: device / bound  m {worst['m']:.3f}  v {worst['v']:.3f}  p {worst['p']:.3f}  ({len(cases)} slots, "
           f"{sum(c.p.size for c in cases)} elements, {flushed} denormal moments flushed to zero)")
    assert flushed == 0
    return worst


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------
FLOAT4_SIZES = (1, 2, 3, 4, 5, 1023, 1025, 1048576, 1048580, 1440000, 2 * 1048576 + 7)


@pytest.mark.parametrize("n", FLOAT4_SIZES)
def test_adam_float4_path_sizes(n):
    """all four pointers 16-byte aligned: float4 loop, `done = n4 << 2`, scalar tail; one pass is 1 048 576 elements"""
    i = FLOAT4_SIZES.index(n)
    c = mixed_case(n, HYPERS[(5 * i + 1) % len(HYPERS)], np.random.default_rng([11, n]))
    hold([c], run_adam([c]), f"adam float4 n {n}")


@pytest.mark.parametrize("n", (5, 262144, 262145, 600001))
def test_adam_scalar_path_gives_the_bits_of_the_float4_path(n):
    """each of p, g, m, v in turn a [1:] slice of a larger buffer (4 bytes off): the scalar loop, 262 144 elements per pass"""
    h = HYPERS[{5: 0, 262144: 13, 262145: 26, 600001: 41}[n]]
    c0 = mixed_case(n, h, np.random.default_rng([12, n]))
    cases = [c0] + [case(c0.p, c0.g, c0.m, c0.v, h, tuple(4 * (j == k) for j in range(4)), c0.which) for k in range(4)]
    outs = run_adam(cases)
    hold(cases[:1], outs[:1], f"adam aligned n {n}")
    for k, o in enumerate(outs[1:]):
        assert all(same_bits(a, b) for a, b in zip(o, outs[0])), f"{'pgmv'[k]} misaligned: other bits than the aligned form"


def test_adam_mixed_launch():
    """a grid sized by the biggest slot, the early exit of the others, an empty slot, the fp64 loop's second pass, a misaligned slot"""
    rng = np.random.default_rng(13)
    hs = [HYPERS[i] for i in (2, 17, 30, 9, 52, 44)]
    cases = [mixed_case(2160000, hs[0], rng), mixed_case(5, hs[1], rng), mixed_case(0, hs[2], rng),
             case(*make_state(1, "ordinary", hs[3].weight_decay, rng, F64), hs[3]),
             case(*make_state(300001, "ordinary", hs[4].weight_decay, rng, F64), hs[4]),
             mixed_case(70001, hs[5], rng, mis=(4, 4, 4, 4))]
    hold(cases, run_adam(cases), "adam mixed launch")


@pytest.mark.parametrize("n_slots", (40, 41, 80, 81))
def test_adam_slot_tables_across_launches(n_slots):
    """nmf_adam_step launches 40 slots at a time: the `base` offset of the second and third launch; every slot has its own row"""
    rng = np.random.default_rng([14, n_slots])
    cases = [mixed_case(1 + 2 * ((5 * i) % 49), random_hyper(rng), rng) for i in range(n_slots)]
    assert len({c.p.size for c in cases}) == min(n_slots, 49) and max(c.p.size for c in cases) == 97
    hold(cases, run_adam(cases), f"adam {n_slots} slots")


def test_adam_every_hyperparameter_set_in_every_regime():
    """beta1 x beta2 x weight decay x step count (both lerp branches and their boundary) x the six regimes of (g, m, v)"""
    for regime in REGIMES:
        rng = np.random.default_rng([15, list(REGIMES).index(regime)])
        cases = [case(*make_state(133, regime, h.weight_decay, rng), h) for h in HYPERS]
        outs = run_adam(cases)
        hold(cases, outs, f"adam regime {regime}")
        if regime == "all_zero":
            for c, o in zip(cases, outs):
                assert all(same_bits(a, b) for a, b in zip(o, (c.p, c.m, c.v)))


def test_adam_chained_steps_from_the_device_state():
    """one gradient, then three zero gradients: the reference of step k starts from the device's fp32 state after step k - 1"""
    rng = np.random.default_rng(16)
    h0s = [h for h in HYPERS if h.t == 1]
    state = []
    for h in h0s:
        p, g, m, v = make_state(1029, "ordinary", h.weight_decay, rng)
        state.append([p, g, np.zeros_like(m), np.zeros_like(v)])
    for t in range(1, 5):
        cases = [case(s[0], s[1] if t == 1 else np.zeros_like(s[1]), s[2], s[3], hyper(h.beta1, h.beta2, h.weight_decay, t))
                 for s, h in zip(state, h0s)]
        outs = run_adam(cases)
        hold(cases, outs, f"adam chained step {t}")
        for s, (p, m, v) in zip(state, outs):
            s[0], s[2], s[3] = p, m, v


def test_adam_non_finite_gradients_keep_their_elements():
    """inf and NaN in each of the four positions of a float4 group and in the scalar tail: p, m, v keep their bits, the neighbours move"""
    rng = np.random.default_rng(17)
    n = 4 * 40 + 3
    cases = []
    for h in (HYPERS[0], HYPERS[28]):
        p, g, m, v = make_state(n, "ordinary", h.weight_decay, rng)
        for q in range(4):
            g[4 * (2 * q) + q], g[4 * (2 * q + 1) + q] = np.inf, np.nan
        g[4 * 9 + 2], g[n - 1], g[n - 3] = -np.inf, np.inf, np.nan
        cases += [case(p, g, m, v, h), case(p, g, m, v, h, mis=(0, 4, 0, 0))]
    outs = run_adam(cases)
    hold(cases, outs, "adam non-finite")                 # (a bound of 0: equal)
    for c, o in zip(cases, outs):
        bad = ~np.isfinite(c.g)
        assert bad.sum() == 11 and all(same_bits(a[bad], b[bad]) for a, b in zip(o, (c.p, c.m, c.v)))
        assert (o[0][~bad] != c.p[~bad]).mean() > 0.9 and (o[2][~bad] != c.v[~bad]).all()


def test_fused_adam_writes_a_table_of_two_launches():
    """FusedAdam over 45 parameters in 5 groups: the table of _step_checked, then of _step_planned (steps 2 and 3), 40 + 5 slots"""
    from nmf_amd.optim import FusedAdam
    rng = np.random.default_rng(18)
    sizes = [1 + 2 * ((7 * i) % 49) for i in range(45)]
    params = [torch.nn.Parameter(torch.from_numpy((0.5 * rng.standard_normal(n)).astype(F64 if i == 43 else F32)).to(DEV))
              for i, n in enumerate(sizes)]
    conf = [dict(lr=0.02, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0), dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-7, weight_decay=0.01),
            dict(lr=0.5, betas=(0.3, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02),
            dict(lr=1e-4, betas=(0.95, 0.9), eps=1e-8, weight_decay=0.001)]
    opt = FusedAdam([dict(params=params[9 * k:9 * k + 9], **conf[k]) for k in range(5)])
    checked, inner = [], opt._step_checked
    opt._step_checked = lambda: (checked.append(1), inner())[1]
    for p in params:
        p.grad = torch.zeros_like(p)
    worst = dict.fromkeys("pmv", 0.0)
    for t in (1, 2, 3):
        for i, p in enumerate(params):
            g = 1e-2 * rng.standard_normal(p.numel()) * ((i + t) % 3 != 0)            # a third of the gradients are zero
            p.grad.copy_(torch.from_numpy(g.astype(F64 if i == 43 else F32)))
        before = []
        for p in params:
            st = opt.state.get(p, {})
            before.append([p.detach().cpu().numpy().copy(), p.grad.cpu().numpy().copy()] +
                          [st[k].cpu().numpy().copy() if k in st else np.zeros(p.numel(), p.detach().cpu().numpy().dtype)
                           for k in ("exp_avg", "exp_avg_sq")])
        opt.step()
        torch.cuda.synchronize()
        for i, (p, b) in enumerate(zip(params, before)):
            c = conf[i // 9]
            h = SimpleNamespace(beta1=c["betas"][0], beta2=c["betas"][1], eps=c["eps"], weight_decay=c["weight_decay"],
                                step_size=c["lr"] / (1 - c["betas"][0] ** t), bc2_sqrt=math.sqrt(1 - c["betas"][1] ** t))
            got = (p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy())
            r = ratios(got, adam_ref(*b, h, f64_slot=i == 43))
            assert max(r.values()) <= 1.0, (t, i, r)
            assert int(opt.state[p]["step"]) == t
            for k in r:
                worst[k] = max(worst[k], r[k])
    assert len(checked) == 1 and opt._plan is not None   # steps 2 and 3 went through _step_planned
    prints(f"FusedAdam 45 parameters: device / bound  m {worst['m']:.3f}  v {worst['v']:.3f}  p {worst['p']:.3f}")


# ---- nmf_multi_copy ------------------------------------------------------------------------------------------------------------------
def _copy(triples):
    """one hip.multi_copy: (src pointer, dst pointer, numel, src_is_f64, dst code) per slot"""
    slots = (hip.CopySlot * max(len(triples), 1))()
    for i, t in enumerate(triples):
        slots[i] = hip.CopySlot(*t)
    hip.multi_copy(slots, len(triples))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_slots", (96, 97, 193))
def test_multi_copy_across_launches_and_passes(n_slots):
    """96 slots per launch, 262 144 elements per pass; pack fp32 -> flat fp32 and fp32 -> flat fp64 at consecutive (4-byte) offsets as
    the trainer lays its gradients out, unpack fp64 -> fp32: bit for bit, guard regions untouched"""
    rng = np.random.default_rng([19, n_slots])
    sizes = [1 + 2 * ((5 * i) % 49) for i in range(n_slots)]
    sizes[0], sizes[n_slots // 2], sizes[n_slots - 1] = 262145, 1440000, 262144
    src = Arena()
    for n in sizes:
        x = rng.standard_normal(n).astype(F32)
        x[:min(n, 5)] = np.array([-0.0, np.inf, 1e-40, -3e-39, 3.4e38], F32)[:min(n, 5)]
        src.add(x)
    src.upload()
    total = sum(sizes)
    flat32, flat64, back = Arena(), Arena(), Arena()
    flat32.add(np.full(total + 1, np.nan, F32))
    flat64.add(np.full(total + 1, np.nan, F64))
    for n in sizes:
        back.add(np.full(n, np.nan, F32))
    for a in (flat32, flat64, back):
        a.upload()
    offs = np.concatenate([[1], 1 + np.cumsum(sizes)[:-1]])          # the flat buffers start one element in: 4 / 8 bytes off
    _copy([(src.ptr(i), flat32.ptr(0) + 4 * int(o), n, 0, 0) for i, (n, o) in enumerate(zip(sizes, offs))])
    _copy([(src.ptr(i), flat64.ptr(0) + 8 * int(o), n, 0, 1) for i, (n, o) in enumerate(zip(sizes, offs))])
    want = np.concatenate([a for _, a in src.parts])
    got32, got64 = flat32.download()[0], flat64.download()[0]
    assert np.isnan(got32[0]) and same_bits(got32[1:], want)
    assert np.isnan(got64[0]) and same_bits(got64[1:], want.astype(F64))
    _copy([(flat64.ptr(0) + 8 * int(o), back.ptr(i), n, 1, 0) for i, (n, o) in enumerate(zip(sizes, offs))])
    for i, (got, (_, a)) in enumerate(zip(back.download(), src.parts)):
        assert same_bits(got, a), i
    src.download()                                                    # (the sources and their guards are unchanged)


def test_multi_copy_fp64_to_fp32_rounds_like_numpy():
    rng = np.random.default_rng(20)
    e = 2.0 ** -24
    x = np.concatenate([
        [1 + e, 1 + 3 * e, 1 + e + 2.0 ** -50, 1 + e - 2.0 ** -52, -(1 + e), 1e39, -1e39, 1e-46, -1e-46, 1e-40, 2.0 ** -149 * 1.5,
         2.0 ** -149 * 2.5, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -40), 2.0 ** -126 * (1 - 2.0 ** -25),
         float(np.finfo(F32).max) * (1 + 2.0 ** -25), float(np.finfo(F32).max) * (1 + 2.0 ** -26), np.inf, -np.inf, 0.0, -0.0],
        rng.standard_normal(3000) * 10.0 ** rng.uniform(-44, 38, 3000), 1 + e * rng.integers(0, 64, 1000)])
    with np.errstate(over="ignore", under="ignore"):
        want = x.astype(F32)
    a, b = Arena(), Arena()
    a.add(x)
    b.add(np.zeros(x.size, F32), mis=4)
    a.upload(), b.upload()
    _copy([(a.ptr(0), b.ptr(0), x.size, 1, 0)])
    got = b.download()[0]
    assert same_bits(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:10]


def test_multi_copy_fp32_to_bf16_every_upper_half():
    """all 65 536 upper halves x the lower halves at and around the tie: the bits of torch's CPU conversion; a NaN stays a NaN of its sign"""
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    bits = (hi | np.array([0x0000, 0x7fff, 0x8000, 0x8001, 0xffff], np.uint32)[None, :]).reshape(-1)
    assert bits.size == 327680
    x = torch.from_numpy(bits.view(F32).copy())
    want = x.bfloat16().view(torch.int16).numpy().view(np.uint16)
    src = x.to(DEV)
    (dst,) = hip.to_bf16_tables([src])
    torch.cuda.synchronize()
    got = dst.view(torch.int16).cpu().numpy().view(np.uint16)
    nan = np.isnan(bits.view(F32))
    assert same_bits(got[~nan], want[~nan]), np.flatnonzero((got != want) & ~nan)[:10]
    assert ((got[nan] & 0x7fff) > 0x7f80).all() and ((got[nan] >> 15) == (bits[nan] >> 31)).all()
    assert same_bits(src.cpu().numpy().view(np.uint32), bits)


# ---- loss kernels --------------------------------------------------------------------------------------------------------------------
PER_PASS = 256 * 256                                    # the l1 / mix / sqerr kernels at their cap of 256 workgroups


def _dev(x):
    """a device tensor with x's memory: channels-last [1, 16, H, W] where the size allows it, flat otherwise"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if x.size >= 4096 and x.size % 4800 == 0:
        return t.view(1, 300, x.size // 4800, 16).permute(0, 3, 1, 2)
    if x.size >= 4096 and x.size % 2048 == 0:
        return t.view(1, 128, x.size // 2048, 16).permute(0, 3, 1, 2)
    return t


def _scalar(v):
    return torch.full((), float(v), dtype=torch.float32, device=DEV)


def _raw(t):
    """a tensor's floats in memory order"""
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).reshape(-1).cpu().numpy()


@pytest.mark.parametrize("sizes", L1_SETS)
def test_l1_mean_and_loss_mix_forward_against_float64(sizes):
    rng = np.random.default_rng([21, sizes[0]])
    xs = [l1_inputs(n, rng) for n in sizes]
    td = [_dev(x) for x in xs]
    assert td[sizes.index(max(sizes))].dim() == (4 if max(sizes) % 16 == 0 else 1)
    val, bound = l1_ref(xs)
    got = float(hip.l1_mean_fwd(td))
    prints(f"l1_mean_fwd {sizes}: device / bound {abs(got - val) / bound:.4f}")
    assert abs(got - val) <= bound
    ys = [(rng.standard_normal(n) + 0.25).astype(F32) for n in sizes]
    ws, scale = [0.37, -1.3, 0.013, 2.0][:len(ys)], 1.0 / 7.0
    val, bound = mix_ref(ys, [F32(w) for w in ws], F32(scale))
    val64, _ = mix_ref(ys, ws, scale)
    got = float(hip.loss_mix_fwd([_dev(y) for y in ys], ws, scale))
    prints(f"loss_mix_fwd {sizes}: device / bound {abs(got - val64) / bound:.4f}")
    assert abs(got - val64) <= bound and abs(got - val) <= bound
    # one element at the edges of every pass: an exactly known sum
    n = max(sizes)
    hot = torch.zeros(n, device=DEV)
    others = [torch.zeros(m, device=DEV) for m in sizes if m != n]
    for k in one_hot_positions(n, PER_PASS):
        hot[k] = -1.5
        assert same_bits(hip.l1_mean_fwd([hot] + others).cpu().numpy(), F32(1.5) / F32(n)), k
        assert same_bits(hip.loss_mix_fwd(others + [hot], [0.5] * len(others) + [0.37], scale).cpu().numpy(),
                         F32(F32(-1.5) * F32(0.37)) * F32(scale)), k
        hot[k] = 0.0


@pytest.mark.parametrize("sizes", L1_SETS)
def test_l1_mean_backward_bits(sizes):
    """+-fp32(d_out / fp32(n)), 0 for +-0.0; the accumulate form is one fp32 add; flat and channels-last storage"""
    rng = np.random.default_rng([22, sizes[0]])
    xs = [l1_inputs(n, rng) for n in sizes]
    td = [_dev(x) for x in xs]
    d_out = F32(0.731)
    grads = hip.l1_mean_bwd(td, _scalar(d_out))
    for x, t, g in zip(xs, td, grads):
        assert g.stride() == t.stride() or x.size <= 1
        assert same_bits(_raw(g), l1_bwd_f32(x, d_out)), x.size
    before = [rng.standard_normal(n).astype(F32) * F32(1e-6) for n in sizes]
    acc = [_dev(b) for b in before]
    hip.l1_mean_bwd(td, _scalar(d_out), out=acc)
    for x, b, g in zip(xs, before, acc):
        assert same_bits(_raw(g), l1_bwd_f32(x, d_out, before=b)), x.size
    for x, t in zip(xs, td):
        assert same_bits(_raw(t), x)


@pytest.mark.parametrize("sizes", L1_SETS)
def test_loss_mix_backward_fills_every_element(sizes):
    """k_mix_bwd: fp32(fp32(d_out scale) w_i) in every element of every tensor, whichever pass writes it"""
    d_out, scale, ws = F32(-0.83), 1.0 / 7.0, [0.37, -1.3, 0.013, 2.0][:len(sizes)]
    grads = hip.loss_mix_bwd([(n,) for n in sizes], ws, scale, _scalar(d_out))
    for n, w, g in zip(sizes, ws, grads):
        assert same_bits(g.cpu().numpy(), np.full(n, head_const_f32(d_out, scale, w), F32)), n


def _special(pred, gt):
    """the clamp's edges in pred, each next to a gt inside, below and above [0, 1]"""
    sp = np.array([0.0, -0.0, 1.0, np.nextafter(F32(1), F32(2)), np.nextafter(F32(0), F32(-1)), np.nan], F32)
    for j, c in enumerate((0.25, -0.5, 1.5)):
        pred.reshape(-1)[6 * j + 256 * j:6 * j + 256 * j + 6] = sp
        gt.reshape(-1)[6 * j + 256 * j:6 * j + 256 * j + 6] = c
    pred.reshape(-1)[-6:] = sp[::-1]


@pytest.mark.parametrize("B", SQERR_RAYS)
def test_sqerr_forward_against_float64_and_backward_bits(B):
    rng = np.random.default_rng([23, B])
    pred, gt = sqerr_inputs(B, rng)
    _special(pred, gt)
    pd, gd = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    val, bound = sqerr_ref(pred, gt)
    got = float(hip.sqerr_fwd(pd, gd))
    prints(f"sqerr_fwd B {B}: device / bound {abs(got - val) / bound:.4f}")
    assert abs(got - val) <= bound
    d = hip.sqerr_bwd(pd, gd, _scalar(0.37)).cpu().numpy()
    want = sqerr_bwd_f32(pred, gt, F32(0.37))
    assert same_bits(d, want), np.flatnonzero(d.view(np.uint32) != want.view(np.uint32))[:10]
    assert not d.reshape(-1)[3:6].any() and d.reshape(-1)[2] != 0 and (d[(pred < 0) | (pred > 1)] == 0).all()
    hot, zero = torch.zeros(B, 3, device=DEV), torch.zeros(B, 3, device=DEV)
    for k in one_hot_positions(3 * B, PER_PASS):
        hot.view(-1)[k] = 0.5
        assert float(hip.sqerr_fwd(hot, zero)) == 0.25 and float(hip.sqerr_fwd(zero, hot)) == 0.25, k
        hot.view(-1)[k] = 0.0


def test_loss_head_on_one_stream():
    """B = 33 001 -> 1 -> 0 -> 33 001 -> 70 000 -> 200 001 on one cached workspace (4096 bytes hold up to 87 040 rays, so it is the
    last size that has to make it grow): every loss within the bound of float64, B = 0 exactly 0, equal inputs give equal bits,
    d_pred / g_a / g_b the bits of their restatements"""
    rng = np.random.default_rng(24)
    d_out, scale, wp, wa, wb = F32(0.75), 1.0 / 7.0, 1.0, 0.013, 0.21
    data = {B: sqerr_inputs(B, rng) for B in set(HEAD_RAYS) | {200001}}
    for pred, gt in data.values():
        if pred.size > 1000:
            _special(pred, gt)
    first, worst = {}, 0.0
    for B in HEAD_RAYS + (200001,):
        pred, gt = data[B]
        loss, d_pred, g_a, g_b = hip.loss_head(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), _scalar(d_out), scale,
                                               wp, wa, wb)
        val, bound = head_ref(pred, gt)
        got = loss.cpu().numpy()
        if B == 0:
            assert float(got) == 0.0 and d_pred.numel() == 0 and g_a.numel() == 0
            continue
        worst = max(worst, abs(float(got) - val) / bound)
        assert abs(float(got) - val) <= bound, (B, float(got), val, bound)
        assert same_bits(d_pred.cpu().numpy(), sqerr_bwd_f32(pred, gt, head_const_f32(d_out, scale, wp))), B
        assert g_a.shape == (B,) and g_b.shape == (B,)
        assert same_bits(g_a.cpu().numpy(), np.full(B, head_const_f32(d_out, scale, wa), F32))
        assert same_bits(g_b.cpu().numpy(), np.full(B, head_const_f32(d_out, scale, wb), F32))
        if B in first:
            assert same_bits(got, first[B])
        first[B] = got
    prints(f"loss_head: device / bound {worst:.4f}")


def test_loss_head_writes_exactly_its_rays():
    """the C entry point on buffers of the test: B entries of g_a / g_b, 3 B of d_pred, the guard regions behind them untouched"""
    rng = np.random.default_rng(25)
    B = 33001
    pred, gt = sqerr_inputs(B, rng)
    d_out, scale, wp, wa, wb = F32(-1.25), 0.3, 0.9, 0.013, 0.21
    ins, outs = Arena(), Arena()
    ins.add(pred), ins.add(gt), ins.add(np.array([d_out], F32))
    for n in (1, 3 * B, B, B):
        outs.add(np.full(n, np.nan, F32))
    ins.upload(), outs.upload()
    ws = hip.loss_head_workspace(torch.device(DEV, torch.cuda.current_device()), B)
    hip._check(hip._lib.nmf_loss_head(ins.ptr(0), ins.ptr(1), B, ins.ptr(2), C.c_float(scale), C.c_float(wp), C.c_float(wa),
                                      C.c_float(wb), outs.ptr(0), outs.ptr(1), outs.ptr(2), outs.ptr(3), ws.data_ptr(), ws.numel(),
                                      hip._stream()), "nmf_loss_head")
    torch.cuda.synchronize()
    loss, d_pred, g_a, g_b = outs.download()
    ins.download()
    val, bound = head_ref(pred, gt)
    assert abs(float(loss[0]) - val) <= bound
    sc = F32(scale)
    assert same_bits(d_pred.reshape(B, 3), sqerr_bwd_f32(pred, gt, head_const_f32(d_out, sc, F32(wp))))
    assert same_bits(g_a, np.full(B, head_const_f32(d_out, sc, F32(wa)), F32))
    assert same_bits(g_b, np.full(B, head_const_f32(d_out, sc, F32(wb)), F32))
