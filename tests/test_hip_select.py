"""Edges of the selection kernels: the radix select / argsort of the re-trace order (csrc/retrace.hip) against
torch.sort(stable=True), and the bounce counts (csrc/select.hip) per element against O.select_bounces.  All comparisons are
exact: these kernels produce indices and counts."""
import numpy as np
import pytest
import torch

from oracle import nmf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 2048                                             # elements per workgroup of the select kernels


def _hip():
    from nmf_amd import hip
    return hip


# ---- topk_select / argsort_f32 -------------------------------------------------------------------------------------------
def _bits(u):
    return torch.from_numpy(np.asarray(u, dtype=np.uint32).view(np.float32).copy())


def _keys(kind, n, gen):
    if kind == "all_equal":
        return torch.full((n,), 0.375)
    if kind == "two_values":
        return torch.where(torch.rand(n, generator=gen) < 0.5, torch.tensor(0.25), torch.tensor(0.75))
    if kind == "last_digit":                             # 1 + i 2^-23, shuffled, every other value twice: passes 0 and 1 see one bin
        i = (torch.randperm(n, generator=gen) // 2).numpy().astype(np.uint32)
        return _bits(np.uint32(0x3F800000) + i)
    if kind == "top_11_bits":                            # sortable codes agree in their top 11 bits only
        low = torch.randint(0, 1 << 21, (n,), generator=gen).numpy().astype(np.uint32)
        low[::5] = low[1 % n]                            # and a tie group
        return _bits(np.uint32(0x3F800000) | low)
    if kind == "realistic":                              # score / sum * num + U with half the scores exactly 0 (models/microfacet.py:501)
        score = torch.rand(n, generator=gen) ** 8
        score[torch.rand(n, generator=gen) < 0.5] = 0.0
        u = torch.rand(n, generator=gen)
        u[::3] = 0.5                                     # ties among the zero scores
        return score / score.sum().clamp_min(1e-20) * (n // 4 + 1) + u
    if kind == "special":
        k = torch.randn(n, generator=gen)
        for j, v in enumerate([float("inf"), float("-inf"), float("nan"), float("inf"), float("-inf"), float("nan")]):
            if n > 2:
                k[(j * 397 + 1) % n] = v                 # (torch's NaN is the positive quiet one, 0x7FC00000)
        return k
    raise KeyError(kind)


def _ks(keys):
    n = keys.shape[0]
    ks = {1, max(n // 2, 1), n - 1, n}
    ks |= {k for k in (4096, 4097) if k <= n}
    if n > CHUNK:                                        # cuts inside a tie group that straddles the first chunk edge
        v = keys[CHUNK - 1] if not bool(torch.isnan(keys[CHUNK - 1])) else keys[0]
        k_edge = int((keys > v).sum()) + int((keys[CHUNK:] == v).sum())
        ks |= {k_edge - 1, k_edge, k_edge + 1}
    return sorted(k for k in ks if 1 <= k <= n)


def _check_select(hip, keys):
    n = keys.shape[0]
    kd = keys.to(DEV)
    order = torch.sort(keys, stable=True).indices
    assert torch.equal(hip.argsort_f32(kd).cpu().long(), order), "argsort_f32"
    for k in _ks(keys):
        top, rest = hip.topk_select(kd, k)
        assert top.shape == (k,) and rest.shape == (n - k,)
        assert torch.equal(top.cpu().long(), order[n - k:]), f"top, n = {n}, k = {k}"
        assert torch.equal(rest.cpu().long(), torch.sort(order[:n - k]).values), f"rest, n = {n}, k = {k}"


@pytest.mark.parametrize("n", [2, 2047, 2048, 2049, 4096, 4097, 3 * 2048 + 5])
@pytest.mark.parametrize("kind", ["all_equal", "two_values", "last_digit", "top_11_bits", "realistic", "special"])
def test_topk_select_and_argsort_on_degenerate_keys(kind, n):
    """top = argsort(keys)[n-k:] in the stable order, rest = the other indices in index order: keys that fill one histogram bin
    in the first passes (the ballot fast path counts whole waves), ties across the cut and across the 2048-element chunks,
    infinities and (positive) NaN, for n at the chunk edges and k at 1, n/2, n-1, n and both sides of the 4096 LDS-sort limit"""
    hip = _hip()
    keys = _keys(kind, n, torch.Generator().manual_seed(n))
    if kind == "two_values" and n >= 2 * CHUNK:           # the tie group of the cut has members on both sides of the chunk edge
        assert bool((keys[:CHUNK] == keys[CHUNK - 1]).sum() > 1) and bool((keys[CHUNK:] == keys[CHUNK - 1]).any())
    _check_select(hip, keys)


@pytest.mark.parametrize("n", [9, 2049, 3 * 2048 + 5])
@pytest.mark.parametrize("first", ["+0", "-0"])
def test_signed_zeros_are_equal_keys_in_every_path(first, n):
    """-0.0 == +0.0: the stable ascending order keeps zeros of either sign in index order (torch.sort(stable=True), and the
    library radix sort behind argsort_f32 / k == n / k > 4096).  The radix select for k < n must agree, with +0.0 before -0.0
    in index order as well as the reverse, zeros on both sides of a chunk edge and the cut inside the zeros."""
    hip = _hip()
    gen = torch.Generator().manual_seed(n)
    keys = torch.rand(n, generator=gen) * 2 - 0.5           # zeros at rank ~ n / 4: for the largest n a cut inside them has k > 4096
    a, b = (0.0, -0.0) if first == "+0" else (-0.0, 0.0)
    zeros = sorted(i for i in {1, 4, n // 2, n - 2, CHUNK - 1, CHUNK, CHUNK + 7} if i < n)
    for j, i in enumerate(zeros):
        keys[i] = a if j % 2 == 0 else b
    order = torch.sort(keys, stable=True).indices
    pos = sorted(int(p) for p in torch.nonzero(keys[order] == 0).reshape(-1))
    assert [int(order[p]) for p in pos] == zeros                     # the reference keeps the zeros in index order
    kd = keys.to(DEV)
    assert torch.equal(hip.argsort_f32(kd).cpu().long(), order), "argsort_f32"
    ks = {n, n - 1, 1} | {n - p for p in pos} | {n - pos[-1] - 1} | ({4097} if n > 4097 else set())
    if n > 4097:
        assert n - pos[0] > 4096                                      # a cut inside the zeros that takes the library sort
    for k in sorted(k for k in ks if 1 <= k <= n):
        top, rest = hip.topk_select(kd, k)
        assert torch.equal(top.cpu().long(), order[n - k:]), f"top, k = {k}"
        assert torch.equal(rest.cpu().long(), torch.sort(order[:n - k]).values), f"rest, k = {k}"


# ---- select_bounces ---------------------------------------------------------------------------------------------------------
def _check_counts(counts, bounce, ray_mask):
    """counts <-> (bounce_mask, ray_mask[bounce_mask]) of the oracle: rows of ray_mask are prefixes of length count"""
    c = counts.cpu().long()
    assert torch.equal(c > 0, bounce)
    assert torch.equal(c[c > 0], ray_mask.sum(1))
    assert torch.equal(torch.arange(ray_mask.shape[1])[None] < c[c > 0][:, None], ray_mask)


def _weights(kind, L, gen):
    if kind == "large":                                  # counts reach the clamp at 400 in both modes
        w = torch.rand(L, generator=gen) * 6
        w[torch.rand(L, generator=gen) < 0.3] *= 1e-3
        return w
    if kind == "small":                                  # pt < 0 for U < 0.5 in mode 0
        return torch.rand(L, generator=gen) * 4e-3
    return torch.zeros(L)


@pytest.mark.parametrize("M", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("kind", ["large", "small", "zero"])
def test_select_bounces_per_element_vs_oracle(kind, M):
    """k_select_bounces against O.select_bounces (pt_selectors.py:5-60) in both modes and both branches of the second one, for M
    at the workgroup edges: the clamp at 400, negative pt, all-zero weights under the clip(min=1e-3) normaliser, and the sum
    handed over as a host scalar or as a device scalar (same bits)."""
    hip = _hip()
    gen = torch.Generator().manual_seed(1000 * M + len(kind))
    L = M + M // 3 + 2
    am = torch.zeros(L, dtype=torch.bool)
    am[torch.randperm(L, generator=gen)[:M]] = True
    w = _weights(kind, L, gen)
    wk = w[am].to(DEV).contiguous()
    # mode 0: pt = w * rays_per_ray + U - 0.5
    U0 = torch.rand(M, generator=gen)
    bounce, ray_mask = O.select_bounces(w, am, 0, 128, O.Noise([("rand", U0)]))
    c0 = hip.select_bounces(wk, U0.to(DEV), 0, 128.0)
    _check_counts(c0, bounce, ray_mask)
    pt0 = w[am] * 128 + U0 - 0.5
    if kind == "large" and M > 1:
        assert int(c0.max()) == 400 and float(pt0.max()) > 401
    if kind != "large" and M > 1:
        assert float(pt0.min()) < 0 and int(c0.min()) == 0
    # mode 1: w' = w + 1e-3 U ; pt = w' / clip(sum w', 1e-3) * N + 1 (N = num_rays - kept > 0) or * num_rays + 0.5
    U1 = torch.rand(L, generator=gen)
    if kind == "zero":
        U1 = U1 * 1e-4                                   # sum(w') < 1e-3 for every M here: the clip is the normaliser
    wp = w + 1e-3 * U1
    S = float(wp.sum().clip(min=1e-3))
    assert (wp.sum() < 1e-3) == (kind == "zero")
    clamped = False
    for num_rays in (M + 700 * M, M + 37, M, max(M // 2, 1)):
        N = num_rays - M
        mul, add = (float(N), 1.0) if N > 0 else (float(num_rays), 0.5)
        bounce, ray_mask = O.select_bounces(w, am, num_rays, None, O.Noise([("rand", U1)]))
        uk = U1[am].to(DEV).contiguous()
        c_host = hip.select_bounces(wk, uk, 1, mul, add, S)
        c_dev = hip.select_bounces(wk, uk, 1, mul, add, torch.tensor(S, dtype=torch.float32, device=DEV))
        assert torch.equal(c_host, c_dev), "S and S_dev forms differ"
        _check_counts(c_host, bounce, ray_mask)
        clamped |= int(c_host.max()) == 400
    if kind == "large" and M > 1:
        assert clamped
