"""GPU checks of the causal filter, the pairwise posteriors xi and autograd through logZ
(vqhmm_filter_f32 / vqhmm_fwdbwd_xi_f32, hmm_pair.hip) against the fp64 restatement in
tests/hmm_pair_ref.py, fed the same fp32 tables.

Bounds (include/vqhmm.h): xi abs 2e-5 (its two factors' 1e-5 contracts, each factor <= 1), filt abs
1e-5 (the gamma contract), loglik / logZ rel 1e-5 against max(1, |ref|), sum_i xi_t(i,j) = the
GPU's own gamma_t(j) within 1e-6 (by construction), exact zeros at t = 0, t >= L and L = 0.

End-to-end autograd (test_autograd_through_model), measured on MI355X: worst got / tol ratio 0.17
(K = 3 dims) and 0.12 (K = 8 dims); the test prints every tensor's ratio.
"""
import numpy as np
import pytest
import torch

import hmm_pair_ref as PR
from oracle import ref_model as RM

pytestmark = pytest.mark.gpu


def log_softmax(a, axis=-1):
    m = a.max(axis=axis, keepdims=True)
    return a - m - np.log(np.exp(a - m).sum(axis=axis, keepdims=True))


def random_hmm(seed, B, T, K, scale=1.5):
    rng = np.random.default_rng(seed)
    log_pi = log_softmax(rng.standard_normal(K)).astype(np.float32)
    log_A = log_softmax(rng.standard_normal((B, T, K, K)) * scale).astype(np.float32)
    em = log_softmax(rng.standard_normal((B, T, K)) * 2.0).astype(np.float32)
    return log_pi, log_A, em


def ragged(seed, B, T):
    """Lengths with T, 0, 1 and 2 first (as far as B and T allow), then random ones."""
    rng = np.random.default_rng(seed)
    L = np.concatenate([[T, 0, 1, 2], rng.integers(0, T + 1, max(B - 4, 0))])[:B]
    return np.minimum(L, T).astype(np.int64)


def gpu(*arrs, offset=False):
    """Device copies; offset: every tensor starts one float past a fresh allocation (4-byte
    aligned only, the kernels' scalar load paths)."""
    out = []
    for a in arrs:
        a = np.ascontiguousarray(a)
        if offset and a.dtype == np.float32:
            buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
            t = buf[1:].view(a.shape)
            t.copy_(torch.from_numpy(a))
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            out.append(t)
        else:
            out.append(torch.from_numpy(a).cuda())
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def rel_ok(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf])
    ok = ~(nan | inf)
    err = np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
    assert err.max(initial=0) <= tol, err.max()


def check_case(log_pi, log_A, em, L, offset=False, skip=()):
    """All the per-case checks; `skip`: sequences about whose posteriors nothing is asserted."""
    import vqhmm
    B, T, K = em.shape
    ref = PR.pair_ref(log_pi, log_A, em, L)
    d_pi, d_A, d_em = gpu(log_pi, log_A, em, offset=offset)
    d_L = torch.from_numpy(L)
    filt, loglik = vqhmm.forward_filter(d_pi, d_A, d_em, d_L)
    gamma, xi, logZ = vqhmm.pairwise_posteriors(d_pi, d_A, d_em, d_L)
    g0, z0 = vqhmm.forward_backward(d_pi, d_A, d_em, d_L)
    assert torch.equal(bits(gamma), bits(g0)) and torch.equal(bits(logZ), bits(z0))
    assert xi.shape == (B, T, K, K) and filt.shape == (B, T, K)
    filt, loglik, gamma, xi, logZ = (t.cpu().numpy() for t in (filt, loglik, gamma, xi, logZ))
    keep = np.array([b not in skip for b in range(B)])
    rel_ok(loglik, ref["loglik"])
    rel_ok(logZ, ref["logZ"])
    assert not np.isnan(xi[keep]).any() and not np.isnan(filt[keep]).any()
    e_xi = np.abs(xi[keep] - ref["xi"][keep]).max(initial=0)
    e_f = np.abs(filt[keep] - ref["filt"][keep]).max(initial=0)
    e_col = np.abs(xi[keep].astype(np.float64).sum(2) - gamma[keep])[:, 1:].max(initial=0)
    print(f"K={K} B={B} T={T}: xi {e_xi:.2e} filt {e_f:.2e} colsum {e_col:.2e}")
    assert e_xi <= 2e-5 and e_f <= 1e-5 and e_col <= 1e-6
    for b in range(B):
        if b in skip:
            continue
        n = int(L[b])
        assert not xi[b, 0].any() and not xi[b, n:].any() and not filt[b, n:].any()
        if n:
            assert np.abs(filt[b, :n].astype(np.float64).sum(1) - 1).max() <= 1e-5
            assert np.abs(filt[b, n - 1] - gamma[b, n - 1]).max() <= 2e-5
    return ref, xi, filt


LANE_K = (1, 2, 3, 4, 5, 8)
LANE_BT = ((3, 1), (5, 2), (7, 17), (70, 64), (9, 65), (6, 130), (4, 300))
WIDE_K = (9, 16, 17, 32)
WIDE_BT = ((3, 1), (5, 45), (4, 130))
GRID = [(K, B, T) for K in LANE_K for B, T in LANE_BT] + [(K, B, T) for K in WIDE_K for B, T in WIDE_BT]


@pytest.mark.parametrize("K,B,T", GRID)
def test_filter_and_xi(K, B, T):
    log_pi, log_A, em = random_hmm(100 * K + B + T, B, T, K)
    check_case(log_pi, log_A, em, ragged(K + T, B, T))


def test_long_sequence_drift():
    K, B, T = 8, 4, 4096
    log_pi, log_A, em = random_hmm(4096, B, T, K)
    check_case(log_pi, log_A, em, np.array([T, T - 1, 1000, 3000], np.int64))


@pytest.mark.parametrize("K,B,T", [(4, 6, 70), (8, 5, 130), (3, 7, 40), (16, 4, 45)])
def test_unaligned_inputs(K, B, T):
    log_pi, log_A, em = random_hmm(K + B, B, T, K)
    check_case(log_pi, log_A, em, ragged(K, B, T), offset=True)


@pytest.mark.parametrize("K,B,T", [(4, 5, 40), (8, 4, 70), (16, 4, 33)])
def test_structural_zeros(K, B, T):
    """Upper-triangular transitions (-inf below the diagonal), finite emissions."""
    rng = np.random.default_rng(K)
    raw = rng.standard_normal((B, T, K, K)) * 1.5
    raw[..., np.tril_indices(K, -1)[0], np.tril_indices(K, -1)[1]] = -np.inf
    log_pi, _, em = random_hmm(K, B, T, K)
    log_A = log_softmax(raw).astype(np.float32)
    L = ragged(K, B, T)
    _, xi, filt = check_case(log_pi, log_A, em, L)
    assert not np.isnan(xi).any() and not np.isnan(filt).any()
    assert not xi[..., np.tril_indices(K, -1)[0], np.tril_indices(K, -1)[1]].any()


@pytest.mark.parametrize("K,B,T", [(3, 6, 60), (8, 4, 70), (16, 4, 45)])
def test_small_step_mass(K, B, T):
    """Unnormalised tables whose step mass is far below the fast step's range at some steps (the
    max-shifted log-sum-exp step takes over there), far above it at one: same contract.  The shifts
    are the smallest round ones that leave the fast range [2^-30, 2^30] = exp(+-20.8) for certain (a
    step's mass is at most exp(shift) for row-stochastic tables): fp32 tables resolve 2e-6 at a
    magnitude of 24-30, and that input resolution, not the kernels, sets the error floor there."""
    log_pi, log_A, em = random_hmm(3 * K, B, T, K)
    log_A[:, 5::7] -= 24.0
    log_A[0, 11] += 30.0
    check_case(log_pi, log_A, em, ragged(K + 1, B, T))


@pytest.mark.parametrize("K,B,T", [(3, 6, 60), (8, 4, 70), (16, 4, 45)])
def test_impossible_sequence(K, B, T):
    """All emissions -inf at one step of one sequence: its loglik and logZ are -inf, the others stay
    within contract (K = 3: they share its wave); nothing is asserted about its posteriors."""
    log_pi, log_A, em = random_hmm(7 * K, B, T, K)
    em[1, T // 3] = -np.inf
    L = np.full(B, T, np.int64)
    L[2] = T // 2
    ref, _, _ = check_case(log_pi, log_A, em, L, skip=(1,))
    assert ref["loglik"][1] == -np.inf


# ------------------------------------------------------------------------ autograd
def logZ_torch(log_pi, log_A, em, L):
    """Log-space forward recursion in torch (any dtype, differentiable); L >= 1 everywhere."""
    al = log_pi[None] + em[:, 0]
    for t in range(1, em.shape[1]):
        nxt = torch.logsumexp(al[:, :, None] + log_A[:, t], 1) + em[:, t]
        al = torch.where((t < L)[:, None], nxt, al)
    return torch.logsumexp(al, 1)


@pytest.mark.parametrize("K,B,T", [(3, 6, 40), (8, 5, 130), (16, 3, 45)])
def test_autograd_leaf_gradients(K, B, T):
    import vqhmm
    log_pi, log_A, em = random_hmm(K * B, B, T, K)
    L = np.minimum(np.array([T, 1, 2, T // 2, 0, T - 1][:B]), T).astype(np.int64)
    if B == 3:
        L = np.array([T, 0, 7], np.int64)
    g = np.random.default_rng(K).standard_normal(B).astype(np.float32)
    d_pi, d_A, d_em, d_g = gpu(log_pi, log_A, em, g)
    d_L = torch.from_numpy(L)
    g_plain, z_plain = vqhmm.forward_backward(d_pi, d_A, d_em, d_L)
    assert z_plain.grad_fn is None and not z_plain.requires_grad
    for t in (d_pi, d_A, d_em):
        t.requires_grad_(True)
    gamma, logZ = vqhmm.forward_backward(d_pi, d_A, d_em, d_L)
    assert gamma.requires_grad is False and logZ.grad_fn is not None
    assert torch.equal(bits(gamma), bits(g_plain)) and torch.equal(bits(logZ), bits(z_plain))
    live = torch.from_numpy(L > 0).cuda()
    (d_g * torch.where(live, logZ, torch.zeros_like(logZ))).sum().backward()

    r_pi, r_A, r_em = (torch.from_numpy(a).double().requires_grad_(True) for a in (log_pi, log_A, em))
    Lt = torch.from_numpy(np.maximum(L, 1))
    w = torch.from_numpy(g).double() * torch.from_numpy(L > 0)
    (w * logZ_torch(r_pi, r_A, r_em, Lt)).sum().backward()
    gmax, gsum = float(np.abs(g).max()), float(np.abs(g).sum())
    e_A = (d_A.grad.cpu().double() - r_A.grad).abs().max().item()
    e_em = (d_em.grad.cpu().double() - r_em.grad).abs().max().item()
    e_pi = (d_pi.grad.cpu().double() - r_pi.grad).abs().max().item()
    print(f"K={K}: dlog_A {e_A / gmax:.2e} dem {e_em / gmax:.2e} dlog_pi {e_pi / gsum:.2e}")
    assert e_A <= 2e-5 * gmax and e_em <= 1e-5 * gmax and e_pi <= 1e-5 * gsum
    for b in np.nonzero(L == 0)[0]:
        assert not d_A.grad[b].any() and not d_em.grad[b].any()


def test_length_zero_rows_get_zero_gradient():
    """logZ of a length-0 sequence is NaN; a loss that sums it still sends no NaN into the inputs."""
    import vqhmm
    log_pi, log_A, em = random_hmm(1, 3, 9, 4)
    d_pi, d_A, d_em = (t.requires_grad_(True) for t in gpu(log_pi, log_A, em))
    _, logZ = vqhmm.forward_backward(d_pi, d_A, d_em, torch.tensor([9, 0, 4]))
    logZ.sum().backward()
    assert torch.isnan(logZ[1]) and not d_A.grad[1].any() and not d_em.grad[1].any()
    assert torch.isfinite(d_A.grad).all() and torch.isfinite(d_em.grad).all() and torch.isfinite(d_pi.grad).all()
    assert d_em.grad[2, 4:].abs().max() == 0 and d_A.grad[0, 1:].abs().max() > 0


def test_gradients_need_k_le_32():
    import vqhmm
    log_pi, log_A, em = random_hmm(2, 2, 5, 33)
    d_pi, d_A, d_em = gpu(log_pi, log_A, em)
    gamma, logZ = vqhmm.forward_backward(d_pi, d_A, d_em)  # without gradients: as before
    assert torch.isfinite(logZ).all()
    d_em.requires_grad_(True)
    with pytest.raises(RuntimeError, match="32"):
        vqhmm.forward_backward(d_pi, d_A, d_em)
    with pytest.raises(RuntimeError, match="32"):
        vqhmm.pairwise_posteriors(d_pi, d_A, d_em.detach())
    with pytest.raises(RuntimeError):
        vqhmm.forward_filter(d_pi, d_A, d_em.detach())


def _ref_model_grads(state, x, u, L, K, dtype):
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in state.items()}
    xr = x.to(dtype)
    ur = u.to(dtype).requires_grad_(True)
    em = torch.log_softmax(RM.encoder_logits(p, xr), 1).transpose(1, 2)
    log_pi, log_A = RM.prior_tables(p, ur, K, 4)
    (-logZ_torch(log_pi, log_A, em, L).mean()).backward()
    out = {k: v.grad for k, v in p.items() if v.grad is not None}
    out["du"] = ur.grad
    return out


@pytest.mark.parametrize("dims,B,T", [((5, 64, 3, 32), 6, 40), ((16, 64, 8, 32), 4, 64)])
def test_autograd_through_model(dims, B, T):
    """-(logZ).mean() through forward_backward, log_softmax(encode(x)) and prior(u), every encoder /
    prior gradient and du against the same graph in fp64 on the CPU.  Tolerance per tensor,
    normwise: max(1e-5, 4 e32), e32 = the reference graph's own fp32-vs-fp64 difference (the
    log-softmax backward forms xi - gamma A, a difference of nearly equal terms, so xi's 1e-5 does
    not carry through as 1e-5; the factor 4 covers another summation order)."""
    import vqhmm
    D, H, K, H2 = dims
    torch.manual_seed(K)
    m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=4, trans_hidden=128).cuda()
    gen = torch.Generator().manual_seed(B * T)
    x = torch.randn(B, D, T, generator=gen)
    u = torch.randn(B, 4, T, generator=gen)
    L = torch.randint(2, T + 1, (B,), generator=gen)
    L[0] = T
    ug = u.cuda().requires_grad_(True)
    em = torch.log_softmax(m.encode(x.cuda()), dim=1).transpose(1, 2).contiguous()
    log_pi, log_A = m.prior(ug)
    gamma, logZ = vqhmm.forward_backward(log_pi, log_A, em, L)
    (-logZ.mean()).backward()

    r64 = _ref_model_grads(m.state_dict(), x, u, L, K, torch.float64)
    r32 = _ref_model_grads(m.state_dict(), x, u, L, K, torch.float32)
    got = {n: prm.grad for n, prm in m.named_parameters()}
    got["du"] = ug.grad
    worst = 0.0
    for name, ref in r64.items():
        assert name.startswith(("prior.", "encoder.")) or name == "du", name
        n64 = max(ref.norm().item(), 1e-30)
        e32 = (r32[name].double() - ref).norm().item() / n64
        tol = max(1e-5, 4 * e32)
        err = (got[name].detach().cpu().double() - ref).norm().item() / n64
        print(f"{name}: err {err:.2e} e32 {e32:.2e} ratio {err / tol:.2f}")
        worst = max(worst, err / tol)
        assert err <= tol, f"{name}: {err:.2e} > {tol:.2e}"
    assert sum(k.startswith("prior.") for k in r64) == 5 and sum(k.startswith("encoder.") for k in r64) == 6
    for n, prm in m.named_parameters():
        if n.startswith("decoder."):
            assert prm.grad is None, n
    print(f"worst ratio {worst:.2f}")


# ----------------------------------------------------------------- filtered_regimes
def test_filtered_regimes():
    import vqhmm
    torch.manual_seed(5)
    B, D, K, T = 5, 5, 3, 48
    m = vqhmm.VAE_HMM(D, 64, K, 32, u_dim=4, trans_hidden=128).cuda()
    x = torch.randn(B, D, T).cuda()
    u = torch.randn(B, 4, T).cuda()
    L = torch.tensor([T, 30, 1, 17, 0])
    regimes, probs = vqhmm.filtered_regimes(m, x, u, L)
    assert regimes.dtype == torch.int64 and regimes.shape == (B, T) and probs.shape == (B, K, T)
    with torch.no_grad():
        em = torch.log_softmax(m.encode(x), dim=1).transpose(1, 2).contiguous()
        log_pi, log_A = m.prior(u)
    filt, _ = vqhmm.forward_filter(log_pi, log_A, em, L)
    assert torch.equal(bits(probs), bits(filt.transpose(1, 2)))
    inside = torch.arange(T)[None, :] < L[:, None]
    r = regimes.cpu()
    assert torch.equal(r[inside], probs.argmax(1).cpu()[inside]) and (r[~inside] == -1).all()
    # causal: x changed after t leaves the probabilities up to t - 2 alone (the encoder's convolutions
    # reach two steps ahead), while the smoothed gamma there moves
    t = 30
    x2 = x.clone()
    x2[:, :, t + 1:] += torch.randn(B, D, T - t - 1, device="cuda")
    _, probs2 = vqhmm.filtered_regimes(m, x2, u, L)
    assert (probs2[..., :t - 1] - probs[..., :t - 1]).abs().max() <= 1e-6
    assert (probs2[0, :, t + 2:] - probs[0, :, t + 2:]).abs().max() > 1e-4
