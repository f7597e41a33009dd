"""GPU checks of the regime-path samplers (vqhmm_ffbs_sample_f32 / vqhmm_markov_sample_f32,
hmm_sample.hip) against the numpy restatement of the draw rule in tests/sample_ref.py.

Exact tests: both sides get the same fp32 bits (filt from the fp64 reference rounded to fp32, the
tables, and uniforms whose every draw clears the margin bound (K + 8) * 2^-22 derived in
sample_ref.py), so the paths must be equal element for element.  The statistics tests compare
empirical state frequencies with the exact marginals within 5 binomial standard deviations + 2 / N
(the committed seed keeps the reference itself inside 4: tests/test_sample_ref.py).
"""
import numpy as np
import pytest
import torch

import sample_ref as SR
from conftest import load_golden

pytestmark = pytest.mark.gpu


def dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def raw_sample(kind, head, log_A, lengths, u):
    """The raw C-ABI call on device tensors -> paths (B, N, T) int32 (prefilled with a sentinel, so
    an element the kernel leaves unwritten shows)."""
    from vqhmm import _ext
    B, N, T = u.shape
    K = log_A.shape[2]
    paths = torch.full((B, N, T), -7, dtype=torch.int32, device="cuda")
    fn = getattr(_ext.load(), "vqhmm_ffbs_sample_f32" if kind == "ffbs" else "vqhmm_markov_sample_f32")
    P = _ext.ptr
    _ext.check(fn(P(head), P(log_A), P(lengths), P(u), B, T, K, N, P(paths), _ext.stream_ptr()), kind)
    return paths


@pytest.mark.parametrize("kind", ["ffbs", "markov"])
@pytest.mark.parametrize("K,T,N", SR.EXACT_CASES)
def test_paths_equal_reference_exactly(kind, K, T, N):
    c = SR.exact_case(K, T, N)
    ref, u_used, _ = c[kind]
    head = c["filt"] if kind == "ffbs" else c["log_pi"]
    d_head, d_A, d_L, d_u = dev(head, c["log_A"], c["lengths"], u_used)
    got = raw_sample(kind, d_head, d_A, d_L, d_u)
    again = raw_sample(kind, d_head, d_A, d_L, d_u)
    g = got.cpu().numpy()
    assert np.array_equal(g, ref), (np.argwhere(g != ref)[:5], g[g != ref][:5], ref[g != ref][:5])
    assert torch.equal(got, again)
    L = c["lengths"]
    for b in range(SR.B_CASE):
        assert (g[b, :, L[b]:] == -1).all() and (g[b, :, :L[b]] >= 0).all()
    assert (g[1] == -1).all()  # the length-0 row


@pytest.mark.parametrize("kind", ["ffbs", "markov"])
def test_bulk_agreement_on_raw_uniforms(kind):
    """50,000 samples of one K = 3, T = 4 sequence, the uniforms as drawn: every row whose reference
    margins all clear the bound matches exactly; at most 0.1 % of the rows are excluded."""
    c = SR.bulk_case()
    ref, keep = c[kind]
    head = c["filt"] if kind == "ffbs" else c["log_pi"]
    g = raw_sample(kind, *dev(head, c["log_A"], c["lengths"], c["u"])).cpu().numpy()
    print(f"{kind}: excluded rows {(~keep).sum()} of {keep.size}, mismatching rows among all "
          f"{(g != ref).any(axis=2).sum()}")
    assert (~keep).sum() <= 0.001 * keep.size
    assert np.array_equal(g[keep], ref[keep])
    assert g.min() >= 0 and g.max() < c["K"]


def structural_tables(seed, B, T, K):
    """A left-to-right-or-stay chain with extra random zeros: -inf in log_A and log_pi, every row
    keeping at least its diagonal."""
    rng = np.random.default_rng(seed)
    log_pi, log_A, em = SR.random_tables(rng, B, T, K)
    mask = rng.random((B, T, K, K)) < 0.4
    mask |= np.tril(np.ones((K, K), bool), -1)[None, None]
    mask &= ~np.eye(K, dtype=bool)[None, None]
    log_A = np.where(mask, -np.inf, log_A).astype(np.float32)
    log_pi = log_pi.copy()
    log_pi[K - 1] = -np.inf
    return log_pi, log_A, em


def path_scores(paths, log_pi, log_A, em=None):
    """joint log score of every sampled path inside its length, in torch (B, N)"""
    B, N, T = paths.shape
    z = paths.long().clamp(min=0)
    valid = paths >= 0
    sc = log_pi[z[:, :, 0]]
    bi = torch.arange(B, device=paths.device)[:, None].expand(B, N)
    if em is not None:
        sc = sc + em[bi, 0, z[:, :, 0]]
    sc = torch.where(valid[:, :, 0], sc, torch.zeros_like(sc))
    for t in range(1, T):
        st = log_A[bi, t, z[:, :, t - 1], z[:, :, t]]
        if em is not None:
            st = st + em[bi, t, z[:, :, t]]
        sc = sc + torch.where(valid[:, :, t], st, torch.zeros_like(st))
    return sc


@pytest.mark.parametrize("K", [4, 12])
def test_structural_zeros_are_never_drawn(K):
    import vqhmm
    B, T, N = 4, 50, 96
    log_pi, log_A, em = structural_tables(K, B, T, K)
    L = np.array([T, 31, 1, 0], np.int64)
    d_pi, d_A, d_em, d_L = dev(log_pi, log_A, em, L)
    u = torch.from_numpy(np.random.default_rng(K).random((B, N, T), dtype=np.float32)).cuda()
    _, loglik = vqhmm.forward_filter(d_pi, d_A, d_em, d_L)
    assert torch.isfinite(loglik[:3]).all()
    past = (torch.arange(T, device="cuda")[None, None, :] >= d_L[:, None, None]).expand(B, N, T)
    post = vqhmm.sample_posterior_paths(d_pi, d_A, d_em, d_L, n_samples=N, uniforms=u)
    assert torch.equal(post < 0, past)
    assert torch.isfinite(path_scores(post, d_pi, d_A, d_em)).all()
    sim = vqhmm.simulate_paths(d_pi, d_A, d_L, n_samples=N, uniforms=u)
    assert torch.equal(sim < 0, past)
    assert torch.isfinite(path_scores(sim, d_pi, d_A)).all()
    assert int(sim.max()) < K and int(post.max()) < K


@pytest.mark.parametrize("K,T", [(3, 40), (8, 70), (20, 33)])
def test_impossible_sequence_gives_minus_one(K, T):
    """As test_forward_backward_impossible_sequence builds it: every emission -inf at one step of
    sequence 1.  It has no posterior: all -1; its neighbours sample as they do without it."""
    import vqhmm
    B, N = 3, 5
    rng = np.random.default_rng(K * 5 + T)
    log_pi, log_A, em = SR.random_tables(rng, B, T, K)
    bad = em.copy()
    bad[1, T // 3, :] = -np.inf
    L = np.array([T, T, T - 7], np.int64)
    u = torch.from_numpy(rng.random((B, N, T), dtype=np.float32)).cuda()
    d_pi, d_A, d_em, d_bad, d_L = dev(log_pi, log_A, em, bad, L)
    good = vqhmm.sample_posterior_paths(d_pi, d_A, d_em, d_L, n_samples=N, uniforms=u)
    got = vqhmm.sample_posterior_paths(d_pi, d_A, d_bad, d_L, n_samples=N, uniforms=u)
    assert (got[1] == -1).all() and (good[1] >= 0).all()
    assert torch.equal(got[0], good[0]) and torch.equal(got[2], good[2])


def test_failed_draws_match_reference():
    """-inf rows and columns in the middle of the walk: the kernels fail the same draws as the
    reference and write -1 from there on (simulation: forward; FFBS: toward t = 0)."""
    K, T, N, B = 5, 20, 70, 2
    rng = np.random.default_rng(99)
    log_pi, log_A, em = SR.random_tables(rng, B, T, K)
    filt = SR.pair_ref(log_pi, log_A, em)["filt"].astype(np.float32)
    log_A[0, 9] = -np.inf          # simulation dies at t = 9 for every sample of sequence 0
    log_A[1, 12, :, 2] = -np.inf   # FFBS: the samples with z_12 = 2 die below t = 12
    log_A[1, 5, 3, :] = -np.inf    # simulation: the samples with z_4 = 3 die from t = 5
    L = np.array([T, T - 1], np.int64)
    u = rng.random((B, N, T), dtype=np.float32)
    fix = np.random.default_rng(5)
    fp, fu, _ = SR.ffbs_ref(filt, log_A, L, u, fix=fix)
    mp, mu, _ = SR.markov_ref(log_pi, log_A, L, u, fix=fix)
    assert (fp[0, :, :9] == -1).all() and (mp[0, :, 9:] == -1).all() and (mp[1] == -1).any() and (mp[1, :, -2] >= 0).any()
    gf = raw_sample("ffbs", *dev(filt, log_A, L, fu)).cpu().numpy()
    gm = raw_sample("markov", *dev(log_pi, log_A, L, mu)).cpu().numpy()
    assert np.array_equal(gf, fp) and np.array_equal(gm, mp)


def test_wrapper_equals_raw_kernel_and_options():
    import vqhmm
    B, T, K, N = 4, 37, 6, 9
    rng = np.random.default_rng(12)
    log_pi, log_A, em = SR.random_tables(rng, B, T, K)
    L = np.array([T, 0, 11, 36], np.int64)
    d_pi, d_A, d_em, d_L = dev(log_pi, log_A, em, L)
    u = torch.from_numpy(rng.random((B, N, T), dtype=np.float32)).cuda()
    filt, loglik = vqhmm.forward_filter(d_pi, d_A, d_em, d_L)
    raw = raw_sample("ffbs", filt, d_A, d_L, u)
    raw[1] = -1  # length 0: loglik is NaN, the wrapper masks the row (the kernel wrote -1 anyway)
    got = vqhmm.sample_posterior_paths(d_pi, d_A, d_em, d_L, n_samples=N, uniforms=u)
    assert got.dtype == torch.int32 and got.shape == (B, N, T) and torch.equal(got, raw)
    sim = vqhmm.simulate_paths(d_pi, d_A, d_L, n_samples=N, uniforms=u)
    assert torch.equal(sim, raw_sample("markov", d_pi, d_A, d_L, u))
    # int32 and CPU lengths
    for Lx in (torch.from_numpy(L), torch.from_numpy(L).int().cuda(), L.tolist()):
        assert torch.equal(vqhmm.sample_posterior_paths(d_pi, d_A, d_em, Lx, n_samples=N, uniforms=u), got)
        assert torch.equal(vqhmm.simulate_paths(d_pi, d_A, Lx, n_samples=N, uniforms=u), sim)
    # lengths=None: full length
    full = vqhmm.simulate_paths(d_pi, d_A, n_samples=2, uniforms=u[:, :2].contiguous())
    assert (full >= 0).all()
    # generator: reproducible, and another seed differs
    def gen(seed):
        return torch.Generator(device="cuda").manual_seed(seed)
    for fn, args in ((vqhmm.sample_posterior_paths, (d_pi, d_A, d_em, d_L)), (vqhmm.simulate_paths, (d_pi, d_A, d_L))):
        a = fn(*args, n_samples=N, generator=gen(1))
        assert torch.equal(a, fn(*args, n_samples=N, generator=gen(1)))
        assert not torch.equal(a, fn(*args, n_samples=N, generator=gen(2)))
        # n_samples = 0, and an empty batch
        assert fn(*args, n_samples=0).shape == (B, 0, T)
    assert vqhmm.simulate_paths(d_pi, d_A[:0], n_samples=3).shape == (0, 3, T)
    assert vqhmm.sample_posterior_paths(d_pi, d_A[:, :0], d_em[:, :0], n_samples=3).shape == (B, 3, 0)
    # inputs that require grad are accepted, the result carries none
    r_pi, r_A, r_em = (t.clone().requires_grad_(True) for t in (d_pi, d_A, d_em))
    out = vqhmm.sample_posterior_paths(r_pi, r_A, r_em, d_L, n_samples=N, uniforms=u)
    assert torch.equal(out, got) and not out.requires_grad
    out = vqhmm.simulate_paths(r_pi, r_A, d_L, n_samples=N, uniforms=u)
    assert torch.equal(out, sim) and not out.requires_grad
    # a wrongly shaped uniforms tensor is refused
    with pytest.raises(ValueError):
        vqhmm.simulate_paths(d_pi, d_A, d_L, n_samples=N, uniforms=u[:, :2])


def test_k33_raises():
    import vqhmm
    K = 33
    log_pi = torch.zeros(K, device="cuda")
    log_A = torch.zeros(2, 5, K, K, device="cuda")
    em = torch.zeros(2, 5, K, device="cuda")
    with pytest.raises(RuntimeError, match="K <= 32"):
        vqhmm.sample_posterior_paths(log_pi, log_A, em, n_samples=2)
    with pytest.raises(RuntimeError, match="K <= 32"):
        vqhmm.simulate_paths(log_pi, log_A, n_samples=2)


def test_state_frequencies_match_exact_marginals():
    """B = 3, T = 40, K = 4, N = 8192 through the public API: posterior samples against
    forward_backward's gamma, simulated paths against the fp64 forward marginals pi * prod A, within
    5 sqrt(p (1 - p) / N) + 2 / N at every (b, t < L, k)."""
    import vqhmm
    c = SR.stat_case()
    N = SR.STAT_SHAPE["N"]
    d_pi, d_A, d_em, d_L, d_u = dev(c["log_pi"], c["log_A"], c["em"], c["lengths"], c["u"])
    post = vqhmm.sample_posterior_paths(d_pi, d_A, d_em, d_L, n_samples=N, uniforms=d_u).cpu().numpy()
    gamma, _ = vqhmm.forward_backward(d_pi, d_A, d_em, d_L)
    ex = SR.freq_excess(post, gamma.double().cpu().numpy(), c["lengths"], 5.0)
    print("posterior: worst excess over the 5 sigma bound", ex)
    assert ex <= 0
    sim = vqhmm.simulate_paths(d_pi, d_A, d_L, n_samples=N, uniforms=d_u).cpu().numpy()
    ex = SR.freq_excess(sim, c["prior"], c["lengths"], 5.0)
    print("simulation: worst excess over the 5 sigma bound", ex)
    assert ex <= 0
    for p in (post, sim):
        for b, L in enumerate(c["lengths"]):
            assert (p[b, :, L:] == -1).all() and (p[b, :, :L] >= 0).all()


def test_model_level_functions_compose():
    import vqhmm
    from test_gpu_model import make_model
    g = load_golden("smoke_tiny")
    m = make_model(g)
    x, u = torch.tensor(g["x"]).cuda(), torch.tensor(g["u"]).cuda()
    B, T = x.shape[0], x.shape[2]
    L = torch.tensor(g["lengths"])
    N = 7
    uni = torch.from_numpy(np.random.default_rng(8).random((B, N, T), dtype=np.float32)).cuda()
    with torch.no_grad():
        em = torch.log_softmax(m.encode(x), dim=1).transpose(1, 2).contiguous()
        log_pi, log_A = m.prior(u)
    post = vqhmm.sampled_regimes(m, x, u, L, n_samples=N, uniforms=uni)
    assert torch.equal(post, vqhmm.sample_posterior_paths(log_pi, log_A, em, L, n_samples=N, uniforms=uni))
    sim = vqhmm.simulate_regimes(m, u, L, n_samples=N, uniforms=uni)
    assert torch.equal(sim, vqhmm.simulate_paths(log_pi, log_A, L, n_samples=N, uniforms=uni))
    assert post.shape == sim.shape == (B, N, T) and post.dtype == sim.dtype == torch.int32
    # the -1 padding is viterbi_regimes' convention
    path, _ = vqhmm.viterbi_regimes(m, x, u, L)
    pad = (path < 0)[:, None, :].expand(B, N, T)
    assert torch.equal(post < 0, pad) and torch.equal(sim < 0, pad)
    # generator form
    a = vqhmm.sampled_regimes(m, x, u, L, n_samples=3, generator=torch.Generator(device="cuda").manual_seed(4))
    b = vqhmm.sampled_regimes(m, x, u, L, n_samples=3, generator=torch.Generator(device="cuda").manual_seed(4))
    assert torch.equal(a, b)


def test_single_state_model_samples_zero():
    import vqhmm
    torch.manual_seed(0)
    m = vqhmm.VAE_HMM(16, 32, 1, 16, u_dim=4, trans_hidden=128).cuda()
    B, T, N = 3, 21, 4
    x, u = torch.randn(B, 16, T, device="cuda"), torch.randn(B, 4, T, device="cuda")
    L = torch.tensor([T, 5, 0])
    want = torch.where(torch.arange(T)[None, :] < L[:, None], 0, -1).int()[:, None, :].expand(B, N, T).cuda()
    assert torch.equal(vqhmm.sampled_regimes(m, x, u, L, n_samples=N), want)
    assert torch.equal(vqhmm.simulate_regimes(m, u, L, n_samples=N), want)
