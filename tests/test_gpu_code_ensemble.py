"""GPU checks of the member axis and the sequence weights of the fused E-step (vqhmm_code_estep_batched_f32,
hmm_code.hip) and of what is built on them: vqhmm.CodeHMMEnsemble, CodeHMM.fit(n_init=R), vqhmm.code_log_prob
and the mixture of HMMs.

Two kinds of comparison.  Bit identity (torch.equal on the raw bits) with the single-model entry
vqhmm_code_estep_f32 wherever the weights are absent or all 1.  Against the fp64 reference of
tests/code_ens_ref.py elsewhere, within the per-position contracts of include/vqhmm.h (gamma abs 1e-5, xi abs
2e-5, loglik rel 1e-5 of max(1, |ref|)) scaled by the weights: pi 1e-5 sum_b |w_b|, trans 2e-5 sum_b |w_b|
max(L_b - 1, 0), emit[., v] 1e-5 sum_b |w_b| n_{b,v} over the sequences that count (the weight multiply is fp64
and adds nothing visible at that scale).
"""
import numpy as np
import pytest
import torch

import code_ens_ref as E
import code_hmm_ref as R
import test_gpu_code_hmm as G
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
NINF = -np.inf
KEYS = ("pi_cnt", "trans_cnt", "emit_cnt", "loglik", "gamma")
CNT = KEYS[:3]
PARAMS = ("log_pi", "log_A", "log_B")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def stack(models):
    return tuple(np.stack([m[k] for m in models]) for k in range(3))


def raw_batched(models, codes, lengths, weights=None, loglik=True, gamma=True, offset=False, M=None):
    """vqhmm_code_estep_batched_f32 through ctypes on guarded exact-size buffers and a guarded, poisoned
    workspace of exactly the queried size (gpu_buffers.guarded); the counts start as NaN and loglik / gamma as 7
    (the call must write every element) -> (rc, dict of device tensors)."""
    from vqhmm import _ext
    lib = _ext.load()
    log_pi, log_A, log_B = (G.dev_f32(a, offset) for a in stack(models))
    Mm, S, V = log_B.shape
    M = Mm if M is None else M
    B, T = codes.shape
    d_codes = G.dev_i32(codes, offset) if codes.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    d_w = None if weights is None else G.dev_f32(weights, offset)
    cnt = [guarded(sh, torch.float64, fill=float("nan")) for sh in ((Mm, S), (Mm, S, S), (Mm, S, V))]
    ll = guarded((Mm, B), torch.float32, fill=7.0) if loglik else None
    gm = guarded((Mm, B, T, S), torch.float32, fill=7.0) if gamma else None
    nb = lib.vqhmm_code_estep_batched_workspace_size(B, T, S, V, M)
    ws = guarded(nb, torch.uint8)
    rc = lib.vqhmm_code_estep_batched_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(log_B), _ext.ptr(d_codes),
                                          _ext.ptr(d_len), _ext.ptr(d_w), B, T, S, V, M, cnt[0].ptr, cnt[1].ptr,
                                          cnt[2].ptr, ll.ptr if loglik else None, gm.ptr if gamma else None, ws.ptr,
                                          nb, _ext.stream_ptr())
    check_all(*cnt, ll, gm, ws)
    return rc, dict(pi_cnt=cnt[0].t, trans_cnt=cnt[1].t, emit_cnt=cnt[2].t, loglik=ll.t if loglik else None,
                    gamma=gm.t if gamma else None)


def make_members(seed, M, S, V, B, T, scale=1.5):
    """M random models with different seeds and one shared ragged batch (lengths T, 0, 1, 2, then random)."""
    _, codes, L = G.make_case(seed, S, V, B, T)
    models = [R.random_model(np.random.default_rng(seed + 1000 * (m + 1)), S, V, scale) for m in range(M)]
    return models, codes, L


def check_members_bit_identical(models, codes, L, offset=False):
    rc, got = raw_batched(models, codes, L, offset=offset)
    assert rc == 0, rc
    rc, ones = raw_batched(models, codes, L, weights=np.ones((len(models), codes.shape[0]), np.float32))
    assert rc == 0, rc
    for m, model in enumerate(models):
        base = G.raw_estep(model, codes, L)
        for k in KEYS:
            assert bits_equal(got[k][m], base[k]), (m, k)
            assert bits_equal(ones[k][m], base[k]), ("ones", m, k)


# ------------------------------------------------------ 1. bit identity with the single-model entry
# a sample of M {1,2,3,5} x S {1,2,3,5,8,9,17,32} x V {1,5,512} x B {1,5,9} x T {1,65,130}: every value of each
# axis occurs, every SP instantiation (1, 2, 4, 8, 16, 32) at its edge and one inside
BIT_CASES = ((1, 1, 1, 1, 1), (2, 2, 5, 5, 65), (3, 3, 512, 9, 130), (5, 5, 5, 9, 65), (2, 8, 512, 5, 130),
             (3, 9, 5, 9, 65), (2, 17, 1, 5, 130), (2, 32, 512, 9, 65), (5, 3, 5, 1, 1), (1, 8, 5, 9, 130))


@pytest.mark.parametrize("M,S,V,B,T", BIT_CASES)
def test_members_bit_identical_to_single_model(M, S, V, B, T):
    check_members_bit_identical(*make_members(7 * S + V + B + T, M, S, V, B, T))


def test_members_bit_identical_l2_tier():
    check_members_bit_identical(*make_members(31, 2, 32, 4096, 6, 70))


def test_members_bit_identical_largest_lds_tier():
    """test_estep_largest_lds_tier's shape (S = 8, V = 512, B = 9, T = 40), two members."""
    check_members_bit_identical(*make_members(850, 2, 8, 512, 9, 40))


def test_members_bit_identical_unaligned():
    """Every pointer offset by 4 bytes; at S = 3 the member slices are 4-byte aligned only (36-byte stride)."""
    check_members_bit_identical(*make_members(41, 3, 3, 5, 9, 70), offset=True)


# --------------------------------------------------- 3. weighted counts against the fp64 reference
def check_weighted(got, ref, codes, L, V, tag=""):
    """got: dict of (M, ...) device tensors; ref: estep_ens_ref's list."""
    for m, r in enumerate(ref):
        b_pi, b_tr, b_em = E.weighted_bounds(r["abs_w"], codes, L, V)
        pi, tr, em = (got[k][m].cpu().numpy() for k in CNT)
        assert not (np.isnan(pi).any() or np.isnan(tr).any() or np.isnan(em).any())
        e_pi, e_tr, e_em = np.abs(pi - r["pi_cnt"]).max(), np.abs(tr - r["trans_cnt"]).max(), np.abs(em - r["emit_cnt"])
        print(f"{tag} m={m} pi {e_pi:.2e}/{b_pi:.1e} trans {e_tr:.2e}/{b_tr:.1e} emit {e_em.max():.2e}/{b_em.max():.1e}")
        assert e_pi <= b_pi and e_tr <= b_tr
        assert (e_em <= b_em[None, :]).all(), (e_em - b_em[None, :]).max()


@pytest.mark.parametrize("V", (5, 64))
@pytest.mark.parametrize("S", (3, 8, 17))
def test_weighted_counts_vs_reference(S, V):
    M, B, T = 3, 9, 70
    models, codes, L = make_members(50 + S + V, M, S, V, B, T)
    w = np.random.default_rng(S * V).uniform(-2, 2, (M, B)).astype(np.float32)
    w[:, 0] = (-1.5, 0.0, 2.0)  # the full-length sequence: negative, exactly 0, the range's end
    w[0, 4], w[2, 5] = 0.0, -2.0
    rc, got = raw_batched(models, codes, L, weights=w)
    assert rc == 0
    ref = E.estep_ens_ref(models, codes, L, w)
    check_weighted(got, ref, codes, L, V, f"S={S} V={V}")
    # loglik and gamma do not depend on the weights
    _, plain = raw_batched(models, codes, L)
    assert bits_equal(got["loglik"], plain["loglik"]) and bits_equal(got["gamma"], plain["gamma"])
    for m in range(M):
        G.rel_ok(got["loglik"][m].cpu().numpy(), ref[m]["loglik"])


# ------------------------------------------------------------------- 4. per-member outcomes
def test_per_member_outcomes():
    """Member 1's structural zeros make sequences 1 and 4 impossible under it alone; sequence 2 carries a code
    outside [0, V): NaN under every member."""
    rng = np.random.default_rng(700)
    S, V, T, B = 3, 6, 20, 6
    models = [list(R.random_model(np.random.default_rng(710 + m), S, V)) for m in range(3)]
    models[1][2][1:, 0] = NINF   # only state 0 emits code 0 ...
    models[1][1][0, 0] = NINF    # ... and it never follows itself
    models = [tuple(m) for m in models]
    codes = rng.integers(1, V, size=(B, T)).astype(np.int32)
    L = np.array([T, 15, 17, T - 1, 9, 12], np.int64)
    codes[0, :] = np.where(np.arange(T) % 2 == 0, 0, codes[0, :])  # possible: code 0 never twice running
    codes[1, 7] = codes[1, 8] = 0   # impossible under member 1
    codes[4, 2] = codes[4, 3] = 0
    codes[2, 9] = V                 # out of range, inside the length
    w = np.random.default_rng(701).uniform(-2, 2, (3, B)).astype(np.float32)
    for weights in (None, w):
        rc, got = raw_batched(models, codes, L, weights=weights)
        assert rc == 0
        ll = got["loglik"].cpu().numpy()
        assert np.isnan(ll[:, 2]).all()
        assert (ll[1, [1, 4]] == NINF).all() and np.isfinite(ll[1, [0, 3, 5]]).all()
        assert np.isfinite(ll[[0, 2]][:, [0, 1, 3, 4, 5]]).all()
        assert not got["gamma"][1][[1, 2, 4]].any() and not got["gamma"][:, 2].any()
        ref = E.estep_ens_ref(models, codes, L, weights)
        assert ref[1]["abs_w"][[1, 2, 4]].tolist() == [0, 0, 0] and (ref[0]["abs_w"][[1, 4]] > 0).all()
        check_weighted(got, ref, codes, L, V, "outcomes")
        # member 1's counts are those of its three possible sequences alone: nothing of 1, 2, 4 entered (the
        # fp64 sums of at most 3 x 20 terms of size <= 2 run in another order: a few 1e-15)
        keep = [0, 3, 5]
        rc, alone = raw_batched(models[1:2], codes[keep], L[keep], weights=None if weights is None else weights[1:2, keep])
        for k in CNT:
            assert (got[k][1] - alone[k][0]).abs().max().item() <= 1e-12, k


# -------------------------------------------------------------------------- 5. padded members
def test_padded_members():
    import vqhmm
    sizes, V, B, T = [2, 3, 5, 8], 6, 9, 40
    ens = vqhmm.CodeHMMEnsemble(num_states=sizes, num_codes=V, generator=torch.Generator().manual_seed(3)).cuda()
    assert ens.num_models == 4 and ens.num_states == 8 and ens.log_B.shape == (4, 8, V)
    _, codes, L = G.make_case(900, 8, V, B, T)
    d_codes, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(L).cuda()
    st = ens.e_step(d_codes, d_len)
    members = [tuple(getattr(ens.member(m), k).cpu().numpy() for k in PARAMS) for m in range(4)]
    for m, s in enumerate(sizes):
        assert members[m][2].shape == (s, V)
        ref = R.estep_ref(*members[m], codes, L)
        G.rel_ok(st["loglik"][m].cpu().numpy(), ref["loglik"])
        pi, tr, em = (st[k][m].cpu().numpy() for k in CNT)
        G.check_counts(dict(pi_cnt=pi[:s], trans_cnt=tr[:s, :s], emit_cnt=em[:s]), ref, codes, L, V, f"S_m={s}")
        assert not pi[s:].any() and not tr[s:].any() and not tr[:, s:].any() and not em[s:].any()
    ens.fit(d_codes, d_len, n_iter=3, prior_count=1e-3)
    for m, s in enumerate(sizes):
        assert (ens.log_pi[m, s:] == NINF).all() and (ens.log_A[m, s:] == NINF).all()
        assert (ens.log_A[m, :, s:] == NINF).all()
        assert torch.isfinite(ens.log_pi[m, :s]).all() and torch.isfinite(ens.log_A[m, :s, :s]).all()
    # free parameters: (S-1) + S(S-1) + S(V-1) of the unpadded model
    want = [(s - 1) + s * (s - 1) + s * (V - 1) for s in sizes]
    assert ens.num_free_parameters().tolist() == want
    ll = ens.log_prob(d_codes, d_len).double().nansum(1)
    bic = ens.bic(d_codes, d_len)
    assert bic.shape == (4,) and bic.dtype == torch.float64
    npos = float(np.clip(L, 0, T).sum())
    assert torch.allclose(bic.cpu(), -2 * ll.cpu() + torch.tensor(want, dtype=torch.float64) * np.log(npos), rtol=1e-12)


# ----------------------------------------------------------------------- 6. one EM iteration
def test_one_em_iteration_matches_separate_models():
    import vqhmm
    M, S, V, B, T = 3, 5, 12, 9, 70
    ens = vqhmm.CodeHMMEnsemble(num_models=M, num_states=S, num_codes=V, generator=torch.Generator().manual_seed(8)).cuda()
    g = torch.Generator().manual_seed(8)
    hmms = [vqhmm.CodeHMM(S, V, generator=g).cuda() for _ in range(M)]  # the same draws, in member order
    _, codes, L = G.make_case(910, S, V, B, T)
    d_codes, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(L).cuda()
    for m, h in enumerate(hmms):
        for k in PARAMS:
            assert torch.equal(getattr(ens, k)[m], getattr(h, k)), (m, k)
    st = ens.e_step(d_codes, d_len, return_gamma=True)
    assert st["flat"].shape == (M, S + S * S + S * V) and st["loglik"].shape == (M, B)
    assert st["pi_cnt"].data_ptr() == st["flat"].data_ptr()  # views of the buffer an all-reduce would sum
    ens.m_step(st, prior_count=1e-3)
    for m, h in enumerate(hmms):
        one = h.e_step(d_codes, d_len, return_gamma=True)
        for k in KEYS:
            assert bits_equal(st[k][m], one[k]), (m, k)
        h.m_step(one, prior_count=1e-3)
        for k in PARAMS:
            # fp64 arithmetic rounded to fp32: one ulp apart at most if torch orders a batched row sum differently
            assert torch.allclose(getattr(ens, k)[m], getattr(h, k), atol=1e-6, rtol=1e-6), (m, k)


# --------------------------------------------------------------------------- 7. fit(n_init=R)
def test_fit_restarts():
    import vqhmm
    Rn, n_iter, B, T, S, V = 4, 5, 32, 40, 3, 8
    truth = R.random_model(np.random.default_rng(2000), S, V, scale=2.0)
    codes = E.sample_codes(truth, B, T, 2001)
    d_codes = torch.from_numpy(codes).cuda()

    def run(seed):
        hmm = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(5)).cuda()
        hist = hmm.fit(d_codes, n_iter=n_iter, n_init=Rn, generator=torch.Generator().manual_seed(seed))
        assert len(hist) == n_iter and all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 for v in hist)
        return hmm, hist

    hmm, hist = run(77)
    hmm2, hist2 = run(77)
    for k in PARAMS:
        assert torch.equal(getattr(hmm, k), getattr(hmm2, k)), k
    assert [v.item() for v in hist] == [v.item() for v in hist2]
    # the four members fitted alone from the same starts
    base = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(5)).cuda()
    starts = base._restart_ensemble(Rn, torch.Generator().manual_seed(77))
    for k in PARAMS:
        assert torch.equal(getattr(starts, k)[0], getattr(base, k)), k
    assert not torch.equal(starts.log_A[1], starts.log_A[2])
    chosen = hmm.log_prob(d_codes).cpu().numpy().astype(np.float64)
    totals, slacks = [], []
    for m in range(Rn):
        alone = starts.member(m)
        alone.fit(d_codes, n_iter=n_iter)
        ll = alone.log_prob(d_codes).cpu().numpy().astype(np.float64)
        slack = (1e-5 * np.maximum(1.0, np.abs(ll))).sum()  # the header's loglik contract, summed
        totals.append(ll.sum())
        slacks.append(slack)
        print(f"member {m}: final total {ll.sum():.4f}, chosen {chosen.sum():.4f}, slack {slack:.1e}")
        assert chosen.sum() >= ll.sum() - slack, (m, chosen.sum(), ll.sum())
    assert chosen.sum() <= max(totals) + max(slacks)  # it is one of the members


def test_fit_n_init_1_is_the_plain_fit_and_tol_is_refused():
    import vqhmm
    S, V, B, T = 3, 8, 16, 64
    truth = R.random_model(np.random.default_rng(2100), S, V, scale=2.0)
    codes = torch.from_numpy(E.sample_codes(truth, B, T, 2101)).cuda()
    a = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(5)).cuda()
    b = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(5)).cuda()
    ha = a.fit(codes, n_iter=4, prior_count=0.1, n_init=1, generator=torch.Generator().manual_seed(1))
    hb = []
    for _ in range(4):  # the parent's loop: e_step, total, m_step
        st = b.e_step(codes)
        hb.append(st["loglik"].double().nansum())
        b.m_step(st, 0.1)
    assert [v.item() for v in ha] == [v.item() for v in hb]
    for k in PARAMS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    with pytest.raises(ValueError):
        a.fit(codes, n_iter=2, tol=1e-4, n_init=2)


# ------------------------------------------------------------------------------- 8. gradient
def torch_loglik(log_pi, log_A, log_B, codes, lengths):
    """fp64 logsumexp forward recursion, differentiable by torch autograd (CPU); length 0 -> a detached NaN."""
    out = []
    for b in range(codes.shape[0]):
        n = int(lengths[b])
        if n == 0:
            out.append(torch.tensor(float("nan"), dtype=torch.float64))
            continue
        c = codes[b, :n].tolist()
        al = log_pi + log_B[:, c[0]]
        for t in range(1, n):
            al = torch.logsumexp(al[:, None] + log_A, 0) + log_B[:, c[t]]
        out.append(torch.logsumexp(al, 0))
    return torch.stack(out)


def grad_case(S, V=6, B=5, T=9):
    rng = np.random.default_rng(3000 + S)
    model = R.random_model(rng, S, V)
    codes = rng.integers(0, V, (B, T)).astype(np.int32)
    L = np.array([T, 0, 4, 1, 7], np.int64)
    g = rng.uniform(-2, 2, B).astype(np.float32)
    return model, codes, L, g


def gpu_grads(model, codes, L, g):
    import vqhmm
    p = [torch.from_numpy(a).cuda().requires_grad_() for a in model]
    ll = vqhmm.code_log_prob(*p, torch.from_numpy(codes).cuda(), torch.from_numpy(L).cuda())
    assert ll.shape == (codes.shape[0],) and ll.dtype == torch.float32 and ll.requires_grad
    ll.backward(torch.from_numpy(g).cuda())
    return ll.detach().cpu().numpy(), [t.grad.cpu().numpy().astype(np.float64) for t in p]


def check_grads(got, want, g, ll_ref, codes, L, V):
    abs_w = np.where(np.isfinite(ll_ref), np.abs(g.astype(np.float64)), 0.0)
    b_pi, b_tr, b_em = E.weighted_bounds(abs_w, codes, L, V)
    # (the cast of a count to fp32 is half an ulp, 6e-8 of an entry that is itself <= sum_b |g_b| n_b: 0.6 % of
    # the bound at most)
    e = [np.abs(a - b) for a, b in zip(got, want)]
    print(f"grad pi {e[0].max():.2e}/{b_pi:.1e} A {e[1].max():.2e}/{b_tr:.1e} B {e[2].max():.2e}/{b_em.max():.1e}")
    assert e[0].max() <= b_pi and e[1].max() <= b_tr
    assert (e[2] <= b_em[None, :]).all()


@pytest.mark.parametrize("S", (2, 5))
def test_code_log_prob_gradient(S):
    model, codes, L, g = grad_case(S)
    V = model[2].shape[1]
    p = [torch.from_numpy(a).double().requires_grad_() for a in model]
    ll_t = torch_loglik(*p, codes, L)
    ok = torch.isfinite(ll_t)
    (ll_t[ok] * torch.from_numpy(g).double()[ok]).sum().backward()
    want = [t.grad.numpy() for t in p]
    ll, got = gpu_grads(model, codes, L, g)
    G.rel_ok(ll, ll_t.detach().numpy())
    check_grads(got, want, g, ll_t.detach().numpy(), codes, L, V)


def test_code_log_prob_impossible_sequence_gives_zero_gradient():
    model, codes, L, g = grad_case(5)
    model = tuple(a.copy() for a in model)
    model[2][:, 5] = NINF           # no state emits code 5
    codes = np.where(codes == 5, 4, codes).astype(np.int32)
    ll0, base = gpu_grads(model, codes, L, g)
    assert np.isfinite(ll0[L > 0]).all()
    codes2 = codes.copy()
    codes2[0, 3] = 5                # sequence 0 becomes impossible
    ll, got = gpu_grads(model, codes2, L, g)
    assert ll[0] == NINF and all(np.isfinite(a).all() for a in got)
    keep = [1, 2, 3, 4]
    _, others = gpu_grads(model, codes[keep], L[keep], g[keep])
    for a, b, c in zip(got, others, base):
        # 0 from the impossible one, the others' unchanged: the same fp64 terms summed in another order (the
        # batch is one shorter) and rounded to fp32, one ulp apart at the most
        assert (np.abs(a - b) <= 2.0 ** -23 * np.maximum(1.0, np.abs(b))).all()
        assert not np.array_equal(a, c)
    # validation, and CodeHMM.log_prob stays outside autograd
    import vqhmm
    with pytest.raises(RuntimeError, match="HIP"):
        vqhmm.code_log_prob(*(torch.from_numpy(a) for a in model), torch.from_numpy(codes))
    with pytest.raises(ValueError):
        vqhmm.code_log_prob(*(torch.from_numpy(a).cuda().double() for a in model), torch.from_numpy(codes).cuda())
    hmm = vqhmm.CodeHMM(5, 6).cuda()
    assert not hmm.log_prob(torch.from_numpy(codes).cuda()).requires_grad


def test_adam_on_logits_raises_the_likelihood():
    import vqhmm
    S, V, B, T = 3, 8, 16, 30
    truth = R.random_model(np.random.default_rng(3100), S, V, scale=2.0)
    codes = torch.from_numpy(E.sample_codes(truth, B, T, 3101)).cuda()
    gen = torch.Generator().manual_seed(4)
    logits = [torch.randn(sh, generator=gen).cuda().requires_grad_() for sh in ((S,), (S, S), (S, V))]
    opt = torch.optim.Adam(logits, lr=0.05)
    means = []
    for _ in range(10):
        opt.zero_grad()
        ll = vqhmm.code_log_prob(*(torch.log_softmax(t, -1) for t in logits), codes)
        (-ll.mean()).backward()
        opt.step()
        means.append(ll.mean().item())
    final = vqhmm.code_log_prob(*(torch.log_softmax(t, -1) for t in logits), codes).mean().item()
    assert final > means[0], (means, final)


# -------------------------------------------------------------------------------- 9. mixture
def mixture_ensemble():
    import vqhmm
    codes, L, labels, start, log_mix = E.planted_mixture_case()
    hmms = []
    for mod in start:
        h = vqhmm.CodeHMM(E.MIX_S, E.MIX_V)
        h.load_state_dict(dict(zip(PARAMS, (torch.from_numpy(a) for a in mod))))
        hmms.append(h.cuda())
    ens = vqhmm.CodeHMMEnsemble.from_models(hmms)
    assert ens.log_mix.is_cuda and torch.allclose(ens.log_mix.cpu().double(), torch.from_numpy(log_mix))
    return ens, codes, L, labels, start, log_mix


def test_mixture_one_iteration_vs_reference():
    ens, codes, L, labels, start, log_mix = mixture_ensemble()
    d_codes, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(L).cuda()
    hist = ens.fit_mixture(d_codes, d_len, n_iter=1)
    assert hist.shape == (1,) and hist.dtype == torch.float64 and hist.is_cuda
    ref_hist, models, mix, _ = E.mixture_ref(start, log_mix, codes, L, n_iter=1)
    ll_ref = np.stack([e["loglik"] for e in E.estep_ens_ref(models, codes, L)])
    r_ref, _, _ = E.responsibilities_ref(mix, ll_ref)
    delta = (1e-5 * np.maximum(1.0, np.abs(ll_ref))).max()
    r = ens.responsibilities(d_codes, d_len)
    assert r.shape == (E.MIX_M, E.MIX_B)
    err = np.abs(r.cpu().numpy() - r_ref).max()
    print(f"responsibilities after one iteration: max err {err:.2e}, bound 2 delta = {2 * delta:.2e}")
    assert err <= 2 * delta
    assert torch.allclose(r.sum(0).cpu(), torch.ones(E.MIX_B, dtype=torch.float64), atol=1e-12)
    slack = (1e-5 * np.maximum(1.0, np.abs(ll_ref))).sum()
    assert abs(hist[0].item() - ref_hist[0]) <= slack


def test_mixture_monotone_and_recovers_the_planted_clusters():
    ens, codes, L, labels, start, log_mix = mixture_ensemble()
    d_codes, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(L).cuda()
    hist = ens.fit_mixture(d_codes, d_len, n_iter=6).cpu().numpy()
    # item 7's slack on the mixture's own per-sequence log-likelihood: sum_b 1e-5 max(1, |ll_b|)
    ll = ens.log_prob(d_codes, d_len).cpu().numpy().astype(np.float64)
    _, ok, _ = E.responsibilities_ref(ens.log_mix.cpu().numpy(), ll)
    with np.errstate(invalid="ignore"):
        z = ens.log_mix.cpu().numpy().astype(np.float64)[:, None] + np.where(np.isnan(ll), NINF, ll)
    mix_ll = np.logaddexp(z[0], z[1])[ok]
    slack = (1e-5 * np.maximum(1.0, np.abs(mix_ll))).sum()
    print("mixture history", hist, "slack", slack)
    assert (np.diff(hist) >= -slack).all(), hist
    assign = ens.responsibilities(d_codes, d_len).argmax(0).cpu().numpy()
    hits = max((assign == labels).sum(), (assign == 1 - labels).sum())
    assert hits >= 22, hits
    assert abs(torch.exp(ens.log_mix.double()).sum().item() - 1) <= 1e-6


# ------------------------------------------------------------- 10. determinism and graph capture
def test_batched_deterministic_and_graph_capturable():
    """B = 300: more than one workgroup per member takes part in the reduction."""
    from vqhmm import _ext
    lib = _ext.load()
    M, S, V, B, T = 3, 4, 9, 300, 70
    models, codes, L = make_members(1400, M, S, V, B, T)
    w = np.random.default_rng(1401).uniform(-2, 2, (M, B)).astype(np.float32)
    _, a = raw_batched(models, codes, L, weights=w)
    _, b = raw_batched(models, codes, L, weights=w)
    for k in KEYS:
        assert bits_equal(a[k], b[k]), k
    d = [G.dev_f32(x) for x in stack(models)]
    d_codes, d_len, d_w = G.dev_i32(codes), torch.from_numpy(L).cuda(), G.dev_f32(w)
    cnt = [torch.zeros(sh, dtype=torch.float64, device="cuda") for sh in ((M, S), (M, S, S), (M, S, V))]
    ll = torch.zeros(M, B, device="cuda")
    nb = lib.vqhmm_code_estep_batched_workspace_size(B, T, S, V, M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.vqhmm_code_estep_batched_f32(_ext.ptr(d[0]), _ext.ptr(d[1]), _ext.ptr(d[2]), _ext.ptr(d_codes),
                                              _ext.ptr(d_len), _ext.ptr(d_w), B, T, S, V, M, _ext.ptr(cnt[0]),
                                              _ext.ptr(cnt[1]), _ext.ptr(cnt[2]), _ext.ptr(ll), None, _ext.ptr(ws), nb,
                                              _ext.stream_ptr())
    assert rc == 0
    for _ in range(2):
        for t in cnt:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for got, k in zip(cnt, CNT):
            assert bits_equal(got, a[k]), k
        assert bits_equal(ll, a["loglik"])


# ------------------------------------------------------------------ 11. empty and edge cases
def test_empty_batches_and_member_limits():
    from vqhmm import _ext
    lib = _ext.load()
    models = [R.random_model(np.random.default_rng(1200 + m), 3, 5) for m in range(2)]
    for B, T in ((0, 4), (2, 0), (0, 0)):
        rc, got = raw_batched(models, np.zeros((B, T), np.int32), np.zeros(B, np.int64))
        assert rc == 0
        for k in CNT:
            assert not got[k].cpu().numpy().any(), (B, T, k)
        assert np.isnan(got["loglik"].cpu().numpy()).all()
    codes = np.zeros((2, 4), np.int32)
    for M in (0, 65536):
        assert lib.vqhmm_code_estep_batched_workspace_size(2, 4, 3, 5, M) == 0
        rc, _ = raw_batched(models, codes, np.full(2, 4, np.int64), M=M)
        assert rc == _ext.EUNSUPPORTED, (M, rc)
    assert lib.vqhmm_code_estep_batched_workspace_size(2, 4, 3, 5, 65535) > 0
    # one member's workspace is the single-model entry's, up to the 256-byte rounding between members
    one = lib.vqhmm_code_estep_workspace_size(9, 70, 8, 64)
    assert one <= lib.vqhmm_code_estep_batched_workspace_size(9, 70, 8, 64, 1) < one + 256


def test_member_groups_give_the_same_bits():
    import vqhmm
    M, S, V, B, T = 5, 4, 9, 9, 70
    ens = vqhmm.CodeHMMEnsemble(num_models=M, num_states=S, num_codes=V, generator=torch.Generator().manual_seed(1)).cuda()
    _, codes, L = G.make_case(1500, S, V, B, T)
    d_codes, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(L).cuda()
    w = torch.from_numpy(np.random.default_rng(1501).uniform(-2, 2, (M, B)).astype(np.float32)).cuda()
    whole = ens.e_step(d_codes, d_len, weights=w, return_gamma=True)
    per = vqhmm._ext.load().vqhmm_code_estep_batched_workspace_size(B, T, S, V, 1)
    for cap in (1, 2 * per, 3 * per + 1):  # groups of 1, 2 and 3 members
        ens.max_workspace_bytes = cap
        part = ens.e_step(d_codes, d_len, weights=w, return_gamma=True)
        for k in KEYS + ("flat",):
            assert bits_equal(whole[k], part[k]), (cap, k)
    # a (B,) weight is broadcast to every member
    ens.max_workspace_bytes = 1 << 30
    bc = ens.e_step(d_codes, d_len, weights=w[0])
    assert bits_equal(bc["flat"], ens.e_step(d_codes, d_len, weights=w[0].expand(M, B))["flat"])


def test_ensemble_selection_and_validation():
    import vqhmm
    S, V, B, T = 3, 8, 12, 30
    truth = R.random_model(np.random.default_rng(1600), S, V, scale=2.0)
    codes = torch.from_numpy(E.sample_codes(truth, B, T, 1601)).cuda()
    ens = vqhmm.CodeHMMEnsemble(num_models=4, num_states=S, num_codes=V, generator=torch.Generator().manual_seed(2)).cuda()
    hist = ens.fit(codes, n_iter=3, prior_count=1e-3)
    assert hist.shape == (3, 4) and hist.dtype == torch.float64 and hist.is_cuda
    ll = ens.log_prob(codes)
    assert ll.shape == (4, B)
    m = int(ll.double().nansum(1).argmax())
    best = ens.best(codes)
    assert isinstance(best, vqhmm.CodeHMM)
    for k in PARAMS:
        assert torch.equal(getattr(best, k), getattr(ens, k)[m]) and torch.equal(getattr(ens.member(m), k), getattr(best, k))
    assert bits_equal(best.log_prob(codes), ll[m])
    with pytest.raises(RuntimeError, match="HIP"):
        ens.e_step(codes.cpu())
    with pytest.raises(ValueError):
        ens.e_step(codes.float())
    with pytest.raises(ValueError):
        ens.e_step(codes, weights=torch.ones(3, B, device="cuda"))
    with pytest.raises(ValueError):
        ens.e_step(codes, weights=torch.ones(4, B, device="cuda", dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP"):
        ens.e_step(codes, weights=torch.ones(4, B))
    with pytest.raises(ValueError):
        vqhmm.CodeHMMEnsemble.from_models([vqhmm.CodeHMM(2, 4), vqhmm.CodeHMM(2, 5)])
