"""GPU checks of the batched Gaussian E-step (vqhmm_gauss_estep_batched_f32 / vqhmm_gauss_full_estep_batched_f32,
hmm_gauss.hip / hmm_gauss_full.hip) and of what is built on it: vqhmm.GaussianHMMEnsemble and
GaussianHMM.fit(n_init=R), against the single-model entries (bit for bit) and the fp64 restatement in
tests/gauss_ens_ref.py.

Bounds.  Weighted counts: the header's per-position contracts (gamma 1e-5, xi 2e-5, moments 2e-5 of the absolute
sums) scaled by sum_b |w_b| (gauss_ens_ref.weighted_bounds), against the reference fed the emission tensors the
emission entries wrote.  loglik: rel 1e-5 of max(1, |ref|).  Everything said to be "the same bits" is compared as
bytes.
"""
import numpy as np
import pytest
import torch

import gauss_ens_ref as E
import gauss_full_ref as F
import gauss_hmm_ref as G
import test_gpu_gauss_full as HF
import test_gpu_gauss_hmm as H
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
NINF = -np.inf
COUNTS = H.COUNTS
OUT = COUNTS + ("loglik", "gamma")
EUNSUPPORTED = -4
FORMS = pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])
dev_f32, rel_ok = H.dev_f32, H.rel_ok

# (S, D, B, T)
SHAPES_BOTH = ((1, 1, 3, 7), (2, 3, 5, 65), (3, 5, 7, 130), (8, 5, 9, 64), (17, 16, 4, 70))
SHAPE_CASES = ([(False, s) for s in SHAPES_BOTH + ((32, 64, 3, 66),)] +
               [(True, s) for s in SHAPES_BOTH + ((32, 16, 3, 66), (8, 32, 3, 66))])


def _id(case):
    return ("full" if case[0] else "diag") + "-S%d-D%d-B%d-T%d" % case[1]


def make_stack(full, seed, M, S, D, B, T, lengths=None):
    """M random models of S states and one data set scattered around member 0's means -> (models, x, L)."""
    mk = HF.make_case if full else H.make_case
    first, x, L = mk(seed, B, T, S, D, lengths=lengths)
    models = [first] + [mk(seed + 1000 * m, 1, 1, S, D)[0] for m in range(1, M)]
    return models, x, L


def single(full, model, x, L, **kw):
    return (HF.raw_estep if full else H.raw_estep)(model, x, L, **kw)


def raw_emissions(full, models, x, L):
    return [(HF.raw_emission if full else H.raw_emission)(m, x, L).cpu().numpy() for m in models]


def _entries(full):
    from vqhmm import _ext
    lib = _ext.load()
    if full:
        return lib.vqhmm_gauss_full_estep_batched_workspace_size, lib.vqhmm_gauss_full_estep_batched_f32
    return lib.vqhmm_gauss_estep_batched_workspace_size, lib.vqhmm_gauss_estep_batched_f32


def raw_batched(full, models, x, lengths, shift=None, weights=None, loglik=True, gamma=True, offset=False,
                expect=0):
    """The batched entry through ctypes on guarded exact-size outputs and a guarded, poisoned workspace of
    exactly the queried size (gpu_buffers.guarded; offset: every float input 4 bytes into its allocation); the
    counts start as NaN (the call must write every element) -> dict of device tensors."""
    from vqhmm import _ext
    size, entry = _entries(full)
    M = len(models)
    log_pi, log_A, mean, last = (dev_f32(np.stack([m[k] for m in models]), offset) for k in range(4))
    S, D = mean.shape[1:]
    B, T = x.shape[:2]
    d_x = dev_f32(x, offset)
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    d_sh, d_w = dev_f32(shift, offset), dev_f32(weights, offset)
    shapes = ((M, S), (M, S, S), (M, S), (M, S, D), (M, S, D, D) if full else (M, S, D))
    cnt = {k: guarded(sh, torch.float64, fill=float("nan")) for k, sh in zip(COUNTS, shapes)}
    ll = guarded((M, B), torch.float32, fill=7.0) if loglik else None
    gm = guarded((M, B, T, S), torch.float32, fill=7.0) if gamma else None
    nb = size(B, T, S, D, M)
    ws = guarded(nb, torch.uint8)
    rc = entry(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(last), _ext.ptr(d_x), _ext.ptr(d_len),
               _ext.ptr(d_sh), _ext.ptr(d_w), B, T, S, D, M, *(cnt[k].ptr for k in COUNTS), ll.ptr if loglik else None,
               gm.ptr if gamma else None, ws.ptr, nb, _ext.stream_ptr())
    assert rc == expect, rc
    check_all(*cnt.values(), ll, gm, ws)
    return dict({k: g.t for k, g in cnt.items()}, loglik=ll.t if loglik else None, gamma=gm.t if gamma else None)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def member_equals(batched, m, one, keys=OUT, tag=""):
    for k in keys:
        assert same_bits(batched[k][m], one[k]), (tag, m, k)


# ------------------------------------------------------- 1. bit identity to the single-model entry
@pytest.mark.parametrize("case", SHAPE_CASES, ids=_id)
def test_members_are_the_single_model_call_bit_for_bit(case):
    full, (S, D, B, T) = case
    models, x, L = make_stack(full, 100 + S + D, 3, S, D, B, T)
    shift = x.reshape(-1, D).mean(0).astype(np.float32)
    ones = [single(full, m, x, L, shift=shift) for m in models]
    for M in (1, 2, 3):
        got = raw_batched(full, models[:M], x, L, shift=shift)
        for m in range(M):
            member_equals(got, m, ones[m], tag=f"M={M}")


@FORMS
def test_misaligned_exact_size_member_buffers(full):
    """S*D = 15: the member slices are only 4-byte aligned; every buffer additionally 4 bytes into its exact-size
    allocation."""
    S, D, B, T = 3, 5, 7, 130
    models, x, L = make_stack(full, 150, 3, S, D, B, T)
    w = np.random.default_rng(151).uniform(0.5, 2.0, (3, B)).astype(np.float32)
    got = raw_batched(full, models, x, L, weights=w, offset=True)
    for m in range(3):
        member_equals(got, m, single(full, models[m], x, L, weights=w[m], offset=True))


@FORMS
def test_more_sequences_than_waves(full):
    """The plan runs at most 2048 waves: with B = 2100 some waves own two sequences."""
    S, D, B, T = 2, 2, 2100, 3
    L = np.random.default_rng(160).integers(0, T + 1, B)
    models, x, L = make_stack(full, 161, 2, S, D, B, T, lengths=L)
    got = raw_batched(full, models, x, L)
    for m in range(2):
        member_equals(got, m, single(full, models[m], x, L))


@FORMS
def test_nullable_outputs(full):
    models, x, L = make_stack(full, 170, 2, 4, 3, 6, 70)
    ref = raw_batched(full, models, x, L)
    no = raw_batched(full, models, x, L, loglik=False, gamma=False)
    for k in COUNTS:
        assert same_bits(ref[k], no[k]), k
    no_g = raw_batched(full, models, x, L, gamma=False)
    for k in COUNTS + ("loglik",):
        assert same_bits(ref[k], no_g[k]), k


# ------------------------------------------------------------------------------------ 2. weights
@FORMS
def test_all_ones_weights_are_the_bits_of_null(full):
    models, x, L = make_stack(full, 200, 3, 5, 4, 8, 70)
    a = raw_batched(full, models, x, L)
    b = raw_batched(full, models, x, L, weights=np.ones((3, 8), np.float32))
    for k in OUT:
        assert same_bits(a[k], b[k]), k


@FORMS
def test_weighted_counts_against_fp64(full):
    M, S, D, B, T = 3, 4, 3, 8, 70
    models, x, L = make_stack(full, 210, M, S, D, B, T)
    rng = np.random.default_rng(211)
    w = (rng.standard_normal((M, B)) * 2).astype(np.float32)
    w[0, 0], w[1, 3], w[2, 5], w[0, 4] = 0.0, -1.5, 0.0, -0.25
    shift = x.reshape(-1, D).mean(0).astype(np.float32)
    got = raw_batched(full, models, x, L, shift=shift, weights=w)
    plain = raw_batched(full, models, x, L, shift=shift)
    for k in ("loglik", "gamma"):          # neither depends on the weights
        assert same_bits(got[k], plain[k]), k
    ref = E.estep_ens_ref(models, x, L, shift=shift, weights=w, full=full, ems=raw_emissions(full, models, x, L))
    for m in range(M):
        rel_ok(got["loglik"][m].cpu().numpy(), ref[m]["loglik"])
        bounds = E.weighted_bounds(ref[m]["abs_w"], x, L, shift, full)
        for k in COUNTS:
            g = got[k][m].cpu().numpy()
            err = np.abs(g - ref[m][k])
            print(f"member {m} {k}: {err.max():.2e} / {np.max(bounds[k]):.1e}")
            assert not np.isnan(g).any() and (err <= bounds[k]).all(), (m, k, err.max(), np.max(bounds[k]))


# ------------------------------------------------------------------------ 3. per-member outcomes
@FORMS
def test_failures_stay_inside_their_member(full):
    S, D, B, T = 3, 3, 6, 70
    models, x, L = make_stack(full, 300, 4, S, D, B, T, lengths=[70, 1, 0, 66, 1, 70])
    x = x.copy()
    x[3, 40, 1] = np.nan                       # sequence 3: a NaN inside its length
    bad = list(models[1])                      # member 1: degenerate parameters
    last = bad[3].copy()
    if full:
        last[1, 0, 0] = -1.0                   # a non-positive prec_chol diagonal
    else:
        last[1, 2] = np.nan
    bad[3] = last
    imp = list(models[2])                      # member 2: every way out of the only start state is closed
    imp[0] = np.array([0.0, NINF, NINF], np.float32)
    imp[1] = imp[1].copy()
    imp[1][0, :] = NINF
    stack = [models[0], tuple(bad), tuple(imp), models[3]]
    got = raw_batched(full, stack, x, L)
    ll = got["loglik"].cpu().numpy()
    # member 1: everything NaN, nothing counted
    assert np.isnan(ll[1]).all() and not got["gamma"][1].any()
    for k in COUNTS:
        assert not got[k][1].any() and not torch.isnan(got[k][1]).any(), k
    # member 2: the sequences longer than 1 are impossible, the NaN and the empty one NaN
    assert ll[2, 0] == NINF and ll[2, 5] == NINF and np.isnan(ll[2, [2, 3]]).all() and np.isfinite(ll[2, [1, 4]]).all()
    assert not got["gamma"][2][[0, 2, 3, 5]].any() and not got["trans_cnt"][2].any()
    assert abs(got["occ"][2].sum().item() - 2.0) <= 2e-5
    # members 0 and 3: the flagged sequences only
    for m in (0, 3):
        assert np.isnan(ll[m, [2, 3]]).all() and np.isfinite(ll[m, [0, 1, 4, 5]]).all()
        assert not got["gamma"][m][[2, 3]].any()
    # ... whose contribution is exactly zero: the counts are those of the batch without them
    keep = [0, 1, 4, 5]
    for m in (0, 3):
        ref = E.estep_ens_ref([stack[m]], x[keep], L[keep], full=full,
                              ems=raw_emissions(full, [stack[m]], x[keep], L[keep]))[0]
        bounds = E.weighted_bounds(ref["abs_w"], x[keep], L[keep], None, full)
        for k in COUNTS:
            assert (np.abs(got[k][m].cpu().numpy() - ref[k]) <= bounds[k]).all(), (m, k)
    # every other member is bit-identical to the call without the bad members
    without = raw_batched(full, [models[0], models[3]], x, L)
    for j, m in enumerate((0, 3)):
        for k in OUT:
            assert same_bits(got[k][m], without[k][j]), (m, k)
    only_imp = raw_batched(full, [tuple(imp)], x, L)
    for k in OUT:
        assert same_bits(got[k][2], only_imp[k][0]), k


# ---------------------------------------------------------------------------- 4. padded members
def gauss_model(full, model, mixture=False):
    """A vqhmm.GaussianHMM on the device holding the reference model (last = log_var, or scale_tril for full)."""
    import vqhmm
    S, D = model[2].shape
    h = vqhmm.GaussianHMM(S, D, "full" if full else "diag").cuda()
    with torch.no_grad():
        h.log_pi.copy_(torch.from_numpy(np.asarray(model[0], np.float32)))
        h.log_A.copy_(torch.from_numpy(np.asarray(model[1], np.float32)))
        h.mean.copy_(torch.from_numpy(np.asarray(model[2], np.float32)))
        (h.scale_tril if full else h.log_var).copy_(torch.from_numpy(np.asarray(model[3], np.float32)))
    if mixture:
        h.as_mixture()
    return h


def hmm_models(full, seed, sizes, D, B, T):
    """One GaussianHMM per size with random parameters, and data -> (hmms, x device, L device, x, L)."""
    hmms = []
    x = L = None
    for i, s in enumerate(sizes):
        mk = HF.make_case if full else H.make_case
        lengths = np.r_[T, np.random.default_rng(seed).integers(1, T, B - 1)]
        model, xs, Ls = mk(seed + 10 * i, B, T, s, D, lengths=lengths)
        if i == 0:
            x, L = xs, Ls
        if full:
            model = model[:3] + (F.scale_tril_of(model[3]).astype(np.float32),)
        hmms.append(gauss_model(full, model))
    return hmms, torch.from_numpy(x).cuda(), torch.from_numpy(L).cuda(), x, L


def params(h):
    return [h.log_pi, h.log_A, h.mean, h.scale_tril if h.full else h.log_var]


@FORMS
def test_padded_members(full):
    import vqhmm
    sizes, D, B, T = (2, 3, 5), 3, 5, 40
    hmms, d_x, d_L, x, L = hmm_models(full, 400, sizes, D, B, T)
    ens = vqhmm.GaussianHMMEnsemble.from_models(hmms)
    assert ens.num_states == 5 and ens.member_states == [2, 3, 5]
    st = ens.e_step(d_x, d_L, return_gamma=True)
    for m, s in enumerate(sizes):
        one = hmms[m].e_step(d_x, d_L, return_gamma=True)
        rel_ok(st["loglik"][m].cpu().numpy(), one["loglik"].cpu().numpy().astype(np.float64))
        assert not st["gamma"][m][:, :, s:].any() and not st["occ"][m, s:].any()
        assert not st["m1"][m, s:].any() and not st["m2"][m, s:].any() and not st["pi_cnt"][m, s:].any()
        assert not st["trans_cnt"][m, s:].any() and not st["trans_cnt"][m, :, s:].any()
        assert (st["gamma"][m][:, :, :s] - one["gamma"]).abs().max().item() <= 2e-5   # 1e-5 each against fp64
    ens.fit(d_x, d_L, n_iter=3)
    last = ens.scale_tril if full else ens.log_var
    for m, s in enumerate(sizes):
        assert torch.isneginf(ens.log_pi[m, s:]).all() and not torch.isnan(ens.log_pi[m]).any()
        assert torch.isneginf(ens.log_A[m, s:]).all() and torch.isneginf(ens.log_A[m, :, s:]).all()
        assert not torch.isnan(ens.log_A[m]).any() and torch.isfinite(ens.mean[m]).all()
        for j in range(s, 5):
            assert torch.equal(ens.mean[m, j], ens.mean[m, 0]) and torch.equal(last[m, j], last[m, 0])
        h = ens.member(m)
        assert h.num_states == s and torch.equal(h.mean, ens.mean[m, :s])


# -------------------------------------------------- 5. one EM iteration vs separate GaussianHMMs
def ulp_distance(a, b):
    """Distance in fp32 steps between finite same-sign values."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return (ia - ib).abs().max().item()


@FORMS
@pytest.mark.parametrize("mixture", [False, True], ids=["hmm", "mixture"])
def test_one_em_iteration_equals_separate_models(full, mixture):
    import vqhmm
    hmms, d_x, d_L, x, L = hmm_models(full, 500, (4, 4, 4), 3, 6, 70)
    if mixture:
        for h in hmms:
            h.as_mixture()
    ens = vqhmm.GaussianHMMEnsemble.from_models(hmms)
    shift = torch.from_numpy(E.data_shift(x, L)).cuda()
    st = ens.e_step(d_x, d_L, shift=shift)
    ens.m_step(st, prior_count=0.1)
    for m, h in enumerate(hmms):
        one = h.e_step(d_x, d_L, shift=shift)
        for k in COUNTS + ("loglik",):
            assert same_bits(st[k][m], one[k]), (m, k)
        h.m_step(one, prior_count=0.1)
        mine = [ens.log_pi[m], ens.log_A[m], ens.mean[m], (ens.scale_tril if full else ens.log_var)[m]]
        for name, a, b in zip(("log_pi", "log_A", "mean", "last"), mine, params(h)):
            if full and name in ("mean", "last"):
                # the batched and the single fp64 Cholesky may differ in the last fp64 bits: one fp32 step at most
                assert ulp_distance(a, b.detach()) <= 1, (m, name)
            else:
                assert same_bits(a, b.detach()), (m, name)


# ------------------------------------------------------------------------------ 6. fit(n_init=R)
@FORMS
def test_fit_n_init_1_is_the_plain_fit_and_tol_is_refused(full):
    hmms, d_x, d_L, x, L = hmm_models(full, 600, (3, 3), 3, 6, 50)
    with torch.no_grad():
        for p, q in zip(params(hmms[1]), params(hmms[0])):
            p.copy_(q)
    ha = hmms[0].fit(d_x, d_L, n_iter=3, n_init=1, generator=torch.Generator().manual_seed(1))
    hb = hmms[1].fit(d_x, d_L, n_iter=3, generator=torch.Generator().manual_seed(1))
    assert [v.item() for v in ha] == [v.item() for v in hb]
    for p, q in zip(params(hmms[0]), params(hmms[1])):
        assert same_bits(p.detach(), q.detach())
    with pytest.raises(ValueError):
        hmms[0].fit(d_x, d_L, n_iter=2, tol=1e-4, n_init=2)
    with pytest.raises(ValueError):
        hmms[0].fit(d_x, d_L, n_iter=2, n_init=0)


@FORMS
def test_fit_n_init_4(full):
    """Column m of the ensemble's history is the plain fit(init=None) from member m's start: the same E-step bits
    and, for "diag", the same M-step bits, so the totals (fp64 sums of a handful of fp32 values of like magnitude,
    exact in any order) are equal; for "full" the Cholesky may move a parameter by one fp32 step per iteration, and
    the totals are held to the header's loglik tolerance, 1e-5 of sum_b max(1, |loglik_b|)."""
    R, n_iter = 4, 3
    hmms, d_x, d_L, x, L = hmm_models(full, 700, (3,), 3, 6, 50)
    hmm = hmms[0]
    ens = hmm._restart_ensemble(R, d_x, d_L, torch.Generator().manual_seed(5))
    assert ens.num_models == R
    first = [ens.log_pi[0], ens.log_A[0], ens.mean[0], (ens.scale_tril if full else ens.log_var)[0]]
    for a, b in zip(params(hmm), first):
        assert same_bits(a.detach(), b)
    starts = [ens.member(m) for m in range(R)]
    # the fresh members: means at distinct rows of x, the data's variance, normalised rows
    rows = {tuple(r) for b in range(x.shape[0]) for r in x[b, :L[b]].tolist()}
    for m in range(1, R):
        got = [tuple(r) for r in starts[m].mean.cpu().tolist()]
        assert len(set(got)) == 3 and all(r in rows for r in got)
        assert abs(torch.exp(starts[m].log_pi.double()).sum().item() - 1.0) <= 1e-6
    hist = ens.fit(d_x, d_L, n_iter=n_iter)
    assert hist.shape == (n_iter, R) and hist.dtype == torch.float64 and hist.is_cuda
    finals = []
    for m in range(R):
        h = starts[m].fit(d_x, d_L, n_iter=n_iter, init=None)
        col = hist[:, m].cpu().numpy()
        one = np.array([v.item() for v in h])
        if full:
            slack = 1e-5 * np.maximum(1.0, np.abs(starts[m].log_prob(d_x, d_L).double().cpu().numpy())).sum()
            assert (np.abs(col - one) <= slack).all(), (m, col, one)
        else:
            assert np.array_equal(col, one), (m, col, one)
        finals.append(float(np.nansum(starts[m].log_prob(d_x, d_L).double().cpu().numpy())))
    # the model ends as the argmax member, with its history
    out = hmm.fit(d_x, d_L, n_iter=n_iter, init=None, n_init=R, generator=torch.Generator().manual_seed(5))
    assert len(out) == n_iter and all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 for v in out)
    best = int(ens.best_index(d_x, d_L).item())
    order = np.argsort(finals)
    if finals[order[-1]] - finals[order[-2]] > 1e-3 * abs(finals[order[-1]]):   # decided beyond the tolerances
        assert best == int(order[-1])
    mine = [ens.log_pi[best], ens.log_A[best], ens.mean[best], (ens.scale_tril if full else ens.log_var)[best]]
    for a, b in zip(params(hmm), mine):
        assert same_bits(a.detach(), b)
    assert [v.item() for v in out] == hist[:, best].cpu().tolist()


# ------------------------------------------------------------------------------------------ 7. BIC
def selection_ensemble(full):
    import vqhmm
    x, L, starts = E.selection_case(full)
    ens = vqhmm.GaussianHMMEnsemble.from_models([gauss_model(full, m) for m in starts])
    return ens, torch.from_numpy(x).cuda(), torch.from_numpy(L).cuda(), x, L, starts


@FORMS
def test_bic_formula_and_planted_selection(full):
    ens, d_x, d_L, x, L, starts = selection_ensemble(full)
    assert ens.member_states == list(E.SEL_SIZES)
    p = ens.num_free_parameters().cpu().numpy()
    assert p.tolist() == [E.num_free_parameters_ref(m, full) for m in starts]
    ens.fit(d_x, d_L, n_iter=E.SEL_ITERS)
    ll = ens.log_prob(d_x, d_L).double().nansum(1).cpu().numpy()
    npos = int(np.clip(L, 0, x.shape[1]).sum())
    want = np.array([E.bic_ref(ll[m], p[m], npos) for m in range(3)])
    bic = ens.bic(d_x, d_L).cpu().numpy()
    assert np.allclose(bic, want, rtol=1e-12, atol=0), (bic, want)
    ref_bic = E.selection_ref(full)[0]
    print("bic", bic, "reference", ref_bic)
    assert E.SEL_SIZES[int(np.argmin(bic))] == 3
    # a mixture's transitions are its pi again
    mix = type(ens).from_models([gauss_model(full, m, mixture=True) for m in starts])
    D = E.SEL_D
    per = D + D * (D + 1) // 2 if full else 2 * D
    assert mix.num_free_parameters().cpu().tolist() == [2 * (s - 1) + s * per for s in E.SEL_SIZES]


# ---------------------------------------------------------------------------------- 8. fit_mixture
def mixture_case(full):
    rng = np.random.default_rng(8)
    D, T = 2, 12
    x = np.concatenate([c + rng.standard_normal((5, T, D)) for c in (-3.0, 3.0)]).astype(np.float32)
    L = np.full(10, T, np.int64)
    L[[2, 7]] = [5, 9]
    models = []
    for m in range(2):
        lp, A, mean, _ = G.random_model(np.random.default_rng(80 + m), 2, D)
        if full:
            last = np.repeat(np.eye(D, dtype=np.float32)[None] * 2.0, 2, 0)
        else:
            last = np.full((2, D), np.log(4.0), np.float32)
        models.append((lp, A, mean, last))
    return x, L, models


@FORMS
def test_fit_mixture_one_iteration_and_monotone(full):
    import vqhmm
    x, L, models = mixture_case(full)
    d_x, d_L = torch.from_numpy(x).cuda(), torch.from_numpy(L).cuda()
    ens = vqhmm.GaussianHMMEnsemble.from_models([gauss_model(full, m) for m in models])
    ref_models = [m[:3] + (np.einsum("sij,skj->sik", m[3].astype(np.float64), m[3].astype(np.float64)),)
                  for m in models] if full else models
    shift = E.data_shift(x, L)
    ref_hist, ref_out, ref_mix, ref_r = E.mixture_ref(ref_models, np.log([0.5, 0.5]), x, L, n_iter=1, shift=shift,
                                                      full=full)
    r = ens.responsibilities(d_x, d_L).cpu().numpy()
    # r moves by at most the two logliks' tolerance (softmax is 1-Lipschitz in its arguments)
    ll_ref = np.stack([e["loglik"] for e in E.estep_ens_ref(E._for_estep(ref_models, full), x, L, full=full)])
    slack = 1e-5 * np.maximum(1.0, np.abs(ll_ref)).sum(0)
    assert (np.abs(r - ref_r) <= 2 * slack[None, :] + 1e-12).all()
    hist = ens.fit_mixture(d_x, d_L, n_iter=1)
    assert hist.shape == (1,) and hist.dtype == torch.float64 and hist.is_cuda
    assert abs(hist[0].item() - ref_hist[0]) <= slack.sum()
    assert np.abs(np.exp(ens.log_mix.double().cpu().numpy()) - np.exp(ref_mix)).max() <= 2 * slack.max() + 1e-6
    # a mean is a ratio of sums over the 10 sequences weighted by r: moving every r by 2 slack moves it by at most
    # 10 x 2 slack x the data's extent (the E-step's own 2e-5 per position is far below that)
    tol = 10 * 2 * slack.max() * np.abs(x).max() + 1e-4
    for m in range(2):
        assert np.abs(ens.mean[m].cpu().numpy() - ref_out[m][2]).max() <= tol
    # five more: the exact EM never decreases the mixture log-likelihood beyond the logliks' tolerance
    hist = ens.fit_mixture(d_x, d_L, n_iter=5).cpu().numpy()
    print("mixture history", hist, "slack", slack.sum())
    assert np.isfinite(hist).all() and (np.diff(hist) >= -2 * slack.sum()).all(), hist


# --------------------------------------------------------------- 9. determinism and graph capture
@FORMS
def test_deterministic_and_graph_capturable(full):
    from vqhmm import _ext
    M, S, D, B, T = 3, 4, 3, 6, 70
    models, x, L = make_stack(full, 900, M, S, D, B, T)
    a = raw_batched(full, models, x, L)
    b = raw_batched(full, models, x, L)
    for k in OUT:
        assert same_bits(a[k], b[k]), k
    size, entry = _entries(full)
    log_pi, log_A, mean, last = (dev_f32(np.stack([m[k] for m in models])) for k in range(4))
    d_x, d_len = dev_f32(x), torch.from_numpy(L).cuda()
    shapes = ((M, S), (M, S, S), (M, S), (M, S, D), (M, S, D, D) if full else (M, S, D))
    cnt = {k: torch.full(sh, float("nan"), dtype=torch.float64, device="cuda") for k, sh in zip(COUNTS, shapes)}
    ll = torch.full((M, B), 7.0, dtype=torch.float32, device="cuda")
    gm = torch.full((M, B, T, S), 7.0, dtype=torch.float32, device="cuda")
    nb = size(B, T, S, D, M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = entry(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(last), _ext.ptr(d_x),
                   _ext.ptr(d_len), None, None, B, T, S, D, M, *(_ext.ptr(cnt[k]) for k in COUNTS), _ext.ptr(ll),
                   _ext.ptr(gm), _ext.ptr(ws), nb, _ext.stream_ptr())
    assert rc == 0, rc
    got = dict(cnt, loglik=ll, gamma=gm)
    for _ in range(2):
        for t in cnt.values():
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in OUT:
            assert same_bits(a[k], got[k]), k


# ------------------------------------------------------------------------------------- 10. limits
@FORMS
def test_member_count_limits_and_empty_batches(full):
    size, entry = _entries(full)
    models, x, L = make_stack(full, 950, 2, 2, 3, 3, 5)
    for M in (0, 65536):
        assert size(3, 5, 2, 3, M) == 0
        one = torch.zeros(64, dtype=torch.float64, device="cuda")
        from vqhmm import _ext
        p = _ext.ptr(one)
        rc = entry(p, p, p, p, p, p, None, None, 3, 5, 2, 3, M, p, p, p, p, p, None, None, p, 512, _ext.stream_ptr())
        assert rc == EUNSUPPORTED, (M, rc)
    assert size(3, 5, 2, 3, 65535) == 65535 * size(3, 5, 2, 3, 1) and size(3, 5, 2, 3, 1) % 256 == 0
    for B, T in ((3, 0), (0, 5)):
        got = raw_batched(full, models, np.zeros((B, T, 3), np.float32), np.zeros(B, np.int64))
        for k in COUNTS:
            assert not got[k].any() and not torch.isnan(got[k]).any(), k
        assert got["loglik"].shape == (2, B) and torch.isnan(got["loglik"]).all()


# ------------------------------------------------------------------------------ 11. member groups
@FORMS
def test_member_groups_give_the_same_bits(full):
    import vqhmm
    hmms, d_x, d_L, x, L = hmm_models(full, 1100, (3, 3, 3, 3, 3), 3, 5, 40)
    ens = vqhmm.GaussianHMMEnsemble.from_models(hmms)
    size, _ = _entries(full)
    per = size(5, 40, 3, 3, 1)
    grouped = vqhmm.GaussianHMMEnsemble.from_models(hmms, max_workspace_bytes=2 * per)   # groups of 2, 2, 1
    w = torch.rand((5, 5), device="cuda")
    a = ens.e_step(d_x, d_L, weights=w, return_gamma=True)
    b = grouped.e_step(d_x, d_L, weights=w, return_gamma=True)
    for k in OUT + ("flat",):
        assert same_bits(a[k], b[k]), k
    tiny = vqhmm.GaussianHMMEnsemble.from_models(hmms, max_workspace_bytes=1)                # one member at a time
    assert same_bits(a["flat"], tiny.e_step(d_x, d_L, weights=w)["flat"])
