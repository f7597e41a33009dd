"""GPU checks of the HMM on code indices (vqhmm_code_estep_f32 / vqhmm_code_sample_f32, hmm_code.hip,
vqhmm.CodeHMM) against the fp64 restatement in tests/code_hmm_ref.py, fed the same fp32 parameters.

Bounds: the per-position contracts of include/vqhmm.h (gamma abs 1e-5, xi abs 2e-5, loglik rel 1e-5
against max(1, |ref|)), summed for the counts: trans_cnt 2e-5 x (transition positions of the batch),
emit_cnt[s,v] 1e-5 x (in-length positions carrying code v), pi_cnt 1e-5 x (sequences with L > 0).
The sampler is compared exactly: tests/test_code_hmm_ref.py vets the uniforms' distance from every
CDF boundary.
"""
import numpy as np
import pytest
import torch

import code_hmm_ref as R
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
NINF = -np.inf


def ragged(seed, B, T):
    """Lengths with T, 0, 1 and 2 first (as far as B and T allow), then random ones."""
    rng = np.random.default_rng(seed)
    L = np.concatenate([[T, 0, 1, 2], rng.integers(0, T + 1, max(B - 4, 0))])[:B]
    return np.minimum(L, T).astype(np.int64)


def dev_f32(a, offset=False):
    a = np.ascontiguousarray(a, np.float32)
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def dev_i32(a, offset=False):
    a = np.ascontiguousarray(a, np.int32)
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.int32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4
    return t


def raw_estep(model, codes, lengths, loglik=True, gamma=True, offset=False):
    """vqhmm_code_estep_f32 through ctypes on guarded exact-size buffers (gpu_buffers.guarded) and a
    guarded, poisoned workspace of exactly the queried size; the counts start as NaN (the call must write
    every element) -> dict of device tensors."""
    from vqhmm import _ext
    lib = _ext.load()
    log_pi, log_A, log_B = (dev_f32(a, offset) for a in model)
    S, V = log_B.shape
    B, T = codes.shape
    d_codes = dev_i32(codes, offset)
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    cnt = [guarded(sh, torch.float64, fill=float("nan")) for sh in ((S,), (S, S), (S, V))]
    ll = guarded((B,), torch.float32, fill=7.0) if loglik else None
    gm = guarded((B, T, S), torch.float32, fill=7.0) if gamma else None
    nb = lib.vqhmm_code_estep_workspace_size(B, T, S, V)
    ws = guarded(nb, torch.uint8)
    rc = lib.vqhmm_code_estep_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(log_B), _ext.ptr(d_codes),
                                  _ext.ptr(d_len), B, T, S, V, cnt[0].ptr, cnt[1].ptr, cnt[2].ptr,
                                  ll.ptr if loglik else None, gm.ptr if gamma else None, ws.ptr, nb, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(*cnt, ll, gm, ws)
    return dict(pi_cnt=cnt[0].t, trans_cnt=cnt[1].t, emit_cnt=cnt[2].t, loglik=ll.t if loglik else None,
                gamma=gm.t if gamma else None)


def rel_ok(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (got, ref)
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf])
    ok = ~(nan | inf)
    err = np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
    assert err.max(initial=0) <= tol, err.max()
    return err.max(initial=0)


def count_bounds(ref, codes, lengths, V):
    """(pi, trans, emit (V,)) bounds: the per-position contracts summed over the sequences that count."""
    B, T = codes.shape
    L = np.clip(np.asarray(lengths, np.int64), 0, T)
    counted = np.isfinite(ref["loglik"])
    n_pi = int((counted & (L > 0)).sum())
    n_tr = int(np.maximum(L[counted] - 1, 0).sum())
    n_v = np.zeros(V)
    for b in np.nonzero(counted)[0]:
        n_v += np.bincount(codes[b, :L[b]], minlength=V)[:V]
    return 1e-5 * n_pi, 2e-5 * n_tr, 1e-5 * n_v


def check_counts(got, ref, codes, lengths, V, tag=""):
    b_pi, b_tr, b_em = count_bounds(ref, codes, lengths, V)
    pi, tr, em = (got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k] for k in ("pi_cnt", "trans_cnt", "emit_cnt"))
    assert pi.dtype == np.float64 and tr.dtype == np.float64 and em.dtype == np.float64
    assert not (np.isnan(pi).any() or np.isnan(tr).any() or np.isnan(em).any())
    e_pi = np.abs(pi - ref["pi_cnt"]).max()
    e_tr = np.abs(tr - ref["trans_cnt"]).max()
    e_em = np.abs(em - ref["emit_cnt"])
    print(f"{tag} pi {e_pi:.2e}/{b_pi:.1e} trans {e_tr:.2e}/{b_tr:.1e} emit {e_em.max():.2e}/{b_em.max():.1e}")
    assert e_pi <= b_pi and e_tr <= b_tr
    assert (e_em <= b_em[None, :]).all(), (e_em - b_em[None, :]).max()


def check_case(model, codes, lengths, offset=False, tag=""):
    S, V = model[2].shape
    ref = R.estep_ref(*model, codes, lengths)
    got = raw_estep(model, codes, lengths, offset=offset)
    e_ll = rel_ok(got["loglik"].cpu().numpy(), ref["loglik"])
    gm = got["gamma"].cpu().numpy()
    e_g = np.abs(gm - ref["gamma"]).max(initial=0)
    print(f"{tag} S={S} V={V} B={codes.shape[0]} T={codes.shape[1]}: gamma {e_g:.2e} loglik {e_ll:.2e}")
    assert not np.isnan(gm).any() and e_g <= 1e-5
    for b in range(codes.shape[0]):
        n = int(min(max(lengths[b], 0), codes.shape[1]))
        assert not gm[b, n:].any()
    check_counts(got, ref, codes, lengths, V, tag)
    return ref, got


def make_case(seed, S, V, B, T, scale=1.5, lengths=None):
    rng = np.random.default_rng(seed)
    model = R.random_model(rng, S, V, scale)
    codes = rng.integers(0, V, size=(B, T)).astype(np.int32)
    L = ragged(seed + 1, B, T) if lengths is None else np.asarray(lengths, np.int64)
    for b in range(B):
        codes[b, int(L[b]):] = -1  # the Viterbi path's padding: never interpreted
    return model, codes, L


# ------------------------------------------------------------------------------ E-step
@pytest.mark.parametrize("V", (1, 5, 64))
@pytest.mark.parametrize("S", (1, 2, 3, 5, 8))
def test_estep_narrow(S, V):
    check_case(*make_case(10 * S + V, S, V, 37, 65))


@pytest.mark.parametrize("V", (7, 512))
@pytest.mark.parametrize("S", (9, 16, 17, 32))
def test_estep_wide(S, V):
    check_case(*make_case(20 * S + V, S, V, 5, 40))


@pytest.mark.parametrize("T", (1, 2, 63, 64, 65, 130))
def test_estep_chunk_edges(T):
    check_case(*make_case(300 + T, 4, 9, 6, T))


@pytest.mark.parametrize("S", (3, 8, 17))
@pytest.mark.parametrize("L", (1, 2, 3))
def test_estep_single_short_sequence(S, L):
    """B = 1: the count bounds collapse to a few 1e-5, so a dropped or doubled end step cannot hide."""
    check_case(*make_case(400 + 10 * S + L, S, 6, 1, 4, lengths=[L]))


def test_estep_long_sequence():
    check_case(*make_case(500, 4, 16, 3, 2048, lengths=[2048, 2048, 1999]))


def test_estep_peaked_tables():
    """log_A scaled x8, log_B with entries near log(1e-30) and exact -inf: steps leave the fast range."""
    rng = np.random.default_rng(600)
    S, V, B, T = 5, 12, 9, 70
    log_pi, log_A, log_B = R.random_model(rng, S, V)
    log_A = (log_A * 8).astype(np.float32)
    log_B = log_B.copy()
    log_B[rng.random((S, V)) < 0.25] = np.float32(np.log(1e-30))
    log_B[:, 0] = np.maximum(log_B[:, 0], -1.0)  # code 0 stays likely everywhere
    log_B[:, 5] = (np.log(1e-30) - rng.random(S)).astype(np.float32)  # a code that is unlikely in every state
    log_B[2, 3] = NINF
    log_B[4, 7] = NINF
    log_A[1, 3] = NINF
    log_A[4, 0] = NINF
    codes = rng.integers(0, V - 1, size=(B, T)).astype(np.int32)  # code V - 1 never occurs
    L = ragged(601, B, T)
    model = (log_pi, log_A, log_B)
    ref, got = check_case(model, codes, L, tag="peaked")
    tr = got["trans_cnt"].cpu().numpy()
    assert tr[1, 3] == 0.0 and tr[4, 0] == 0.0
    assert np.isfinite(ref["loglik"][L > 0]).all()
    # an -inf column at the code that never occurs changes nothing
    log_B2 = log_B.copy()
    log_B2[:, V - 1] = NINF
    got2 = raw_estep((log_pi, log_A, log_B2), codes, L)
    for k in ("pi_cnt", "trans_cnt", "emit_cnt", "loglik", "gamma"):
        assert torch.equal(got[k].view(torch.uint8), got2[k].view(torch.uint8)), k


@pytest.mark.parametrize("bad", ("both", "V", "-1"))
def test_estep_degenerate_sequences(bad):
    """An impossible sequence and one with an out-of-range code (V and -1 inside the length) in a batch of
    4: -inf / NaN loglik, zero contribution, the other two untouched."""
    rng = np.random.default_rng(700)
    S, V, T = 3, 6, 20
    log_pi, log_A, log_B = R.random_model(rng, S, V)
    log_B[1:, 0] = NINF   # only state 0 emits code 0 ...
    log_A[0, 0] = NINF    # ... and it never follows itself
    model = (log_pi, log_A, log_B)
    codes = rng.integers(1, V, size=(4, T)).astype(np.int32)
    L = np.array([T, 15, 17, T - 1], np.int64)
    codes[0, :] = np.where(np.arange(T) % 2 == 0, 0, codes[0, :])  # possible: code 0 never twice running
    codes[1, 7] = codes[1, 8] = 0   # impossible
    if bad in ("both", "V"):
        codes[2, 9] = V             # out of range, inside the length
    if bad in ("both", "-1"):
        codes[2, 0 if bad == "-1" else 16] = -1
    ref, got = check_case(model, codes, L, tag="degenerate")
    ll = got["loglik"].cpu().numpy()
    assert ll[1] == NINF and np.isnan(ll[2]) and np.isfinite(ll[[0, 3]]).all()
    gm = got["gamma"].cpu().numpy()
    assert not gm[[1, 2]].any()
    # the counts and the others' gamma equal those of the two ordinary sequences alone
    keep = [0, 3]
    ref2 = R.estep_ref(*model, codes[keep], L[keep])
    got2 = raw_estep(model, codes[keep], L[keep])
    check_counts(got, ref2, codes[keep], L[keep], V, "others")
    assert torch.equal(got["gamma"][keep].view(torch.int32), got2["gamma"].view(torch.int32))
    assert torch.equal(got["loglik"][keep].view(torch.int32), got2["loglik"].view(torch.int32))
    # codes past the length are never interpreted
    codes3 = codes.copy()
    for b in range(4):
        codes3[b, int(L[b]):] = 1 << 30
    got3 = raw_estep(model, codes3, L)
    for k in ("pi_cnt", "trans_cnt", "emit_cnt", "loglik", "gamma"):
        assert torch.equal(got[k].view(torch.uint8), got3[k].view(torch.uint8)), k


def test_estep_past_the_lds_tier():
    check_case(*make_case(800, 32, 4096, 4, 33))


def test_estep_largest_lds_tier():
    """S = 8, V = 512: the table and four fp64 slabs fill most of the CU's LDS (the benchmark's shape)."""
    check_case(*make_case(850, 8, 512, 9, 40))


def test_estep_unaligned_inputs_and_int64_codes():
    import vqhmm
    model, codes, L = make_case(900, 8, 64, 7, 70)
    ref, got = check_case(model, codes, L, offset=True, tag="offset")
    base = raw_estep(model, codes, L)
    for k in ("pi_cnt", "trans_cnt", "emit_cnt", "loglik", "gamma"):
        assert torch.equal(got[k].view(torch.uint8), base[k].view(torch.uint8)), k
    hmm = vqhmm.CodeHMM(8, 64).cuda()
    hmm.load_state_dict(dict(zip(("log_pi", "log_A", "log_B"), (torch.from_numpy(a) for a in model))))
    for dt in (torch.int64, torch.int32):
        out = hmm.e_step(torch.from_numpy(codes).to(dt).cuda(), torch.from_numpy(L), return_gamma=True)
        for k in ("pi_cnt", "trans_cnt", "emit_cnt", "loglik", "gamma"):
            assert torch.equal(out[k].view(torch.uint8), base[k].view(torch.uint8)), (dt, k)
    d_codes, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(L)
    assert torch.equal(hmm.log_prob(d_codes, d_len).view(torch.int32), base["loglik"].view(torch.int32))
    assert torch.equal(hmm.posterior(d_codes, d_len).view(torch.int32), base["gamma"].view(torch.int32))


def test_estep_nullable_outputs_same_counts():
    model, codes, L = make_case(1000, 5, 17, 11, 66)
    full = raw_estep(model, codes, L)
    for ll, gm in ((True, False), (False, True), (False, False)):
        part = raw_estep(model, codes, L, loglik=ll, gamma=gm)
        for k in ("pi_cnt", "trans_cnt", "emit_cnt"):
            assert torch.equal(part[k].view(torch.int64), full[k].view(torch.int64)), (ll, gm, k)
        if ll:
            assert torch.equal(part["loglik"].view(torch.int32), full["loglik"].view(torch.int32))
        if gm:
            assert torch.equal(part["gamma"].view(torch.int32), full["gamma"].view(torch.int32))


def test_estep_deterministic():
    """B = 300: more than one workgroup's slab takes part in the reduction."""
    model, codes, L = make_case(1100, 8, 64, 300, 65)
    a = raw_estep(model, codes, L)
    b = raw_estep(model, codes, L)
    for k in ("pi_cnt", "trans_cnt", "emit_cnt", "loglik", "gamma"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    ref = R.estep_ref(*model, codes, L)
    check_counts(a, ref, codes, L, 64, "B=300")


def test_estep_empty_batches():
    model, _, _ = make_case(1200, 3, 5, 2, 4)
    for B, T in ((0, 4), (2, 0), (0, 0)):
        got = raw_estep(model, np.zeros((B, T), np.int32), np.zeros(B, np.int64))
        for k in ("pi_cnt", "trans_cnt", "emit_cnt"):
            assert not got[k].cpu().numpy().any(), (B, T, k)
        assert np.isnan(got["loglik"].cpu().numpy()).all()


def test_estep_matches_forward_backward():
    """The library's own forward-backward on the broadcast tables: gamma and loglik within the sum of the
    two contracts (gamma 2e-5, logZ rel 2e-5)."""
    import vqhmm
    S, V, B, T = 8, 16, 8, 130
    model, codes, L = make_case(1300, S, V, B, T)
    got = raw_estep(model, codes, L)
    log_pi, log_A, log_B = (torch.from_numpy(a).cuda() for a in model)
    c = torch.from_numpy(np.maximum(codes, 0)).long().cuda()
    em = log_B[:, c].permute(1, 2, 0).contiguous()
    gamma, logZ = vqhmm.forward_backward(log_pi, log_A.expand(B, T, S, S).contiguous(), em, torch.from_numpy(L))
    assert (got["gamma"] - gamma).abs().max().item() <= 2e-5
    rel_ok(got["loglik"].cpu().numpy(), logZ.cpu().numpy().astype(np.float64), tol=2e-5)


def test_estep_graph_capture():
    """The call is capturable (no host sync, no allocation) and replays to the same bits."""
    from vqhmm import _ext
    lib = _ext.load()
    model, codes, L = make_case(1400, 4, 9, 6, 70)
    base = raw_estep(model, codes, L)
    S, V = 4, 9
    B, T = codes.shape
    d = [dev_f32(a) for a in model]
    d_codes, d_len = dev_i32(codes), torch.from_numpy(L).cuda()
    cnt = [torch.zeros(sh, dtype=torch.float64, device="cuda") for sh in ((S,), (S, S), (S, V))]
    ll = torch.zeros(B, device="cuda")
    nb = lib.vqhmm_code_estep_workspace_size(B, T, S, V)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.vqhmm_code_estep_f32(_ext.ptr(d[0]), _ext.ptr(d[1]), _ext.ptr(d[2]), _ext.ptr(d_codes), _ext.ptr(d_len),
                                      B, T, S, V, _ext.ptr(cnt[0]), _ext.ptr(cnt[1]), _ext.ptr(cnt[2]), _ext.ptr(ll),
                                      None, _ext.ptr(ws), nb, _ext.stream_ptr())
    assert rc == 0
    for _ in range(2):
        for t in cnt:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for got, k in zip(cnt, ("pi_cnt", "trans_cnt", "emit_cnt")):
            assert torch.equal(got.view(torch.int64), base[k].view(torch.int64)), k
        assert torch.equal(ll.view(torch.int32), base["loglik"].view(torch.int32))


# ---------------------------------------------------------------------------------- EM
def _sample_host(rng, log_pi, log_A, log_B, B, T):
    pi, A, Bm = np.exp(log_pi.astype(np.float64)), np.exp(log_A.astype(np.float64)), np.exp(log_B.astype(np.float64))
    codes = np.zeros((B, T), np.int32)
    for b in range(B):
        z = rng.choice(len(pi), p=pi / pi.sum())
        for t in range(T):
            if t:
                z = rng.choice(len(pi), p=A[z] / A[z].sum())
            codes[b, t] = rng.choice(Bm.shape[1], p=Bm[z] / Bm[z].sum())
    return codes


def test_em_fit():
    import vqhmm
    S, V, B, T = 3, 8, 16, 64
    rng = np.random.default_rng(2000)
    truth = R.random_model(rng, S, V, scale=2.0)
    codes = _sample_host(rng, *truth, B, T)
    L = np.concatenate([[T, 40, 1], rng.integers(2, T + 1, B - 3)]).astype(np.int64)
    hmm = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(5)).cuda()
    d_codes, d_len = torch.from_numpy(codes).cuda(), torch.from_numpy(L).cuda()
    hist = []
    for it in range(6):
        before = tuple(getattr(hmm, k).cpu().numpy() for k in ("log_pi", "log_A", "log_B"))
        ll = hmm.fit(d_codes, d_len, n_iter=1)
        assert len(ll) == 1 and torch.is_tensor(ll[0]) and ll[0].is_cuda  # tol=None: no host sync in the loop
        # this iteration's E-step against the helper on the parameters going in (not a trajectory comparison)
        ref = R.estep_ref(*before, codes, L)
        got = hmm_counts = raw_estep(before, codes, L, gamma=False)
        check_counts(got, ref, codes, L, V, f"EM it {it}")
        assert abs(ll[0].item() - ref["loglik"].sum()) <= 1e-5 * max(1.0, abs(ref["loglik"].sum()))
        # ... and the M-step that followed is the helper's on the GPU's own counts
        want = R.mstep_ref({k: hmm_counts[k].cpu().numpy() for k in ("pi_cnt", "trans_cnt", "emit_cnt")}, *before)
        for k, w in zip(("log_pi", "log_A", "log_B"), want):
            p = getattr(hmm, k).cpu().numpy().astype(np.float64)
            # the fp32 rounding of a log of size |w|
            assert (np.abs(p - w) <= 1e-6 * np.maximum(1.0, np.abs(w))).all(), k
            assert np.abs(np.exp(p).sum(-1) - 1).max() <= 1e-6, k
        hist.append(ll[0].item())
    for a, b in zip(hist, hist[1:]):
        assert b >= a - 1e-5 * max(1.0, abs(a)), hist
    assert hist[-1] > hist[0]
    # one call, six iterations: the same trajectory
    hmm2 = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(5)).cuda()
    hist2 = [v.item() for v in hmm2.fit(d_codes, d_len, n_iter=6)]
    assert hist2 == hist
    for k in ("log_pi", "log_A", "log_B"):
        assert torch.equal(getattr(hmm, k), getattr(hmm2, k))
    # state_dict round trip on the device
    hmm3 = vqhmm.CodeHMM(S, V).cuda()
    hmm3.load_state_dict(hmm.state_dict())
    assert torch.equal(hmm3.log_prob(d_codes, d_len), hmm.log_prob(d_codes, d_len))


def test_em_fit_tol_stops_early():
    import vqhmm
    S, V, B, T = 3, 8, 16, 64
    rng = np.random.default_rng(2100)
    truth = R.random_model(rng, S, V, scale=2.0)
    codes = torch.from_numpy(_sample_host(rng, *truth, B, T)).cuda()
    hmm = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(6)).cuda()
    hmm.fit(codes, n_iter=100)  # converge
    hist = hmm.fit(codes, n_iter=50, tol=1e-4)
    assert 2 <= len(hist) < 50 and all(isinstance(v, float) for v in hist)
    assert (hist[-1] - hist[-2]) / (B * T) < 1e-4


# ----------------------------------------------------------------------------- sampler
def raw_sample(model, u):
    from vqhmm import _ext
    lib = _ext.load()
    log_pi, log_A, log_B = (dev_f32(a) for a in model)
    S, V = log_B.shape
    N, T = u.shape[:2]
    d_u = dev_f32(u)
    st = guarded((N, T), torch.int32, fill=-7)
    cd = guarded((N, T), torch.int32, fill=-7)
    rc = lib.vqhmm_code_sample_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(log_B), _ext.ptr(d_u), N, T, S, V,
                                   st.ptr, cd.ptr, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(st, cd)
    return st.t.cpu().numpy(), cd.t.cpu().numpy()


@pytest.mark.parametrize("S,V,seed", R.SAMPLER_CASES)
def test_sampler_exact(S, V, seed):
    log_pi, log_A, log_B, u = R.sampler_case(S, V, seed)
    states, codes, _ = R.sample_ref(log_pi, log_A, log_B, u)
    st, cd = raw_sample((log_pi, log_A, log_B), u)
    assert np.array_equal(st, states) and np.array_equal(cd, codes)


def test_sampler_never_draws_zero_probability():
    rng = np.random.default_rng(3000)
    S, V, N, T = 4, 7, 64, 24
    log_pi, log_A, log_B = R.random_model(rng, S, V)
    log_pi[[0, 3]] = NINF          # first and last category closed
    log_A[:, 2] = NINF
    log_A[1, 3] = NINF
    log_B[:, [0, 6]] = NINF
    log_B[2, 3] = NINF
    u = rng.random((N, T, 2), dtype=np.float32)
    u[:8] = 0.0
    u[8:16] = np.nextafter(np.float32(1), np.float32(0))
    u[16:24, :, 0] = 0.0
    u[16:24, :, 1] = np.nextafter(np.float32(1), np.float32(0))
    st, cd = raw_sample((log_pi, log_A, log_B), u)
    assert st.min() >= 0 and st.max() < S and cd.min() >= 0 and cd.max() < V
    assert np.isfinite(log_pi[st[:, 0]]).all()
    assert np.isfinite(log_A[st[:, :-1], st[:, 1:]]).all()
    assert np.isfinite(log_B[st, cd]).all()
    # u = 0 takes the first open category, the largest u the last open one
    assert (st[:8, 0] == 1).all() and (st[8:16, 0] == 2).all()
    assert (cd[:8] >= 1).all() and (cd[8:16] <= 5).all()


def test_codehmm_sample_reproducible():
    import vqhmm
    hmm = vqhmm.CodeHMM(5, 11, generator=torch.Generator().manual_seed(1)).cuda()
    g = torch.Generator(device="cuda")
    s1, c1 = hmm.sample(16, 20, generator=g.manual_seed(42))
    s2, c2 = hmm.sample(16, 20, generator=g.manual_seed(42))
    s3, c3 = hmm.sample(16, 20, generator=g.manual_seed(43))
    assert s1.dtype == torch.int64 and c1.dtype == torch.int64 and s1.shape == c1.shape == (16, 20)
    assert torch.equal(s1, s2) and torch.equal(c1, c2)
    assert not (torch.equal(s1, s3) and torch.equal(c1, c3))
    # the wrapper's draws are the kernel's rule on its own uniforms
    u = torch.rand((16, 20, 2), generator=g.manual_seed(42), device="cuda").cpu().numpy()
    model = tuple(getattr(hmm, k).cpu().numpy() for k in ("log_pi", "log_A", "log_B"))
    st, cd = raw_sample(model, u)
    assert np.array_equal(st, s1.cpu().numpy()) and np.array_equal(cd, c1.cpu().numpy())


def test_sampler_distribution():
    """S = 32, V = 512, N = 4096, T = 16: state frequencies at t in {0, 1, 15} and the 8 most probable codes'
    frequencies at t = 15 within 6 binomial standard errors of pi A^t and pi A^t B."""
    rng = np.random.default_rng(3100)
    S, V, N, T = 32, 512, 4096, 16
    model = R.random_model(rng, S, V)
    u = rng.random((N, T, 2), dtype=np.float32)
    st, cd = raw_sample(model, u)
    ps, pc = R.state_marginals(*model, T)
    for t in (0, 1, 15):
        f = np.bincount(st[:, t], minlength=S) / N
        se = np.sqrt(ps[t] * (1 - ps[t]) / N)
        assert (np.abs(f - ps[t]) <= 6 * se).all(), (t, np.abs(f - ps[t]) / se)
    top = np.argsort(pc[15])[-8:]
    f = np.bincount(cd[:, 15], minlength=V)[top] / N
    se = np.sqrt(pc[15][top] * (1 - pc[15][top]) / N)
    assert (np.abs(f - pc[15][top]) <= 6 * se).all()


# -------------------------------------------------------------------------- round trip
def test_quantize_fit_sample_round_trip():
    import vqhmm
    g = torch.Generator(device="cuda").manual_seed(7)
    B, Dv, T, K = 4, 8, 32, 8
    z = torch.randn(B, Dv, T, device="cuda", generator=g)
    codebook = torch.randn(K, Dv, device="cuda", generator=g)
    _, idx, _, _ = vqhmm.quantize(z, codebook)
    assert idx.shape == (B, T) and idx.dtype == torch.int32
    hmm = vqhmm.CodeHMM(3, K, generator=torch.Generator().manual_seed(0)).cuda()
    hist = hmm.fit(idx, n_iter=3, prior_count=0.1)
    assert len(hist) == 3 and all(torch.isfinite(v) for v in hist)
    states, codes = hmm.sample(5, 12, generator=g)
    assert states.shape == codes.shape == (5, 12) and states.dtype == codes.dtype == torch.int64
    assert 0 <= int(states.min()) and int(states.max()) < 3 and 0 <= int(codes.min()) and int(codes.max()) < K
    z_q_seq = codebook[codes]
    assert z_q_seq.shape == (5, 12, Dv) and z_q_seq.dtype == torch.float32
    assert hmm.posterior(idx).shape == (B, T, 3) and hmm.log_prob(idx).shape == (B,)
