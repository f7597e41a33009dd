"""GPU checks of GaussianHMM's fused Viterbi decode and causal filter on observations (vqhmm_gauss_viterbi_f32 /
vqhmm_gauss_filter_f32 and the _full_ pair; hmm_gauss_decode_dev.h) against tests/gauss_decode_ref.py, fed the
emission tensor the emission entry wrote on the GPU (the kernels reproduce it on chip bit for bit).

Viterbi is compared bit for bit: with the fp32 restatement of the rule, and with vqhmm.viterbi on the expanded
tables (log_A broadcast to (B,T,S,S), em from the emission entry).  The filter's bounds are the contract's
(include/vqhmm.h): |filt|, |last| abs 1e-5 and loglik rel 1e-5 of max(1, |loglik|) against the fp64
restatement; two filtered results compared with each other (a chunked run against the single call, last
against the E-step's smoothed gamma, loglik against the E-step's) get twice the per-result bound, 2e-5.
"""
import functools

import numpy as np
import pytest
import torch

import gauss_decode_ref as D
import gauss_full_ref as GF
import gauss_hmm_ref as G
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
NINF = -np.inf


def ragged(seed, B, T):
    """Lengths with T, 0, 1 and 2 first (as far as B and T allow), then random ones."""
    rng = np.random.default_rng(seed)
    L = np.concatenate([[T, 0, 1, 2], rng.integers(0, T + 1, max(B - 4, 0))])[:B]
    return np.minimum(L, T).astype(np.int64)


def dev(a, dtype=np.float32, offset=False):
    """`a` on the device in an exact-size buffer, or (offset) at a pointer 4 bytes past a 16-byte boundary."""
    if a is None:
        return None
    a = torch.tensor(np.ascontiguousarray(a, dtype))  # a copy: the shared cases are read-only
    if not offset:
        return a.cuda()
    buf = torch.empty(a.numel() + 1, dtype=a.dtype, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(a)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def out(shape, dtype, offset=False, fill=7):
    """A guarded exact-size output (gpu_buffers.guarded) filled with `fill`; offset: 4 bytes past a 16-byte
    boundary, the guards around that view."""
    g = guarded(shape, dtype, fill=fill, offset=offset)
    assert g.t.data_ptr() % 16 == (4 if offset else 0) or g.nbytes == 0
    return g


def _lib():
    from vqhmm import _ext
    return _ext, _ext.load()


def raw_emission(full, model, x, lengths):
    """The emission entry's tensor (B,T,S) as numpy fp32."""
    _ext, lib = _lib()
    mean, par = dev(model[2]), dev(model[3])
    S, Dm = mean.shape
    B, T = x.shape[:2]
    d_x, d_len = dev(x), dev(lengths, np.int64)
    em = out((B, T, S), torch.float32)
    entry = lib.vqhmm_gauss_full_emission_f32 if full else lib.vqhmm_gauss_emission_f32
    rc = entry(_ext.ptr(mean), _ext.ptr(par), _ext.ptr(d_x), _ext.ptr(d_len), B, T, S, Dm, em.ptr,
               _ext.stream_ptr())
    assert rc == 0, rc
    check_all(em)
    return em.t.cpu().numpy()


def raw_viterbi(full, model, x, lengths, offset=False):
    """The Viterbi entry through ctypes; path and score start as 7 (the call must write every element)."""
    _ext, lib = _lib()
    log_pi, log_A, mean, par = (dev(a, np.float32, offset) for a in model)
    S, Dm = mean.shape
    B, T = x.shape[:2]
    d_x, d_len = dev(x, np.float32, offset), dev(lengths, np.int64)
    path = out((B, T), torch.int32, offset)
    score = out((B,), torch.float32, offset)
    size, entry = ((lib.vqhmm_gauss_full_viterbi_workspace_size, lib.vqhmm_gauss_full_viterbi_f32) if full
                   else (lib.vqhmm_gauss_viterbi_workspace_size, lib.vqhmm_gauss_viterbi_f32))
    nb = size(B, T, S, Dm)
    ws = guarded(nb, torch.uint8)  # exactly the queried size, poisoned
    rc = entry(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(par), _ext.ptr(d_x), _ext.ptr(d_len), B, T,
               S, Dm, path.ptr, score.ptr, ws.ptr, nb, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(path, score, ws)
    return path.t.cpu().numpy(), score.t.cpu().numpy()


def raw_filter(full, model, x, lengths, prev=None, offset=False, want=("filt", "last", "loglik"), no_pi=False):
    """The filter entry through ctypes -> dict of numpy arrays (the outputs asked for start as 7)."""
    _ext, lib = _lib()
    log_pi, log_A, mean, par = (dev(a, np.float32, offset) for a in model)
    S, Dm = mean.shape
    B, T = x.shape[:2]
    d_x, d_len = dev(x, np.float32, offset), dev(lengths, np.int64)
    d_prev = dev(prev, np.float32, offset)
    bufs = dict(filt=out((B, T, S), torch.float32, offset) if "filt" in want else None,
                last=out((B, S), torch.float32, offset) if "last" in want else None,
                loglik=out((B,), torch.float32, offset) if "loglik" in want else None)
    entry = lib.vqhmm_gauss_full_filter_f32 if full else lib.vqhmm_gauss_filter_f32
    rc = entry(_ext.ptr(None if no_pi else log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(par), _ext.ptr(d_x),
               _ext.ptr(d_len), _ext.ptr(d_prev), B, T, S, Dm,
               *(None if bufs[k] is None else bufs[k].ptr for k in ("filt", "last", "loglik")), _ext.stream_ptr())
    assert rc == 0, rc
    check_all(*bufs.values())
    return {k: None if v is None else v.t.cpu().numpy() for k, v in bufs.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


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


def check_filter(got, ref, L, tag=""):
    """The contract's bounds against the fp64 restatement, and the rows' sums."""
    B, T, S = ref["filt"].shape
    e_l = np.abs(got["last"] - ref["last"]).max(initial=0)
    e_ll = rel_ok(got["loglik"], ref["loglik"])
    e_f = 0.0
    if got.get("filt") is not None:
        assert not np.isnan(got["filt"]).any()
        e_f = np.abs(got["filt"] - ref["filt"]).max(initial=0)
        rows = got["filt"].astype(np.float64).sum(-1)
        live = ref["filt"].any(-1)
        assert np.abs(rows[live] - 1).max(initial=0) <= 1e-5 and not got["filt"][~live].any()
    print(f"{tag}: filt {e_f:.2e} last {e_l:.2e} loglik {e_ll:.2e}")
    assert e_f <= 1e-5 and e_l <= 1e-5


def make_model(full, rng, S, Dm):
    return GF.random_model(rng, S, Dm) if full else G.random_model(rng, S, Dm)


def make_data(rng, model, B, T, full):
    """Data scattered around the means (every state gets visited)."""
    mean = model[2]
    S, Dm = mean.shape
    z = rng.integers(0, S, (B, T))
    return (mean[z] + rng.standard_normal((B, T, Dm)) * 1.5).astype(np.float32)


# ------------------------------------------------------------------------------ the shape cases
T_SET, B_SET = (1, 2, 7, 8, 63, 64, 65, 130), (1, 5, 70)
DIAG_SD = [(S, Dm) for S in (1, 2, 3, 8, 9, 32) for Dm in (1, 5, 64)]
FULL_SD = [(1, 1), (3, 8), (2, 9), (32, 16), (9, 17), (8, 32)]   # the gf_em_dp widths and the S D D limit
# T and B cycle (B with a slip, so that a T meets another B on its next turn)
CASES = [(False, S, Dm, B_SET[(k + k // 8) % 3], T_SET[k % 8]) for k, (S, Dm) in enumerate(DIAG_SD)]
CASES += [(True, S, Dm, B_SET[(k + 2) % 3], T_SET[(3 * k + 5) % 8]) for k, (S, Dm) in enumerate(FULL_SD)]
CASE_IDS = ["%s-S%d-D%d-B%d-T%d" % (("full" if c[0] else "diag",) + c[1:]) for c in CASES]


@functools.lru_cache(maxsize=None)
def shape_case(full, S, Dm, B, T):
    """Model, data, lengths, the GPU's emission tensor and both references: computed once, shared, never
    modified."""
    rng = np.random.default_rng(1000 * S + Dm + 7 * T + (5000 if full else 0))
    model = make_model(full, rng, S, Dm)
    x = make_data(rng, model, B, T, full)
    L = ragged(S + Dm + T, B, T)
    em = raw_emission(full, model, x, L)
    vit = D.viterbi_em_f32(model[0], model[1], em, L)
    fil = D.filter_em_ref(model[0], model[1], em, L)
    for a in (*model, x, L, em, *vit, *fil.values()):
        a.setflags(write=False)
    return model, x, L, em, vit, fil


@pytest.mark.parametrize("offset", (False, True), ids=("exact", "offset4"))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_viterbi_shapes(case, offset):
    import vqhmm
    full, S, Dm, B, T = case
    model, x, L, em, (rpath, rscore), _ = shape_case(*case)
    path, score = raw_viterbi(full, model, x, L, offset)
    assert np.array_equal(path, rpath)
    assert np.array_equal(bits(score), bits(rscore)), (score, rscore)
    # the time-varying kernel on the expanded tables: the same bits
    p2, s2 = vqhmm.viterbi(dev(model[0]), dev(D.expand_log_A(model[1], B, T)), dev(em), dev(L, np.int64))
    assert np.array_equal(path, p2.cpu().numpy())
    assert np.array_equal(bits(score), bits(s2.cpu().numpy()))


@pytest.mark.parametrize("offset", (False, True), ids=("exact", "offset4"))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_filter_shapes(case, offset):
    full, S, Dm, B, T = case
    model, x, L, em, _, ref = shape_case(*case)
    got = raw_filter(full, model, x, L, offset=offset)
    check_filter(got, ref, L, CASE_IDS[CASES.index(case)])
    inside = np.arange(T)[None, :] < L[:, None]
    assert not got["filt"][~inside].any() and got["filt"][inside].any(-1).all()
    # the streaming form: the same bits without filt; last alone
    lean = raw_filter(full, model, x, L, offset=offset, want=("last", "loglik"))
    assert np.array_equal(bits(lean["last"]), bits(got["last"]))
    assert np.array_equal(bits(lean["loglik"]), bits(got["loglik"]))
    only = raw_filter(full, model, x, L, offset=offset, want=("last",))
    assert np.array_equal(bits(only["last"]), bits(got["last"]))
    # with prev, log_pi may be NULL
    prev = np.random.default_rng(S + T).random((B, S)).astype(np.float32) * 2 + 0.01
    carried = raw_filter(full, model, x, L, prev=prev, offset=offset, no_pi=True)
    check_filter(carried, D.filter_em_ref(None, model[1], em, L, prev=prev), L, "with prev")
    assert np.array_equal(carried["last"][L == 0], prev[L == 0])


# ------------------------------------------------------------------------------ streaming
def _hmm(full, model):
    """A GaussianHMM holding `model` -> (module on the device, the model tuple its kernels are fed)."""
    import vqhmm
    S, Dm = model[2].shape
    hmm = vqhmm.GaussianHMM(S, Dm, covariance_type="full" if full else "diag")
    last = ("scale_tril", GF.scale_tril_of(model[3]).astype(np.float32)) if full else ("log_var", model[3])
    hmm.load_state_dict({"log_pi": torch.tensor(model[0]), "log_A": torch.tensor(model[1]),
                         "mean": torch.tensor(model[2]), last[0]: torch.tensor(last[1])})
    hmm = hmm.cuda()
    return hmm, tuple(p.cpu().numpy() for p in hmm._params())


@functools.lru_cache(maxsize=None)
def stream_case(full):
    S, Dm, B, T = (3, 8, 5, 130) if full else (8, 5, 5, 130)
    rng = np.random.default_rng(42 + full)
    hmm, model = _hmm(full, make_model(full, rng, S, Dm))
    x = make_data(rng, model, B, T, full)
    L = np.array([T, 0, 1, 64, 100], np.int64)  # ragged, on both sides of every split
    whole = raw_filter(full, model, x, L)
    return hmm, model, x, L, whole


@pytest.mark.parametrize("split", (1, 64, 77))
@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_filter_chunk_carry(full, split):
    _, model, x, L, whole = stream_case(full)
    L1, L2 = np.minimum(L, split), np.maximum(L - split, 0)
    a = raw_filter(full, model, x[:, :split], L1)
    b = raw_filter(full, model, x[:, split:], L2, prev=a["last"], no_pi=True)
    filt = np.concatenate([a["filt"], b["filt"]], 1)
    assert np.abs(filt - whole["filt"]).max() <= 2e-5
    assert np.abs(b["last"] - whole["last"]).max() <= 2e-5
    tot = np.nansum(np.stack([a["loglik"], b["loglik"]]).astype(np.float64), 0)
    live = L > 0
    rel_ok(tot[live], whole["loglik"][live], 2e-5)
    assert np.isnan(a["loglik"][1]) and np.isnan(b["loglik"][1]) and not b["last"][1].any()
    # and against the fp64 restatement fed the same carry
    em2 = raw_emission(full, model, x[:, split:], L2)
    check_filter(b, D.filter_em_ref(None, model[1], em2, L2, prev=a["last"]), L2, "second chunk")


@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_filter_agrees_with_the_estep(full):
    hmm, model, x, L, whole = stream_case(full)
    d_x, d_len = dev(x), dev(L, np.int64)
    rel_ok(whole["loglik"], hmm.log_prob(d_x, d_len).cpu().numpy(), 2e-5)
    gamma = hmm.posterior(d_x, d_len).cpu().numpy()
    for b in np.nonzero(L > 0)[0]:
        assert np.abs(whole["last"][b] - gamma[b, L[b] - 1]).max() <= 2e-5


def test_grid_striding():
    """More sequences than the grid has waves: B = 2100 > 2048."""
    rng = np.random.default_rng(77)
    B, T, S, Dm = 2100, 3, 2, 1
    model = G.random_model(rng, S, Dm)
    x = make_data(rng, model, B, T, False)
    L = rng.integers(0, T + 1, B).astype(np.int64)
    em = raw_emission(False, model, x, L)
    rpath, rscore = D.viterbi_em_f32(model[0], model[1], em, L)
    path, score = raw_viterbi(False, model, x, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    check_filter(raw_filter(False, model, x, L), D.filter_em_ref(model[0], model[1], em, L), L, "striding")


# ------------------------------------------------------------------------------ ties and structure
@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_identical_states_keep_the_lowest_index(full):
    rng = np.random.default_rng(5)
    S, Dm, B, T = 4, 3, 5, 65
    log_pi, log_A, mean, par = (a.copy() for a in make_model(full, rng, S, Dm))
    for a in (log_pi, mean, par):
        a[1], a[3] = a[0], a[2]
    log_A[1], log_A[3] = log_A[0], log_A[2]
    log_A[:, 1], log_A[:, 3] = log_A[:, 0], log_A[:, 2]
    model = (log_pi, log_A, mean, par)
    x = make_data(rng, model, B, T, full)
    L = ragged(6, B, T)
    em = raw_emission(full, model, x, L)
    assert np.array_equal(bits(em[..., 1]), bits(em[..., 0])) and np.array_equal(bits(em[..., 3]), bits(em[..., 2]))
    rpath, rscore = D.viterbi_em_f32(log_pi, log_A, em, L)
    path, score = raw_viterbi(full, model, x, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    inside = np.arange(T)[None, :] < L[:, None]
    assert np.isin(path[inside], (0, 2)).all() and (path[~inside] == -1).all()
    got = raw_filter(full, model, x, L)
    assert np.array_equal(bits(got["filt"][..., 1]), bits(got["filt"][..., 0]))


def test_left_to_right_and_impossible():
    """A left-to-right chain (-inf below the diagonal), and a model whose only start state has no way out: the
    sequences longer than 1 are impossible, their neighbours' bits do not change."""
    rng = np.random.default_rng(720)
    S, Dm, B, T = 4, 3, 6, 70
    log_pi, log_A, mean, log_var = (a.copy() for a in G.random_model(rng, S, Dm))
    x = make_data(rng, (log_pi, log_A, mean, log_var), B, T, False)
    ltr = log_A.copy()
    ltr[np.tril_indices(S, -1)] = NINF
    L = np.array([T, 50, 69, 0, 1, 30], np.int64)
    model = (log_pi, ltr, mean, log_var)
    em = raw_emission(False, model, x, L)
    rpath, rscore = D.viterbi_em_f32(log_pi, ltr, em, L)
    path, score = raw_viterbi(False, model, x, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    assert (np.diff(path[0]) >= 0).all() and np.isfinite(score[L > 0]).all()
    check_filter(raw_filter(False, model, x, L), D.filter_em_ref(log_pi, ltr, em, L), L, "left to right")
    # impossible: from state 0 nothing follows
    pi0 = np.array([0.0, NINF, NINF, NINF], np.float32)
    dead = log_A.copy()
    dead[0, :] = NINF
    model = (pi0, dead, mean, log_var)
    L = np.array([1, T, 1, 40, 0, 1], np.int64)
    em = raw_emission(False, model, x, L)
    rpath, rscore = D.viterbi_em_f32(pi0, dead, em, L)
    assert rscore[1] == NINF and rscore[3] == NINF and np.isfinite(rscore[[0, 2, 5]]).all()
    path, score = raw_viterbi(False, model, x, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    ref = D.filter_em_ref(pi0, dead, em, L)
    got = raw_filter(False, model, x, L)
    check_filter(got, ref, L, "impossible")
    ll = got["loglik"]
    assert ll[1] == NINF and ll[3] == NINF and np.isnan(ll[4]) and np.isfinite(ll[[0, 2, 5]]).all()
    for b in (1, 3):  # the first position is filtered, the rows from the failing step on are zero
        assert got["filt"][b, 0].any() and not got["filt"][b, 1:].any() and not got["last"][b].any()
    keep = [0, 2, 5]
    alone_v = raw_viterbi(False, model, x[keep], L[keep])
    assert np.array_equal(path[keep], alone_v[0]) and np.array_equal(bits(score[keep]), bits(alone_v[1]))
    alone = raw_filter(False, model, x[keep], L[keep])
    for k in ("filt", "last", "loglik"):
        assert np.array_equal(bits(got[k][keep]), bits(alone[k])), k


# ------------------------------------------------------------------------------ hard inputs
HARD = dict(B=6, T=70, S=4, Dm=3)


def hard_case(seed, full=False):
    rng = np.random.default_rng(seed)
    model = make_model(full, rng, HARD["S"], HARD["Dm"])
    return model, make_data(rng, model, HARD["B"], HARD["T"], full)


def check_both(full, model, x, L, prev=None, tag=""):
    em = raw_emission(full, model, x, L)
    rpath, rscore = D.viterbi_em_f32(model[0], model[1], em, L)
    path, score = raw_viterbi(full, model, x, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    ref = D.filter_em_ref(model[0], model[1], em, L, prev=prev)
    got = raw_filter(full, model, x, L, prev=prev)
    check_filter(got, ref, L, tag)
    return em, ref, got, (path, score)


@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_hard_far_observations(full):
    """An observation 60 sigma from every mean at t = T // 3 and at t = 0: the step runs on exp(em - max em)."""
    model, x = hard_case(700, full)
    L = np.array([70, 70, 30, 70, 1, 24])
    far = np.abs(model[2]).max() + 60.0 * 2.0
    x[0, 70 // 3] = far
    x[1, 0] = -far
    x[2, 70 // 3] = far
    x[3, 0] = far
    x[3, 70 // 3] = -far
    x[4, 0] = far
    em, ref, _, _ = check_both(full, model, x, L, tag="far")
    assert em[0, 70 // 3].max() < -1000.0 and em[1, 0].max() < -1000.0
    assert np.isfinite(ref["loglik"]).all()


@pytest.mark.parametrize("with_prev", (False, True), ids=("pi", "prev"))
def test_hard_step_mass_leaves_the_fast_range(with_prev):
    """Well separated states, and transitions of probability ~1e-12 into the state the data then jumps to: the
    step's linear mass is ~1e-12 < 2^-30 (asserted on the reference's own masses), so the max-shifted step
    runs."""
    rng = np.random.default_rng(740)
    S, Dm, B, T = HARD["S"], HARD["Dm"], HARD["B"], HARD["T"]
    mean = (np.arange(S)[:, None] * 12.0 + np.zeros((1, Dm))).astype(np.float32)
    log_var = np.zeros((S, Dm), np.float32)
    A = np.full((S, S), 1.0 / (S - 1))
    A[:, 3] = 1e-12
    A[3, :] = 0.25
    log_pi = np.log(np.full(S, 1.0 / S)).astype(np.float32)
    model = (log_pi, np.log(A).astype(np.float32), mean, log_var)
    z = rng.integers(0, 3, (B, T))
    z[:, 20] = z[:, 64] = z[:, 65] = 3      # the jumps: mid-chunk, a chunk's first steps
    z[0, 0] = z[1, 1] = 3
    x = (mean[z] + rng.standard_normal((B, T, Dm))).astype(np.float32)
    L = np.array([70, 70, 21, 66, 1, 65])
    prev = (rng.random((B, S)).astype(np.float32) + 0.1) if with_prev else None
    if with_prev:
        prev[:, 3] = 0
    em = raw_emission(False, model, x, L)
    ref = D.filter_em_ref(log_pi, model[1], em, L, prev=prev, want_masses=True)
    m = ref["masses"][np.isfinite(ref["masses"])]
    assert (m < 2.0 ** -30).sum() >= 8 and (m > 0).all(), "the case must leave the fast range"
    assert np.isfinite(ref["loglik"]).all()
    check_filter(raw_filter(False, model, x, L, prev=prev), ref, L, "slow step")
    rpath, rscore = D.viterbi_em_f32(log_pi, model[1], em, L)
    path, score = raw_viterbi(False, model, x, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    assert (path[0, [20, 64, 65]] == 3).all()


@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_hard_nan_inside_and_beyond_the_length(full):
    model, x = hard_case(710, full)
    L = np.array([70, 50, 70, 20, 70, 65])
    clean_v, clean_f = raw_viterbi(full, model, x, L), raw_filter(full, model, x, L)
    xn = x.copy()
    xn[1, 60] = np.nan        # beyond the length: never interpreted
    xn[3, 20:, 1] = np.inf
    v, f = raw_viterbi(full, model, xn, L), raw_filter(full, model, xn, L)
    assert np.array_equal(v[0], clean_v[0]) and np.array_equal(bits(v[1]), bits(clean_v[1]))
    for k in ("filt", "last", "loglik"):
        assert np.array_equal(bits(f[k]), bits(clean_f[k])), k
    xn[2, 69, 2] = np.nan     # inside: the last row of the second chunk
    xn[5, 3, 0] = np.inf      # inside: the first chunk
    path, score = raw_viterbi(full, model, xn, L)
    assert (path[[2, 5]] == -1).all() and np.isnan(score[[2, 5]]).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(path[keep], clean_v[0][keep]) and np.array_equal(bits(score[keep]), bits(clean_v[1][keep]))
    got = raw_filter(full, model, xn, L)
    ll = got["loglik"]
    assert np.isnan(ll[[2, 5]]).all() and not got["last"][[2, 5]].any()
    for b, t in ((2, 69), (5, 3)):   # zero from exactly that position on, the rows before it within bound
        assert not got["filt"][b, t:].any() and got["filt"][b, :t].any(-1).all()
        assert np.abs(got["filt"][b, :t] - clean_f["filt"][b, :t]).max() <= 2e-5
    em = raw_emission(full, model, xn, L)
    assert not np.isfinite(em[2, 69]).all() and not np.isfinite(em[5, 3]).all()
    check_filter(got, D.filter_em_ref(model[0], model[1], em, L), L, "nan")
    for k in ("filt", "last", "loglik"):
        assert np.array_equal(bits(got[k][keep]), bits(clean_f[k][keep])), k


def test_hard_length_one_and_dead_carry():
    model, x = hard_case(730)
    check_both(False, model, x, np.ones(6, np.int64), tag="L=1")
    L = np.array([70, 3, 1, 0, 65, 64])
    prev = np.random.default_rng(731).random((6, 4)).astype(np.float32)
    prev[0] = 0                      # sum(prev) = 0: impossible from the start
    prev[2, 1] = np.inf              # a sum that is not finite
    _, ref, got, _ = check_both(False, model, x, L, prev=prev, tag="dead carry")
    for b in (0, 2):
        assert got["loglik"][b] == NINF and not got["filt"][b].any() and not got["last"][b].any()
    assert np.array_equal(got["last"][3], prev[3]) and np.isnan(got["loglik"][3])
    assert np.isfinite(got["loglik"][[1, 4, 5]]).all()


# ------------------------------------------------------------------------------ determinism, independence
@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_deterministic_and_independent_of_the_batch(full):
    case = next(c for c in CASES if c[0] == full and c[3] == 70 and c[4] >= 63)
    model, x, L, _, _, _ = shape_case(*case)
    a, b = raw_viterbi(full, model, x, L), raw_viterbi(full, model, x, L)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    fa, fb = raw_filter(full, model, x, L), raw_filter(full, model, x, L)
    for k in ("filt", "last", "loglik"):
        assert np.array_equal(bits(fa[k]), bits(fb[k])), k
    for s in (0, int(np.argmax(L[4:])) + 4):   # a full-length sequence and the longest ragged one, alone
        v1 = raw_viterbi(full, model, x[s:s + 1], L[s:s + 1])
        assert np.array_equal(v1[0][0], a[0][s]) and np.array_equal(bits(v1[1][0]), bits(a[1][s]))
        f1 = raw_filter(full, model, x[s:s + 1], L[s:s + 1])
        for k in ("filt", "last", "loglik"):
            assert np.array_equal(bits(f1[k][0]), bits(fa[k][s])), k


@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_empty_shapes(full):
    _ext, lib = _lib()
    S, Dm, B = 3, 2, 3
    model = [dev(a) for a in make_model(full, np.random.default_rng(1), S, Dm)]
    P, sp = _ext.ptr, _ext.stream_ptr
    vit = lib.vqhmm_gauss_full_viterbi_f32 if full else lib.vqhmm_gauss_viterbi_f32
    fil = lib.vqhmm_gauss_full_filter_f32 if full else lib.vqhmm_gauss_filter_f32
    lens = torch.zeros((B,), dtype=torch.int64, device="cuda")
    g_out = [out((B,), torch.float32), out((B,), torch.float32), out((B, S), torch.float32), out((B, 5), torch.int32)]
    score, ll, last, path = (g.t for g in g_out)
    prev = torch.rand((B, S), device="cuda")
    # (B, T) = (3, 0): every length is 0, the size-B outputs are written, no pointer but theirs is needed
    assert vit(None, None, None, None, None, None, B, 0, S, Dm, None, P(score), None, 0, sp()) == 0
    assert fil(None, None, None, None, None, None, None, B, 0, S, Dm, None, P(last), P(ll), sp()) == 0
    torch.cuda.synchronize()
    assert (score == NINF).all() and torch.isnan(ll).all() and not last.any()
    assert fil(None, None, None, None, None, None, P(prev), B, 0, S, Dm, None, P(last), P(ll), sp()) == 0
    torch.cuda.synchronize()
    assert torch.equal(last, prev)
    # (0, 5)
    assert vit(*(P(m) for m in model), None, P(lens), 0, 5, S, Dm, None, None, None, 0, sp()) == 0
    assert fil(*(P(m) for m in model), None, P(lens), None, 0, 5, S, Dm, None, None, None, sp()) == 0
    # T > 0 and every length 0
    x = torch.zeros((B, 5, Dm), device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    assert vit(*(P(m) for m in model), P(x), P(lens), B, 5, S, Dm, P(path), P(score), P(ws), 4096, sp()) == 0
    torch.cuda.synchronize()
    assert (path == -1).all() and (score == NINF).all()
    check_all(*g_out)


# ------------------------------------------------------------------------------ GaussianHMM
@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_python_decode_filter_update(full):
    hmm, model, x, L, whole = stream_case(full)
    B, T = x.shape[:2]
    S = model[2].shape[0]
    d_x = dev(x)
    em = hmm.emission_log_prob(d_x, L).cpu().numpy()
    path, score = hmm.decode(d_x.double(), torch.tensor(L))
    rpath, rscore = D.viterbi_em_f32(model[0], model[1], em, L)
    assert path.dtype == torch.int32 and score.dtype == torch.float32 and path.shape == (B, T)
    assert np.array_equal(path.cpu().numpy(), rpath) and np.array_equal(bits(score.cpu().numpy()), bits(rscore))
    p2, _ = hmm.decode(d_x)       # lengths default to T
    assert (p2 >= 0).all()
    filt, ll, st = hmm.filter(d_x, L, return_state=True)
    assert np.array_equal(bits(filt.cpu().numpy()), bits(whole["filt"]))
    assert np.array_equal(bits(ll.cpu().numpy()), bits(whole["loglik"]))
    assert np.array_equal(bits(st.cpu().numpy()), bits(whole["last"]))
    assert len(hmm.filter(d_x, L)) == 2
    # a feed in chunks of 16 through update() ends in the same state and the same total log-likelihood
    state, tot = None, torch.zeros(B, dtype=torch.float64, device="cuda")
    for t0 in range(0, T, 16):
        n = min(16, T - t0)
        state, l = hmm.update(d_x[:, t0:t0 + n], np.clip(L - t0, 0, n), state=state)
        tot += torch.nan_to_num(l.double(), nan=0.0)
    assert np.abs(state.cpu().numpy() - whole["last"]).max() <= 2e-5
    live = L > 0
    rel_ok(tot.cpu().numpy()[live], whole["loglik"][live], 2e-5)
    s2, l2 = hmm.update(d_x, L)   # update == filter without filt
    assert torch.equal(s2.view(torch.int32), st.view(torch.int32))
    assert torch.equal(l2.view(torch.int32), ll.view(torch.int32))
    with pytest.raises(ValueError):
        hmm.filter(d_x, L, state=torch.zeros((B, S + 1), device="cuda"))
    with pytest.raises(ValueError):
        hmm.update(d_x, L, state=torch.zeros((B, S), dtype=torch.float64, device="cuda"))


def _predict_next_ref(hmm, state):
    A = np.exp(hmm.log_A.detach().cpu().numpy().astype(np.float64))
    mu = hmm.mean.detach().cpu().numpy().astype(np.float64)
    if hmm.full:
        Lt = np.tril(hmm.scale_tril.detach().cpu().numpy().astype(np.float64))
        sigma = Lt @ Lt.transpose(0, 2, 1)
    else:
        sigma = np.stack([np.diag(v) for v in np.exp(hmm.log_var.detach().cpu().numpy().astype(np.float64))])
    nxt = state.astype(np.float64) @ A
    probs = nxt / nxt.sum(-1, keepdims=True)
    mean = probs @ mu
    second = sigma + mu[:, :, None] * mu[:, None, :]
    cov = np.einsum("bs,sij->bij", probs, second) - mean[:, :, None] * mean[:, None, :]
    return probs, mean, cov


@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_python_predict_next(full):
    hmm, model, x, L, whole = stream_case(full)
    state = whole["last"][L > 0]
    got = hmm.predict_next(torch.from_numpy(state).cuda())
    ref = _predict_next_ref(hmm, state)
    S, Dm = model[2].shape
    for g, r, shape in zip(got, ref, ((len(state), S), (len(state), Dm), (len(state), Dm, Dm))):
        g = g.cpu().numpy()
        assert g.shape == shape and g.dtype == np.float32
        assert np.abs(g - r).max() <= 1e-6 * np.abs(r).max()
    assert np.abs(got[0].double().sum(-1).cpu().numpy() - 1).max() <= 1e-6


@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_python_after_a_mixture_fit_and_planted_decode(full):
    """Three well separated sticky regimes (means -5, 0, 5 in D = 2, unit covariances): the reference Viterbi
    recovers the planted states on >= 99 % of the positions (checked first, on the CPU), so decode must clear
    95 %; then every method runs on a model fitted as a mixture."""
    import vqhmm
    rng = np.random.default_rng(9)
    S, Dm, B, T = 3, 2, 16, 80
    A = np.full((S, S), 0.05) + np.eye(S) * 0.85
    log_pi, log_A = np.log(np.full(S, 1 / S)).astype(np.float32), np.log(A).astype(np.float32)
    mean = np.repeat(np.array([-5.0, 0.0, 5.0], np.float32)[:, None], Dm, 1)
    eye = np.repeat(np.eye(Dm)[None], S, 0)
    x, z = GF.sample_data(rng, log_pi, log_A, mean, eye, B, T)
    par = eye.astype(np.float32) if full else np.zeros((S, Dm), np.float32)
    hmm, model = _hmm(full, (log_pi, log_A, mean, par))
    em_ref = (GF.emission_ref(mean, par, x) if full else G.emission_ref(mean, par, x))[0]
    rpath, _ = D.viterbi_em_f32(log_pi, log_A, em_ref.astype(np.float32))
    assert (rpath == z).mean() >= 0.99
    d_x = dev(x)
    path, _ = hmm.decode(d_x)
    assert (path.cpu().numpy() == z).mean() >= 0.95
    # after fit(mixture=True)
    fitted = vqhmm.GaussianHMM(S, Dm, covariance_type="full" if full else "diag",
                               generator=torch.Generator().manual_seed(3)).cuda()
    fitted.fit(d_x, n_iter=5, mixture=True, generator=torch.Generator(device="cuda").manual_seed(4))
    params = tuple(p.cpu().numpy() for p in fitted._params())
    em = fitted.emission_log_prob(d_x).cpu().numpy()
    path, score = fitted.decode(d_x)
    rpath, rscore = D.viterbi_em_f32(params[0], params[1], em)
    assert np.array_equal(path.cpu().numpy(), rpath) and np.array_equal(bits(score.cpu().numpy()), bits(rscore))
    filt, ll, st = fitted.filter(d_x, return_state=True)
    got = dict(filt=filt.cpu().numpy(), last=st.cpu().numpy(), loglik=ll.cpu().numpy())
    check_filter(got, D.filter_em_ref(params[0], params[1], em), np.full(B, T), "mixture")
    s2, _ = fitted.update(d_x)
    assert torch.equal(s2.view(torch.int32), st.view(torch.int32))
    probs, m, cov = fitted.predict_next(st)
    ref = _predict_next_ref(fitted, got["last"])
    for g, r in zip((probs, m, cov), ref):
        assert np.abs(g.cpu().numpy() - r).max() <= 1e-6 * np.abs(r).max()


@pytest.mark.parametrize("full", (False, True), ids=("diag", "full"))
def test_python_routes_allocate_no_per_position_table(full):
    """update allocates nothing of size B T S, decode only the path and the backpointer bytes (B T SP): the peak
    of the allocator over each call stays far below one (B,T,S) fp32 table."""
    S, Dm, B, T = 32, 4, 64, 512
    hmm, _ = _hmm(full, make_model(full, np.random.default_rng(3), S, Dm))
    x = torch.randn((B, T, Dm), device="cuda")
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    table = B * T * S * 4
    hmm.update(x, L), hmm.decode(x, L)      # the library and the allocator are warm
    for call, allowed in ((lambda: hmm.update(x, L), table // 16), (lambda: hmm.decode(x, L), table // 2)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = call()
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base <= allowed
        del res
