"""GPU checks of CodeHMM's fused Viterbi decode and causal filter (vqhmm_code_viterbi_f32 /
vqhmm_code_filter_f32, hmm_code_decode.hip) against tests/code_decode_ref.py, fed the same fp32 parameters.

Viterbi is compared bit for bit: with the fp32 restatement of the rule, and with vqhmm.viterbi on the
expanded tables (log_A broadcast to (B,T,S,S), em = log_B[:, codes]).  The filter's bounds are the
contract's (include/vqhmm.h): |filt|, |last| abs 1e-5 and loglik rel 1e-5 of max(1, |loglik|) against the
fp64 restatement; two filtered results compared with each other (a chunked run against the single call,
last against the E-step's smoothed gamma) get twice the per-result bound, 2e-5.
"""
import functools

import numpy as np
import pytest
import torch

import code_decode_ref as D
import code_hmm_ref as R
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
NINF = -np.inf


def ragged(seed, B, T):
    """Lengths with T, 0, 1 and 2 first (as far as B and T allow), then random ones."""
    rng = np.random.default_rng(seed)
    L = np.concatenate([[T, 0, 1, 2], rng.integers(0, T + 1, max(B - 4, 0))])[:B]
    return np.minimum(L, T).astype(np.int64)


def dev(a, dtype, offset=False):
    """`a` on the device in an exact-size buffer, or (offset) at a pointer 4 bytes past a 16-byte boundary."""
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


def raw_viterbi(model, codes, lengths, offset=False):
    """vqhmm_code_viterbi_f32 through ctypes; path and score start as 7 (the call must write every element)."""
    from vqhmm import _ext
    lib = _ext.load()
    log_pi, log_A, log_B = (dev(a, np.float32, offset) for a in model)
    S, V = log_B.shape
    B, T = codes.shape
    d_codes = dev(codes, np.int32, offset)
    d_len = dev(lengths, np.int64)
    path = out((B, T), torch.int32, offset)
    score = out((B,), torch.float32, offset)
    nb = lib.vqhmm_code_viterbi_workspace_size(B, T, S, V)
    ws = guarded(nb, torch.uint8)  # exactly the queried size, poisoned
    rc = lib.vqhmm_code_viterbi_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(log_B), _ext.ptr(d_codes),
                                    _ext.ptr(d_len), B, T, S, V, path.ptr, score.ptr, ws.ptr, nb,
                                    _ext.stream_ptr())
    assert rc == 0, rc
    check_all(path, score, ws)
    return path.t.cpu().numpy(), score.t.cpu().numpy()


def raw_filter(model, codes, lengths, prev=None, offset=False, want_filt=True, no_pi=False):
    """vqhmm_code_filter_f32 through ctypes -> dict of numpy arrays (outputs start as 7)."""
    from vqhmm import _ext
    lib = _ext.load()
    log_pi, log_A, log_B = (dev(a, np.float32, offset) for a in model)
    S, V = log_B.shape
    B, T = codes.shape
    d_codes = dev(codes, np.int32, offset)
    d_len = dev(lengths, np.int64)
    d_prev = None if prev is None else dev(prev, np.float32, offset)
    filt = out((B, T, S), torch.float32, offset) if want_filt else None
    last = out((B, S), torch.float32, offset)
    ll = out((B,), torch.float32, offset)
    nb = lib.vqhmm_code_filter_workspace_size(B, T, S, V)
    ws = guarded(nb, torch.uint8)  # exactly the queried size, poisoned
    rc = lib.vqhmm_code_filter_f32(_ext.ptr(None if no_pi else log_pi), _ext.ptr(log_A), _ext.ptr(log_B),
                                   _ext.ptr(d_codes), _ext.ptr(d_len), _ext.ptr(d_prev), B, T, S, V,
                                   None if filt is None else filt.ptr, last.ptr, ll.ptr, ws.ptr, nb, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(filt, last, ll, ws)
    return dict(filt=None if filt is None else filt.t.cpu().numpy(), last=last.t.cpu().numpy(),
                loglik=ll.t.cpu().numpy())


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


# ------------------------------------------------------------------------------ the shape cases
S_SET, V_SET = (1, 2, 3, 8, 9, 32), (1, 5, 300)
T_SET, B_SET = (1, 2, 63, 64, 65, 130), (1, 5, 70)
# every (S, V) pair; T and B cycle so that each T meets three S and every B.  Then the L2 tier (the table
# past 64 KB) at the narrowest and at the widest lane width.
CASES = [(S, V, B_SET[(k + k // 6) % 3], T_SET[k % 6])
         for k, (S, V) in enumerate((S, V) for S in S_SET for V in V_SET)]
CASES += [(2, 65536, 5, 130), (32, 600, 5, 65)]
CASE_IDS = ["S%d-V%d-B%d-T%d" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def shape_case(S, V, B, T):
    """Model, codes, lengths and both references of a case: computed once, shared, never modified."""
    rng = np.random.default_rng(1000 * S + V + 7 * T)
    model = R.random_model(rng, S, V, 1.5)
    codes = rng.integers(0, V, size=(B, T)).astype(np.int32)
    L = ragged(S + V + T, B, T)
    for b in range(B):
        codes[b, int(L[b]):] = -1  # padding: never interpreted
    vit = D.viterbi_f32(*model, codes, L)
    fil = D.filter_ref(*model, codes, L)
    for a in (*model, codes, L, *vit, *fil.values()):
        a.setflags(write=False)
    return model, codes, L, vit, fil


@pytest.mark.parametrize("offset", (False, True), ids=("exact", "offset4"))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_viterbi_shapes(case, offset):
    import vqhmm
    model, codes, L, (rpath, rscore), _ = shape_case(*case)
    path, score = raw_viterbi(model, codes, L, offset)
    assert np.array_equal(path, rpath)
    assert np.array_equal(bits(score), bits(rscore)), (score, rscore)
    # the time-varying kernel on the expanded tables: the same bits
    log_A, em = D.expand_tables(model[1], model[2], codes)
    p2, s2 = vqhmm.viterbi(dev(model[0], np.float32), dev(log_A, np.float32), dev(em, np.float32), dev(L, np.int64))
    assert np.array_equal(path, p2.cpu().numpy())
    assert np.array_equal(bits(score), bits(s2.cpu().numpy()))


@pytest.mark.parametrize("offset", (False, True), ids=("exact", "offset4"))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_filter_shapes(case, offset):
    import vqhmm
    S, V, B, T = case
    model, codes, L, _, ref = shape_case(*case)
    got = raw_filter(model, codes, L, offset=offset)
    e_f = np.abs(got["filt"] - ref["filt"]).max(initial=0)
    e_l = np.abs(got["last"] - ref["last"]).max(initial=0)
    e_ll = rel_ok(got["loglik"], ref["loglik"])
    print(f"S={S} V={V} B={B} T={T}: filt {e_f:.2e} last {e_l:.2e} loglik {e_ll:.2e}")
    assert not np.isnan(got["filt"]).any() and e_f <= 1e-5 and e_l <= 1e-5
    rows = got["filt"].astype(np.float64).sum(-1)
    inside = np.arange(T)[None, :] < L[:, None]
    assert np.abs(rows[inside] - 1).max(initial=0) <= 1e-5 and not got["filt"][~inside].any()
    # the streaming form: the same bits without filt
    lean = raw_filter(model, codes, L, offset=offset, want_filt=False)
    assert np.array_equal(bits(lean["last"]), bits(got["last"]))
    assert np.array_equal(bits(lean["loglik"]), bits(got["loglik"]))
    if offset:
        return
    # against the E-step: its loglik, and its smoothed gamma at the last position
    hmm = _codehmm(S, V, model)
    d_codes, d_len = dev(codes, np.int32), dev(L, np.int64)
    rel_ok(got["loglik"], hmm.log_prob(d_codes, d_len).cpu().numpy())
    gamma = hmm.posterior(d_codes, d_len).cpu().numpy()
    for b in np.nonzero(L > 0)[0]:
        assert np.abs(got["last"][b] - gamma[b, L[b] - 1]).max() <= 2e-5


# ------------------------------------------------------------------------------ viterbi edge cases
def test_viterbi_ties_keep_the_lowest_index():
    """All-equal log_A and log_B on a grid of 0.5: sums are exact, ties are everywhere, and the restatement's
    lowest-index rule decides every one of them."""
    rng = np.random.default_rng(5)
    S, V, B, T = 9, 5, 5, 65
    log_pi = np.zeros(S, np.float32)
    log_A = np.full((S, S), -1.0, np.float32)
    log_B = (np.round(rng.standard_normal((S, V)) * 2) / 2).astype(np.float32)
    codes = rng.integers(0, V, size=(B, T)).astype(np.int32)
    L = ragged(6, B, T)
    rpath, rscore = D.viterbi_f32(log_pi, log_A, log_B, codes, L)
    path, score = raw_viterbi((log_pi, log_A, log_B), codes, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    # a fully tied model decodes to state 0 throughout
    z = np.zeros((S, V), np.float32)
    path, score = raw_viterbi((log_pi, log_A, z), codes, L)
    inside = np.arange(T)[None, :] < L[:, None]
    assert not path[inside].any() and (path[~inside] == -1).all()


def test_viterbi_structural_zeros_and_impossible():
    rng = np.random.default_rng(700)
    S, V, T = 3, 6, 20
    log_pi, log_A, log_B = R.random_model(rng, S, V)
    log_B[1:, 0] = NINF   # only state 0 emits code 0 ...
    log_A[0, 0] = NINF    # ... and it never follows itself
    log_A[2, 1] = NINF
    model = (log_pi, log_A, log_B)
    codes = rng.integers(1, V, size=(4, T)).astype(np.int32)
    L = np.array([T, 15, 17, T - 1], np.int64)
    codes[0, :] = np.where(np.arange(T) % 2 == 0, 0, codes[0, :])  # possible: code 0 never twice running
    codes[1, 7] = codes[1, 8] = 0                                  # impossible
    rpath, rscore = D.viterbi_f32(*model, codes, L)
    assert rscore[1] == NINF and np.isfinite(rscore[[0, 2, 3]]).all()
    path, score = raw_viterbi(model, codes, L)
    assert np.array_equal(path, rpath) and np.array_equal(bits(score), bits(rscore))
    assert (path[0, ::2] == 0).all()


@pytest.mark.parametrize("badval", (-1, 6, 1 << 30))
def test_viterbi_bad_codes(badval):
    rng = np.random.default_rng(710)
    S, V, T = 5, 6, 70
    model = R.random_model(rng, S, V)
    codes = rng.integers(0, V, size=(4, T)).astype(np.int32)
    L = np.array([T, 66, 40, T], np.int64)
    good = raw_viterbi(model, codes, L)
    bad = codes.copy()
    bad[1, 65] = badval   # inside the length (second chunk)
    bad[2, 40:] = badval  # past the length: never interpreted
    path, score = raw_viterbi(model, bad, L)
    assert (path[1] == -1).all() and np.isnan(score[1])
    keep = [0, 2, 3]
    assert np.array_equal(path[keep], good[0][keep]) and np.array_equal(bits(score[keep]), bits(good[1][keep]))
    assert (path[2, 40:] == -1).all()


# ------------------------------------------------------------------------------ filter edge cases
@pytest.mark.parametrize("split", (1, 64, 65))
def test_filter_chunk_carry(split):
    S, V, B, T = 8, 300, 5, 130
    rng = np.random.default_rng(42)
    model = R.random_model(rng, S, V, 1.5)
    codes = rng.integers(0, V, size=(B, T)).astype(np.int32)
    L = np.array([T, 0, 1, 64, 100], np.int64)  # ragged, on both sides of every split
    whole = raw_filter(model, codes, L)
    L1, L2 = np.minimum(L, split), np.maximum(L - split, 0)
    a = raw_filter(model, np.ascontiguousarray(codes[:, :split]), L1)
    b = raw_filter(model, np.ascontiguousarray(codes[:, split:]), L2, prev=a["last"], no_pi=True)
    filt = np.concatenate([a["filt"], b["filt"]], 1)
    assert np.abs(filt - whole["filt"]).max() <= 2e-5
    assert np.abs(b["last"] - whole["last"]).max() <= 2e-5
    tot = np.nansum(np.stack([a["loglik"], b["loglik"]]).astype(np.float64), 0)
    live = L > 0
    rel_ok(tot[live], whole["loglik"][live])
    assert np.isnan(a["loglik"][1]) and np.isnan(b["loglik"][1]) and not b["last"][1].any()
    # and against the fp64 restatement fed the same carry
    ref = D.filter_ref(*model, codes[:, split:], L2, prev=a["last"])
    assert np.abs(b["filt"] - ref["filt"]).max() <= 1e-5 and np.abs(b["last"] - ref["last"]).max() <= 1e-5
    rel_ok(b["loglik"], ref["loglik"])


def test_filter_fallback_steps():
    """Tables scaled x8: step masses leave [2^-30, 2^30] (checked on the reference), so the max-shifted step
    runs, in the LDS tier and with a carried state."""
    rng = np.random.default_rng(81)
    S, V, B, T = 8, 300, 5, 130
    model = R.random_model(rng, S, V, 8.0)
    codes = rng.integers(0, V, size=(B, T)).astype(np.int32)
    L = ragged(82, B, T)
    prev = rng.random((B, S)).astype(np.float32) * 3
    for pv in (None, prev):
        ref = D.filter_ref(*model, codes, L, prev=pv, want_masses=True)
        m = ref["masses"][:, (1 if pv is None else 0):]
        m = m[np.isfinite(m)]
        assert (m < 2.0 ** -30).sum() >= 10, "the case must leave the fast range"
        assert np.isfinite(ref["loglik"][L > 0]).all()
        got = raw_filter(model, codes, L, prev=pv)
        e_f, e_l = np.abs(got["filt"] - ref["filt"]).max(), np.abs(got["last"] - ref["last"]).max()
        print(f"fallback prev={pv is not None}: filt {e_f:.2e} last {e_l:.2e}")
        assert e_f <= 1e-5 and e_l <= 1e-5
        rel_ok(got["loglik"], ref["loglik"])


@pytest.mark.parametrize("with_prev", (False, True))
def test_filter_degenerate_sequences(with_prev):
    """An impossible sequence, a code out of range and a length of 0 in one batch: the contract's values, the
    rows before the failing position intact, the neighbours' bits unchanged."""
    rng = np.random.default_rng(700)
    S, V, T = 3, 6, 70
    log_pi, log_A, log_B = R.random_model(rng, S, V)
    log_B[1:, 0] = NINF   # only state 0 emits code 0 ...
    log_A[0, 0] = NINF    # ... and it never follows itself
    model = (log_pi, log_A, log_B)
    codes = rng.integers(1, V, size=(6, T)).astype(np.int32)
    L = np.array([T, 50, 69, 0, T - 1, 30], np.int64)
    codes[1, 7] = codes[1, 8] = 0   # impossible at t = 8
    codes[2, 66] = V                # out of range in the second chunk
    codes[5, 30:] = -1              # past the length
    prev = None
    if with_prev:
        prev = rng.random((6, S)).astype(np.float32) + 0.1
        prev[4] = 0                 # a dead carry: impossible from the start
    ref = D.filter_ref(*model, codes, L, prev=prev)
    got = raw_filter(model, codes, L, prev=prev)
    assert np.abs(got["filt"] - ref["filt"]).max() <= 1e-5 and np.abs(got["last"] - ref["last"]).max() <= 1e-5
    rel_ok(got["loglik"], ref["loglik"])
    ll = got["loglik"]
    assert ll[1] == NINF and np.isnan(ll[2]) and np.isnan(ll[3]) and np.isfinite(ll[[0, 5]]).all()
    assert got["filt"][1, :8].any(-1).all() and not got["filt"][1, 8:].any() and not got["last"][1].any()
    assert got["filt"][2, :66].any(-1).all() and not got["filt"][2, 66:].any() and not got["last"][2].any()
    assert not got["filt"][3].any()
    assert np.array_equal(got["last"][3], prev[3] if with_prev else np.zeros(S, np.float32))
    if with_prev:
        assert ll[4] == NINF and not got["filt"][4].any() and not got["last"][4].any()
    # the ordinary sequences alone give the same bits
    keep = [0, 5]
    alone = raw_filter(model, codes[keep], L[keep], prev=None if prev is None else prev[keep])
    for k in ("filt", "last", "loglik"):
        assert np.array_equal(bits(got[k][keep]), bits(alone[k])), k


# ------------------------------------------------------------------------------ determinism, return codes
def test_deterministic():
    assert (32, 300, 5, 130) in CASES
    model, codes, L, _, _ = shape_case(32, 300, 5, 130)
    a, b = raw_viterbi(model, codes, L), raw_viterbi(model, codes, L)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    a, b = raw_filter(model, codes, L), raw_filter(model, codes, L)
    for k in ("filt", "last", "loglik"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_return_codes_and_empty_shapes():
    from vqhmm import _ext
    lib = _ext.load()
    S, V, B = 3, 5, 4
    model = R.random_model(np.random.default_rng(1), S, V)
    d = [torch.from_numpy(a).cuda() for a in model]
    P, sp = _ext.ptr, _ext.stream_ptr
    codes = torch.zeros((B, 6), dtype=torch.int32, device="cuda")
    lens = torch.full((B,), 6, dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    g_out = [out((B,), torch.float32), out((B, 6), torch.int32), out((B, S), torch.float32), out((B,), torch.float32)]
    score, path, last, ll = (g.t for g in g_out)
    prev = torch.rand((B, S), device="cuda")

    def vit(B_=B, T=6, S_=S, V_=V, lp=d[0], w=ws, nb=1 << 16):
        return lib.vqhmm_code_viterbi_f32(P(lp), P(d[1]), P(d[2]), P(codes), P(lens), B_, T, S_, V_, P(path), P(score),
                                          P(w), nb, sp())

    def fil(B_=B, T=6, S_=S, V_=V, lp=d[0], pv=None, w=ws, nb=1 << 16):
        return lib.vqhmm_code_filter_f32(P(lp), P(d[1]), P(d[2]), P(codes), P(lens), P(pv), B_, T, S_, V_, None, P(last),
                                         P(ll), P(w), nb, sp())

    for f in (vit, fil):
        assert f(B_=-1, S_=33) == -1 and f(T=-1, V_=65537) == -1       # a negative size first
        assert f(S_=33) == -4 and f(V_=65537) == -4 and f(S_=0) == -4  # then the limits
        assert f(S_=33, lp=None) == -4
        assert f(B_=0, lp=None, w=None, nb=0) == 0
        assert f(lp=None) == -1 and f(w=None) == -1 and f(nb=16) == -1
    # T = 0 with B > 0: every length is 0, the size-B outputs are written, no pointer but theirs is needed
    assert vit(T=0, lp=None, w=None, nb=0) == 0
    torch.cuda.synchronize()
    assert (score == NINF).all()
    assert fil(T=0, lp=None, w=None, nb=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(ll).all() and not last.any()
    assert fil(T=0, lp=None, pv=prev, w=None, nb=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(last, prev)
    # with prev, log_pi may be NULL
    assert fil(lp=None, pv=prev) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(ll).all()
    check_all(*g_out)


# ------------------------------------------------------------------------------ CodeHMM
def _codehmm(S, V, model):
    import vqhmm
    hmm = vqhmm.CodeHMM(S, V)
    hmm.load_state_dict({k: torch.tensor(v) for k, v in zip(("log_pi", "log_A", "log_B"), model)})
    return hmm.cuda()


def test_codehmm_decode():
    assert (32, 300, 5, 130) in CASES
    model, codes, L, (rpath, rscore), _ = shape_case(32, 300, 5, 130)
    hmm = _codehmm(32, 300, model)
    path, score = hmm.decode(dev(codes, np.int32).long(), torch.tensor(L))
    assert path.dtype == torch.int32 and score.dtype == torch.float32 and path.shape == codes.shape
    assert np.array_equal(path.cpu().numpy(), rpath) and np.array_equal(bits(score.cpu().numpy()), bits(rscore))
    # lengths default to T
    full = np.where(codes < 0, 0, codes)
    p2, s2 = hmm.decode(torch.from_numpy(full).cuda())
    r2 = D.viterbi_f32(*model, full)
    assert np.array_equal(p2.cpu().numpy(), r2[0]) and np.array_equal(bits(s2.cpu().numpy()), bits(r2[1]))


def test_codehmm_filter_update_round_trip():
    S, V, B, T = 9, 5, 5, 65
    rng = np.random.default_rng(90)
    model = R.random_model(rng, S, V, 1.5)
    codes = rng.integers(0, V, size=(B, T)).astype(np.int32)
    L = np.array([T, 0, 1, 40, 64], np.int64)
    hmm = _codehmm(S, V, model)
    d_codes = torch.from_numpy(codes).cuda()
    filt, ll, st = hmm.filter(d_codes, L, return_state=True)
    ref = D.filter_ref(*model, codes, L)
    assert np.abs(filt.cpu().numpy() - ref["filt"]).max() <= 1e-5
    rel_ok(ll.cpu().numpy(), ref["loglik"])
    assert len(hmm.filter(d_codes, L)) == 2
    # a feed in chunks of 16 through update() ends in the same state and the same total log-likelihood
    state, tot = None, torch.zeros(B, dtype=torch.float64, device="cuda")
    for t0 in range(0, T, 16):
        n = min(16, T - t0)
        state, l = hmm.update(d_codes[:, t0:t0 + n], np.clip(L - t0, 0, n), state=state)
        tot += torch.nan_to_num(l.double(), nan=0.0)
    assert np.abs(state.cpu().numpy() - st.cpu().numpy()).max() <= 2e-5
    live = L > 0
    rel_ok(tot.cpu().numpy()[live], ref["loglik"][live])
    # update == filter without filt
    s2, l2 = hmm.update(d_codes, L)
    assert torch.equal(s2.view(torch.int32), st.view(torch.int32)) and torch.equal(l2.view(torch.int32), ll.view(torch.int32))
    with pytest.raises(ValueError):
        hmm.filter(d_codes, L, state=torch.zeros((B, S + 1), device="cuda"))
    with pytest.raises(ValueError):
        hmm.update(d_codes, L, state=torch.zeros((B, S), dtype=torch.float64, device="cuda"))


def test_codehmm_predict_next():
    S, V, B = 9, 300, 5
    rng = np.random.default_rng(91)
    model = R.random_model(rng, S, V, 1.5)
    hmm = _codehmm(S, V, model)
    state = rng.random((B, S)).astype(np.float32)
    state /= state.sum(-1, keepdims=True)
    got = hmm.predict_next(torch.from_numpy(state).cuda()).cpu().numpy()
    A, Bm = np.exp(model[1].astype(np.float64)), np.exp(model[2].astype(np.float64))
    nxt = state.astype(np.float64) @ A
    ref = (nxt / nxt.sum(-1, keepdims=True)) @ Bm
    assert got.shape == (B, V) and got.dtype == np.float32
    # rows of log_B are normalised in fp64 and then rounded to fp32: an entry of magnitude up to ~16 moves its
    # probability by up to 16 x 2^-24 ~ 1e-6 relative, and the fp32 product adds a few 2^-24 more
    assert np.abs(got.astype(np.float64).sum(-1) - 1).max() <= 4e-6
    assert np.abs(got - ref).max() <= 1e-6
