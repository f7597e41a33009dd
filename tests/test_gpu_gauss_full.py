"""GPU checks of the full-covariance Gaussian HMM (vqhmm_gauss_full_emission_f32 / vqhmm_gauss_full_estep_f32 /
vqhmm_gauss_moments_f32, hmm_gauss_full.hip, vqhmm.GaussianHMM(covariance_type="full"), vqhmm.gauss_full_log_prob,
vqhmm.regime_moments / regime_covariance) against the fp64 restatement in tests/gauss_full_ref.py.

Emissions: against fp64 on the same fp32 inputs, |d| <= (3 D + 16) 2^-23 A[b,t,s] with A = 1/2 sum_i (sum_{j<=i}
|W_ij| |x_j - mu_j|)^2 + |sum_i log W_ii| + (D/2) ln 2 pi: nested fp32 sums of at most D terms in any order (each
row's product sum, relative error <= (D + 1) u on sum |W||z|; its square, doubling that; the sum of the squares,
another D u), with slack for the constant.  Derived, not measured.

E-step: against the fp64 reference fed the emission tensor the emission entry wrote, with the diagonal file's
bounds (tests/test_gpu_gauss_hmm.py, whose helpers this file uses): gamma abs 1e-5, loglik rel 1e-5 of max(1,
|ref|), pi_cnt 1e-5 x sequences, trans_cnt 2e-5 x transitions, occ 1e-5 x positions, m1[s,d] 2e-5 x sum |y_d|,
m2[s,i,j] 2e-5 x sum |y_i| |y_j| over the in-length positions (y = x - shift; with weights every position counts
|w_b| times).
"""
import numpy as np
import pytest
import torch

import gauss_full_ref as F
import test_gpu_gauss_hmm as H
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
NINF = -np.inf
COUNTS = ("pi_cnt", "trans_cnt", "occ", "m1", "m2")
SHAPES = ((5, 1, 1, 1), (6, 63, 3, 5), (6, 70, 3, 12), (7, 65, 17, 17), (5, 130, 32, 16), (5, 130, 8, 32))  # B,T,S,D
EINVAL, EUNSUPPORTED = -1, -4
dev_f32, bits_equal, rel_ok, ragged = H.dev_f32, H.bits_equal, H.rel_ok, H.ragged


def make_case(seed, B, T, S, D, lengths=None, centre=0.0):
    """A random model and data scattered around its means with 1.5 x its covariances' spread."""
    rng = np.random.default_rng(seed)
    log_pi, log_A, mean, W = F.random_model(rng, S, D)
    mean = (mean + centre).astype(np.float32)
    Lc = F.scale_tril_of(W)
    z = rng.integers(0, S, (B, T))
    x = (mean[z] + 1.5 * np.einsum("btij,btj->bti", Lc[z], rng.standard_normal((B, T, D)))).astype(np.float32)
    L = ragged(seed + 1, B, T) if lengths is None else np.asarray(lengths, np.int64)
    return (log_pi, log_A, mean, W), x, L


def raw_emission(model, x, lengths, offset=False, fill=7.0):
    from vqhmm import _ext
    lib = _ext.load()
    mean, W = (dev_f32(a, offset) for a in model[2:])
    S, D = mean.shape
    B, T = x.shape[:2]
    d_x = dev_f32(x, offset)
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    em = guarded((B, T, S), torch.float32, fill=fill)
    rc = lib.vqhmm_gauss_full_emission_f32(_ext.ptr(mean), _ext.ptr(W), _ext.ptr(d_x), _ext.ptr(d_len), B, T, S, D,
                                           em.ptr, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(em)
    return em.t


def raw_estep(model, x, lengths, shift=None, weights=None, loglik=True, gamma=True, offset=False):
    """vqhmm_gauss_full_estep_f32 through ctypes on guarded exact-size buffers and a guarded, poisoned workspace of exactly the
    queried size (gpu_buffers.guarded); the counts start as NaN (the call must
    write every element) -> dict of device tensors."""
    from vqhmm import _ext
    lib = _ext.load()
    log_pi, log_A, mean, W = (dev_f32(a, offset) for a in model)
    S, D = mean.shape
    B, T = x.shape[:2]
    d_x = dev_f32(x, offset)
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    d_sh, d_w = dev_f32(shift, offset), dev_f32(weights, offset)
    cnt = {k: guarded(sh, torch.float64, fill=float("nan"))
           for k, sh in zip(COUNTS, ((S,), (S, S), (S,), (S, D), (S, D, D)))}
    ll = guarded((B,), torch.float32, fill=7.0) if loglik else None
    gm = guarded((B, T, S), torch.float32, fill=7.0) if gamma else None
    nb = lib.vqhmm_gauss_full_estep_workspace_size(B, T, S, D)
    ws = guarded(nb, torch.uint8)  # exactly the queried size, poisoned
    rc = lib.vqhmm_gauss_full_estep_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(W),
                                        _ext.ptr(d_x), _ext.ptr(d_len), _ext.ptr(d_sh), _ext.ptr(d_w), B, T, S, D,
                                        *(cnt[k].ptr for k in COUNTS), ll.ptr if loglik else None, gm.ptr if gamma else None,
                                        ws.ptr, nb, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(*cnt.values(), ll, gm, ws)
    return dict({k: g.t for k, g in cnt.items()}, loglik=ll.t if loglik else None, gamma=gm.t if gamma else None)


def raw_moments(x, gamma, lengths, shift=None, weights=None, offset=False):
    """vqhmm_gauss_moments_f32 through ctypes on guarded exact-size, NaN-prefilled buffers and a guarded, poisoned
    workspace of exactly the queried size."""
    from vqhmm import _ext
    lib = _ext.load()
    B, T, D = x.shape
    S = gamma.shape[2]
    d_x, d_g = dev_f32(x, offset), dev_f32(gamma, offset)
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    d_sh, d_w = dev_f32(shift, offset), dev_f32(weights, offset)
    cnt = {k: guarded(sh, torch.float64, fill=float("nan"))
           for k, sh in zip(("occ", "m1", "m2"), ((S,), (S, D), (S, D, D)))}
    nb = lib.vqhmm_gauss_moments_workspace_size(B, T, S, D)
    ws = guarded(nb, torch.uint8)  # exactly the queried size, poisoned
    rc = lib.vqhmm_gauss_moments_f32(_ext.ptr(d_x), _ext.ptr(d_g), _ext.ptr(d_len), _ext.ptr(d_sh), _ext.ptr(d_w),
                                     B, T, S, D, *(cnt[k].ptr for k in ("occ", "m1", "m2")), ws.ptr, nb,
                                     _ext.stream_ptr())
    assert rc == 0, rc
    check_all(*cnt.values(), ws)
    return {k: g.t for k, g in cnt.items()}


def count_bounds(loglik, x, lengths, shift, weights):
    """The per-position contracts summed over the sequences that count (those with a finite loglik) -> dict of
    bounds (m1: (1,D), m2: (1,D,D))."""
    B, T, D = x.shape
    L = np.clip(np.asarray(lengths, np.int64), 0, T)
    w = np.ones(B) if weights is None else np.abs(np.asarray(weights, np.float64))
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    counted = np.isfinite(loglik) & (L > 0)
    s1, s2 = np.zeros(D), np.zeros((D, D))
    for b in np.nonzero(counted)[0]:
        y = np.abs(np.asarray(x[b, :L[b]], np.float64) - sh)
        s1 += w[b] * y.sum(0)
        s2 += w[b] * (y.T @ y)
    return dict(pi_cnt=1e-5 * w[counted].sum(), trans_cnt=2e-5 * (w[counted] * (L[counted] - 1)).sum(),
                occ=1e-5 * (w[counted] * L[counted]).sum(), m1=2e-5 * s1[None], m2=2e-5 * s2[None])


def check_counts(got, ref, x, lengths, shift=None, weights=None, tag="", keys=COUNTS, counted=None):
    bounds = count_bounds(ref["loglik"] if counted is None else counted, x, lengths, shift, weights)
    msg, bad = [], []
    for k in keys:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == np.float64 and not np.isnan(g).any(), k
        err = np.abs(g - ref[k])
        msg.append(f"{k} {err.max():.2e}/{np.max(bounds[k]):.1e}")
        if not (err <= bounds[k]).all():
            bad.append(k)
    print(tag, " ".join(msg))
    assert not bad, (bad, msg)


def check_case(model, x, lengths, shift=None, weights=None, offset=False, tag=""):
    """E-step against the reference fed the emission entry's own tensor -> (ref, got)."""
    S, D = model[2].shape
    B, T = x.shape[:2]
    em = raw_emission(model, x, lengths, offset=offset).cpu().numpy()
    ref = F.estep_ref(*model, x, lengths, shift=shift, weights=weights, em=em)
    got = raw_estep(model, x, lengths, shift=shift, weights=weights, offset=offset)
    e_ll = rel_ok(got["loglik"].cpu().numpy(), ref["loglik"])
    gm = got["gamma"].cpu().numpy()
    e_g = np.abs(gm - ref["gamma"]).max(initial=0)
    print(f"{tag} S={S} D={D} B={B} T={T}: gamma {e_g:.2e} loglik {e_ll:.2e}")
    assert not np.isnan(gm).any() and e_g <= 1e-5
    for b in range(B):
        n = int(min(max(lengths[b], 0), T))
        assert not gm[b, n:].any()
    check_counts(got, ref, x, lengths, shift, weights, tag)
    m2 = got["m2"]
    assert torch.equal(m2.view(torch.int64), m2.transpose(1, 2).contiguous().view(torch.int64))
    return ref, got


# ---------------------------------------------------------------------------- emissions
@pytest.mark.parametrize("fill", (7.0, float("nan")))
@pytest.mark.parametrize("B,T,S,D", SHAPES)
def test_emission_against_fp64(B, T, S, D, fill):
    model, x, L = make_case(100 + T + D, B, T, S, D)
    x[0, T - 1] += 40.0   # a far observation (40 sigma and more): the bound scales with z^2
    got = raw_emission(model, x, L, offset=True, fill=fill).cpu().numpy().astype(np.float64)
    ref, mag = F.emission_ref(model[2], model[3], x, L)
    pad = np.arange(T)[None, :] >= L[:, None]
    assert np.isneginf(got[pad]).all()
    assert np.isfinite(got[~pad]).all()
    err = np.abs(got[~pad] - ref[~pad])
    bound = (3 * D + 16) * 2.0 ** -23 * mag[~pad]
    print(f"emission S={S} D={D}: worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), np.max(err / bound)
    # the module's method is the same entry (W derived from the factor L = W^-1 it is given)
    import vqhmm
    hmm = vqhmm.GaussianHMM(S, D, covariance_type="full").cuda()
    hmm.mean.data.copy_(torch.from_numpy(model[2]))
    em2 = hmm.emission_log_prob(torch.from_numpy(x).cuda(), torch.from_numpy(L).cuda()).cpu().numpy()
    ident = (np.zeros(1, np.float32), np.zeros((1, 1), np.float32), model[2],
             np.repeat(np.eye(D, dtype=np.float32)[None], S, 0))
    em3 = raw_emission(ident, x, L).cpu().numpy()
    assert np.array_equal(em2.view(np.uint32), em3.view(np.uint32))


def test_upper_triangle_is_never_read():
    model, x, L = make_case(150, 4, 70, 5, 7)
    clean = raw_emission(model, x, L)
    W = model[3].copy()
    W[:, np.triu_indices(7, 1)[0], np.triu_indices(7, 1)[1]] = np.nan
    dirty = raw_emission(model[:3] + (W,), x, L)
    assert torch.equal(clean.view(torch.int32), dirty.view(torch.int32))
    a = raw_estep(model, x, L)
    b = raw_estep(model[:3] + (W,), x, L)
    bits_equal(a, b, COUNTS + ("loglik", "gamma"))


# ------------------------------------------------------------------------------- E-step
@pytest.mark.parametrize("B,T,S,D", SHAPES)
def test_estep_shapes(B, T, S, D):
    model, x, L = make_case(200 + T + D, B, T, S, D)
    shift = x.reshape(-1, D).mean(0)
    check_case(model, x, L, shift=shift, offset=True, tag="shapes")


@pytest.mark.parametrize("T", (64, 128, 129))
def test_estep_chunk_edges(T):
    model, x, L = make_case(300 + T, 6, T, 8, 12)
    check_case(model, x, L, tag="edges")


def test_estep_lengths_around_a_chunk():
    model, x, _ = make_case(400, 3, 65, 8, 12)
    check_case(model, x, [63, 64, 65], tag="63/64/65")


def test_estep_nullable_outputs_weights_and_determinism():
    model, x, L = make_case(500, 9, 70, 5, 7, centre=30.0)
    shift = np.full(7, 30.0, np.float32)
    full = raw_estep(model, x, L, shift=shift)
    again = raw_estep(model, x, L, shift=shift)
    bits_equal(full, again, COUNTS + ("loglik", "gamma"))
    no_g = raw_estep(model, x, L, shift=shift, gamma=False)
    no_l = raw_estep(model, x, L, shift=shift, loglik=False)
    bits_equal(full, no_g, COUNTS + ("loglik",))
    bits_equal(full, no_l, COUNTS + ("gamma",))
    ones = raw_estep(model, x, L, shift=shift, weights=np.ones(9, np.float32))
    bits_equal(full, ones, COUNTS + ("loglik", "gamma"))
    w = np.random.default_rng(501).standard_normal(9).astype(np.float32) * 2
    w[0], w[4] = 0.0, -1.5
    ref, got = check_case(model, x, L, shift=shift, weights=w, tag="weights")
    bits_equal(full, got, ("loglik", "gamma"))   # neither depends on the weights


def test_estep_rows_do_not_depend_on_the_batch():
    rng = np.random.default_rng(600)
    model, x, _ = make_case(600, 600, 40, 4, 3)
    L = rng.integers(1, 41, 600)
    L[:3] = (40, 17, 1)
    small = raw_estep(model, x[:3], L[:3])
    big = raw_estep(model, x, L)
    assert torch.equal(small["loglik"].view(torch.int32), big["loglik"][:3].view(torch.int32))
    assert torch.equal(small["gamma"].view(torch.int32), big["gamma"][:3].view(torch.int32))


@pytest.mark.parametrize("B,T", ((3, 0), (0, 5)))
def test_estep_empty_batch(B, T):
    """B*T == 0: VQHMM_OK, the five counts zeroed (they start as NaN) and loglik NaN for B > 0; the moments
    entry zeroes its three."""
    model = F.random_model(np.random.default_rng(650), 2, 3)
    got = raw_estep(model, np.zeros((B, T, 3), np.float32), np.zeros(B, np.int64))
    for k in COUNTS:
        assert not got[k].any() and not torch.isnan(got[k]).any(), k
    assert got["loglik"].shape == (B,) and torch.isnan(got["loglik"]).all()
    mom = raw_moments(np.zeros((B, T, 3), np.float32), np.zeros((B, T, 2), np.float32), np.zeros(B, np.int64))
    for k in ("occ", "m1", "m2"):
        assert not mom[k].any() and not torch.isnan(mom[k]).any(), k


@pytest.mark.parametrize("T,D", ((1, 1), (64, 5), (130, 17)))
def test_estep_emissions_are_the_emission_entry_bits(T, D):
    """With one state and log_pi = log_A = 0 every step's mass is exactly 1, so loglik is the fp64 sum in time
    order of the emissions the chain used, rounded once: it must equal that sum of the tensor the emission entry
    writes bit for bit, and for L = 1 the emission itself."""
    rng = np.random.default_rng(660 + T)
    B = 6
    W = F.random_model(rng, 1, D)[3]
    model = (np.zeros(1, np.float32), np.zeros((1, 1), np.float32), rng.standard_normal((1, D)).astype(np.float32), W)
    x = (rng.standard_normal((B, T, D)) * 2).astype(np.float32)
    L = np.array([1, T, T, max(T - 1, 1), 1, T])
    em = raw_emission(model, x, L).cpu().numpy()
    got = raw_estep(model, x, L)["loglik"].cpu().numpy()
    want = np.empty(B, np.float32)
    for b in range(B):
        acc = 0.0
        for t in range(int(L[b])):
            acc += float(em[b, t, 0])
        want[b] = np.float32(acc)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert np.array_equal(got[[0, 4]].view(np.uint32), em[[0, 4], 0, 0].view(np.uint32))


# -------------------------------------------------------------------------- hard inputs
HARD = dict(B=6, T=70, S=4, D=3)


def test_hard_far_observations():
    """An observation 60 sigma (of the widest direction of any state) from every mean at t = T // 3 and at t = 0:
    the step runs on exp(em - max em)."""
    model, x, _ = make_case(700, **HARD)
    L = np.array([70, 70, 30, 70, 1, 24])
    Lc = F.scale_tril_of(model[3])
    sd_max = float(np.sqrt(np.linalg.eigvalsh(Lc @ Lc.transpose(0, 2, 1)).max()))
    far = np.abs(model[2]).max() + 60.0 * sd_max
    x[0, 70 // 3] = far
    x[1, 0] = -far
    x[2, 70 // 3] = far
    x[3, 0] = far
    x[3, 70 // 3] = -far
    x[4, 0] = far
    em = raw_emission(model, x, L).cpu().numpy()
    assert em[0, 70 // 3].max() < -1000.0 and em[1, 0].max() < -1000.0
    ref, got = check_case(model, x, L, tag="far")
    assert np.isfinite(ref["loglik"]).all()


def test_hard_nan_inside_and_beyond_the_length():
    model, x, _ = make_case(710, **HARD)
    L = np.array([70, 50, 70, 20, 70, 65])
    clean = raw_estep(model, x, L)
    xn = x.copy()
    xn[1, 60] = np.nan        # beyond the length: never interpreted
    xn[3, 20:, 1] = np.inf
    beyond = raw_estep(model, xn, L)
    bits_equal(clean, beyond, COUNTS + ("loglik", "gamma"))
    xn[2, 69, 2] = np.nan     # inside: the last row of the second chunk
    xn[5, 3, 0] = np.inf      # inside: the first chunk
    got = raw_estep(model, xn, L)
    ll = got["loglik"].cpu().numpy()
    assert np.isnan(ll[[2, 5]]).all() and np.isfinite(ll[[0, 1, 3, 4]]).all()
    assert not got["gamma"][[2, 5]].any()
    keep = [0, 1, 3, 4]
    em = raw_emission(model, x[keep], L[keep]).cpu().numpy()
    ref = F.estep_ref(*model, x[keep], L[keep], em=em)
    check_counts(got, ref, x[keep], L[keep], tag="nan")
    assert np.abs(got["gamma"].cpu().numpy()[keep] - ref["gamma"]).max() <= 1e-5
    rel_ok(ll[keep], ref["loglik"])


def test_hard_impossible_sequence():
    """log_A closes every way out of the only start state: the one sequence longer than 1 is impossible."""
    (log_pi, log_A, mean, W), x, _ = make_case(720, **HARD)
    log_pi = np.array([0.0, NINF, NINF, NINF], np.float32)
    log_A = log_A.copy()
    log_A[0, :] = NINF
    L = np.array([1, 70, 1, 1, 0, 1])
    ref, got = check_case((log_pi, log_A, mean, W), x, L, tag="impossible")
    ll = got["loglik"].cpu().numpy()
    assert ll[1] == NINF and np.isnan(ll[4]) and np.isfinite(ll[[0, 2, 3, 5]]).all()
    assert not got["gamma"][1].any() and got["trans_cnt"].abs().max().item() == 0.0
    assert abs(got["occ"].sum().item() - 4.0) <= 4e-5


def test_hard_length_one_sequences_only():
    model, x, _ = make_case(730, **HARD)
    ref, got = check_case(model, x, np.ones(6, np.int64), shift=np.ones(3, np.float32), tag="L=1")
    assert got["trans_cnt"].abs().max().item() == 0.0
    assert np.abs(got["pi_cnt"].cpu().numpy() - got["occ"].cpu().numpy()).max() == 0.0


# -------------------------------------------------------------------------- return codes
def test_return_codes():
    from vqhmm import _ext
    lib = _ext.load()
    f = torch.zeros(40000, dtype=torch.float32, device="cuda")
    d = torch.zeros(40000, dtype=torch.float64, device="cuda")
    ln = torch.full((2,), 4, dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    p, q, n = _ext.ptr(f), _ext.ptr(d), _ext.ptr(ln)
    st = _ext.stream_ptr()

    def estep(S, D, B=2, T=4, ws_bytes=1 << 20, **null):
        a = dict(log_pi=p, log_A=p, mean=p, prec=p, x=p, lengths=n, pi_cnt=q, trans=q, occ=q, m1=q, m2=q, ws=_ext.ptr(ws))
        a.update({k: None for k in null})
        return lib.vqhmm_gauss_full_estep_f32(a["log_pi"], a["log_A"], a["mean"], a["prec"], a["x"], a["lengths"],
                                              None, None, B, T, S, D, a["pi_cnt"], a["trans"], a["occ"], a["m1"],
                                              a["m2"], None, None, a["ws"], ws_bytes, st)

    for S, D in ((3, 33), (9, 32), (33, 2), (0, 4), (4, 0)):
        assert lib.vqhmm_gauss_full_estep_workspace_size(2, 4, S, D) == 0
        assert lib.vqhmm_gauss_moments_workspace_size(2, 4, S, D) == 0
        assert estep(S, D) == EUNSUPPORTED
        assert lib.vqhmm_gauss_full_emission_f32(p, p, p, n, 2, 4, S, D, p, st) == EUNSUPPORTED
        assert lib.vqhmm_gauss_moments_f32(p, p, n, None, None, 2, 4, S, D, q, q, q, _ext.ptr(ws), 1 << 20,
                                           st) == EUNSUPPORTED
    for S, D in ((32, 16), (8, 32), (3, 12)):
        assert lib.vqhmm_gauss_full_estep_workspace_size(2, 4, S, D) > 0
    assert estep(3, 4, B=-1) == EINVAL
    for k in ("log_pi", "log_A", "mean", "prec", "x", "lengths", "pi_cnt", "trans", "occ", "m1", "m2", "ws"):
        assert estep(3, 4, **{k: True}) == EINVAL, k
    need = lib.vqhmm_gauss_full_estep_workspace_size(2, 4, 3, 4)
    assert estep(3, 4, ws_bytes=need - 1) == EINVAL
    assert estep(3, 4, ws_bytes=need) == 0
    assert lib.vqhmm_gauss_full_emission_f32(p, None, p, n, 2, 4, 3, 4, p, st) == EINVAL
    need = lib.vqhmm_gauss_moments_workspace_size(2, 4, 3, 4)
    assert lib.vqhmm_gauss_moments_f32(p, p, n, None, None, 2, 4, 3, 4, q, q, q, _ext.ptr(ws), need - 1, st) == EINVAL
    assert lib.vqhmm_gauss_moments_f32(p, None, n, None, None, 2, 4, 3, 4, q, q, q, _ext.ptr(ws), need, st) == EINVAL
    assert lib.vqhmm_gauss_moments_f32(p, p, n, None, None, 2, 4, 3, 4, q, None, q, _ext.ptr(ws), need, st) == EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ moments entry
@pytest.mark.parametrize("B,T,S,D", ((6, 70, 3, 12), (5, 130, 32, 16), (5, 130, 8, 32), (4, 1, 1, 1)))
def test_moments_reproduce_the_estep(B, T, S, D):
    """Fed the E-step's own gamma, the moments entry gives the E-step's occ / m1 / m2 within the E-step's bounds
    (twice: each side is within them of the fp64 sums), and the same bits run to run."""
    model, x, L = make_case(850 + T + D, B, T, S, D)
    shift = x.reshape(-1, D).mean(0).astype(np.float32)
    w = np.linspace(0.5, 2.0, B).astype(np.float32)
    es = raw_estep(model, x, L, shift=shift, weights=w)
    gamma = es["gamma"].cpu().numpy()
    got = raw_moments(x, gamma, L, shift=shift, weights=w, offset=True)
    again = raw_moments(x, gamma, L, shift=shift, weights=w, offset=True)
    bits_equal(got, again, ("occ", "m1", "m2"))
    assert torch.equal(got["m2"].view(torch.int64), got["m2"].transpose(1, 2).contiguous().view(torch.int64))
    ref = F.moments_ref(x, gamma, L, shift=shift, weights=w)
    counted = np.where(L > 0, 0.0, np.nan)
    check_counts(got, ref, x, L, shift, w, tag="moments", keys=("occ", "m1", "m2"), counted=counted)
    check_counts(es, ref, x, L, shift, w, tag="estep", keys=("occ", "m1", "m2"), counted=counted)


def test_moments_drop_non_finite_sequences():
    rng = np.random.default_rng(870)
    B, T, S, D = 5, 100, 3, 4
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    g = rng.dirichlet(np.ones(S), (B, T)).astype(np.float32)
    L = np.array([100, 70, 100, 0, 64])
    clean = raw_moments(x[[0, 4]], g[[0, 4]], L[[0, 4]])
    x[1, 69, 2] = np.nan       # inside (second chunk)
    x[1, 80] = np.inf          # beyond
    g[2, 3, 1] = np.inf        # inside (first chunk)
    g[4, 64:] = np.nan         # beyond
    got = raw_moments(x, g, L)
    ref = F.moments_ref(x, g, L)
    counted = np.array([0.0, np.nan, np.nan, np.nan, 0.0])
    check_counts(got, ref, x, L, tag="moments nan", keys=("occ", "m1", "m2"), counted=counted)
    check_counts(clean, ref, x, L, tag="moments clean", keys=("occ", "m1", "m2"), counted=counted)


def test_regime_covariance_against_numpy():
    """A one-hot gamma: per class, the pooled mean and np.cov(bias=True) of the class's rows, to 1e-5 of the
    largest entry."""
    import vqhmm
    rng = np.random.default_rng(880)
    B, T, S, D = 7, 90, 3, 12
    z = rng.integers(0, S, (B, T))
    A = rng.standard_normal((S, D, D)) * 0.5
    x = (5.0 + np.einsum("btij,btj->bti", A[z], rng.standard_normal((B, T, D)))).astype(np.float32)
    L = ragged(881, B, T)
    g = np.eye(S, dtype=np.float32)[z]
    mean, cov = vqhmm.regime_covariance(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(),
                                        torch.from_numpy(L).cuda())
    assert mean.dtype == torch.float64 and cov.shape == (S, D, D)
    inlen = np.arange(T)[None, :] < L[:, None]
    for s in range(S):
        rows = x[inlen & (z == s)].astype(np.float64)
        rm, rc = rows.mean(0), np.cov(rows.T, bias=True)
        assert np.abs(mean[s].cpu().numpy() - rm).max() <= 1e-5 * np.abs(rm).max()
        assert np.abs(cov[s].cpu().numpy() - rc).max() <= 1e-5 * np.abs(rc).max()
    mom = vqhmm.regime_moments(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(L).cuda())
    assert mom["flat"].numel() == S + S * D + S * D * D and mom["m2"].data_ptr() > mom["flat"].data_ptr()
    assert abs(mom["occ"].sum().item() - L.sum()) <= 1e-9


# ------------------------------------------------------------------------------- module
def _full_model(init, S=3, D=F.FIT_D):
    import vqhmm
    hmm = vqhmm.GaussianHMM(S, D, covariance_type="full").cuda()
    for k, v in zip(("log_pi", "log_A", "mean", "scale_tril"), init):
        getattr(hmm, k).data.copy_(torch.from_numpy(np.asarray(v, np.float32)))
    return hmm


def test_state_dict_keys():
    import vqhmm
    assert list(vqhmm.GaussianHMM(3, 4).state_dict()) == ["log_pi", "log_A", "mean", "log_var"]
    assert list(vqhmm.GaussianHMM(3, 4, covariance_type="diag").state_dict()) == ["log_pi", "log_A", "mean", "log_var"]
    full = vqhmm.GaussianHMM(3, 4, covariance_type="full")
    assert list(full.state_dict()) == ["log_pi", "log_A", "mean", "scale_tril"]
    assert torch.equal(full.scale_tril, torch.eye(4).repeat(3, 1, 1))
    assert torch.equal(full.covariances, torch.eye(4).repeat(3, 1, 1))
    with pytest.raises(ValueError):
        vqhmm.GaussianHMM(9, 32, covariance_type="full")
    with pytest.raises(ValueError):
        vqhmm.GaussianHMM(3, 4, covariance_type="tied")


def test_fit_full_against_em_ref():
    """fit(covariance_type="full"), 10 iterations, against em_ref from the same initial parameters at (B,T,S,D) =
    (8,60,3,4): the per-iteration totals to rel 1e-5, the parameters to 1e-3 of their scale (the margin is for
    fp32 parameters re-rounded every iteration).
    Measured on an MI355X: totals 1.9e-8; mean 7.9e-8 and covariances 4.5e-7 of their largest entry, pi 1.4e-8
    and A 5.5e-9 absolute."""
    x, lengths, init = F.fit_case()
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    hmm = _full_model(init)
    hist = hmm.fit(dx, dl, n_iter=10, init=None)
    assert len(hist) == 10 and all(torch.is_tensor(h) for h in hist)
    H._monotone(hist)
    shift = np.concatenate([x[b, :lengths[b]] for b in range(len(lengths))]).astype(np.float64).mean(0)
    cov0 = init[3].astype(np.float64) @ init[3].astype(np.float64).transpose(0, 2, 1)
    (rpi, rA, rmean, rcov), rhist = F.em_ref(init[0], init[1], init[2], cov0, x, lengths, n_iter=10, shift=shift)
    e_h = rel_ok(np.array([float(h) for h in hist]), np.array(rhist), tol=1e-5)
    mean = hmm.mean.detach().cpu().numpy().astype(np.float64)
    cov = hmm.covariances.cpu().numpy().astype(np.float64)
    gaps = dict(hist=e_h, mean=np.abs(mean - rmean).max() / np.abs(rmean).max(),
                cov=np.abs(cov - rcov).max() / np.abs(rcov).max(),
                pi=np.abs(np.exp(hmm.log_pi.cpu().numpy().astype(np.float64)) - np.exp(rpi)).max(),
                A=np.abs(np.exp(hmm.log_A.cpu().numpy().astype(np.float64)) - np.exp(rA)).max())
    print("fit full vs em_ref:", {k: f"{v:.2e}" for k, v in gaps.items()})
    assert all(v <= 1e-3 for k, v in gaps.items() if k != "hist"), gaps
    # the derived properties and the other entry points agree with each other
    W = hmm.precisions_cholesky.double()
    eye = torch.eye(F.FIT_D, dtype=torch.float64, device="cuda")
    assert ((W.transpose(1, 2) @ W) @ hmm.covariances.double() - eye).abs().max().item() <= 1e-4
    pred = hmm.predict(dx, dl)
    assert (pred[1, int(lengths[1]):] == -1).all() and pred[:, 0].min().item() >= 0
    assert torch.equal(pred[0], hmm.posterior(dx, dl)[0].argmax(-1))
    st = hmm.e_step(dx, dl)
    assert torch.equal(hmm.log_prob(dx, dl), st["loglik"]) and st["m2"].shape == (3, F.FIT_D, F.FIT_D)
    assert st["flat"].numel() == 3 + 9 + 3 + 3 * F.FIT_D + 3 * F.FIT_D ** 2


def test_fit_full_mixture_kmeans_and_sample():
    x, lengths, init = F.fit_case()
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    mix = _full_model(init)
    hist = mix.fit(dx, dl, n_iter=10, init=None, mixture=True)
    H._monotone(hist)
    for i in range(3):
        assert torch.equal(mix.log_A[i], mix.log_pi)
    assert abs(torch.exp(mix.log_pi.double()).sum().item() - 1.0) <= 1e-6
    km = _full_model(init)
    hist = km.fit(dx, dl, n_iter=5, generator=torch.Generator(device="cuda").manual_seed(1))
    H._monotone(hist)
    assert torch.isfinite(km.mean).all() and torch.isfinite(km.scale_tril).all()
    assert not km.scale_tril.triu(1).any()
    # a state nothing is counted into keeps its parameters
    lone = _full_model(init)
    with torch.no_grad():
        lone.log_pi.copy_(torch.tensor([0.0, NINF, 0.0]).log_softmax(0))
        lone.log_A[:, 1] = NINF
    before = (lone.mean[1].clone(), lone.scale_tril[1].clone())
    lone.fit(dx, dl, n_iter=2, init=None)
    assert torch.equal(lone.mean[1], before[0]) and torch.equal(lone.scale_tril[1], before[1])
    g = torch.Generator(device="cuda")
    a = mix.sample(64, 50, generator=g.manual_seed(5))
    b = mix.sample(64, 50, generator=g.manual_seed(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape == (64, 50) and a[1].shape == (64, 50, F.FIT_D) and a[0].dtype == torch.int64
    # whitened by the state's W the draws are standard normal
    wz = torch.einsum("ntij,ntj->nti", mix.precisions_cholesky[a[0]], a[1] - mix.mean[a[0]])
    assert abs(wz.mean().item()) <= 0.05 and abs(wz.var().item() - 1.0) <= 0.1
    assert mix.mean_path(5).shape == (5, F.FIT_D)


def test_full_recovers_a_correlation_the_diagonal_model_cannot():
    """Two regimes with the same mean and unit variances; in one of them the two coordinates have correlation 0.9.
    The full model recovers it; the diagonal model cannot tell the regimes apart and ends lower."""
    import vqhmm
    rng = np.random.default_rng(900)
    B, T = 16, 100
    A = np.array([[0.95, 0.05], [0.05, 0.95]])
    cov = np.array([[[1.0, 0.0], [0.0, 1.0]], [[1.0, 0.9], [0.9, 1.0]]])
    x, _ = F.sample_data(rng, np.log([0.5, 0.5]), np.log(A), np.zeros((2, 2)), np.linalg.cholesky(cov), B, T)
    dx = torch.from_numpy(x).cuda()
    start = dict(log_pi=np.log([0.5, 0.5]), log_A=np.log([[0.8, 0.2], [0.2, 0.8]]), mean=[[0.0, 0.0], [0.0, 0.0]])
    full = vqhmm.GaussianHMM(2, 2, covariance_type="full").cuda()
    diag = vqhmm.GaussianHMM(2, 2).cuda()
    with torch.no_grad():
        for m in (full, diag):
            for k, v in start.items():
                getattr(m, k).copy_(torch.tensor(np.asarray(v, np.float32)))
        full.scale_tril.copy_(torch.tensor(np.linalg.cholesky(
            np.array([[[1.0, -0.3], [-0.3, 1.0]], [[1.0, 0.3], [0.3, 1.0]]])).astype(np.float32)))
        diag.log_var.copy_(torch.tensor([[0.2, -0.2], [-0.2, 0.2]]))
    hf = full.fit(dx, n_iter=30, init=None)
    hd = diag.fit(dx, n_iter=30, init=None)
    c = full.covariances.cpu().numpy().astype(np.float64)
    corr = c[:, 0, 1] / np.sqrt(c[:, 0, 0] * c[:, 1, 1])
    print("correlations", corr, "final loglik full", float(hf[-1]), "diag", float(hd[-1]))
    assert abs(corr.max() - 0.9) <= 0.05 and abs(corr.min()) <= 0.15
    assert float(hd[-1]) < float(hf[-1])


def _dense_loglik(log_pi, log_A, mean, scale_tril, x, lengths):
    """The forward algorithm in torch fp64 (autograd reference)."""
    dist = torch.distributions.MultivariateNormal(mean, scale_tril=scale_tril.tril())
    em = dist.log_prob(x[:, :, None, :])
    out = []
    for b in range(x.shape[0]):
        al = log_pi + em[b, 0]
        for t in range(1, int(lengths[b])):
            al = torch.logsumexp(al[:, None] + log_A, 0) + em[b, t]
        out.append(torch.logsumexp(al, 0))
    return torch.stack(out)


def test_gauss_full_log_prob_gradients():
    """Against fp64 autograd of the dense forward algorithm at (6,40,3,4), rel 1e-4 of each gradient's max-abs.
    Measured on an MI355X: log_pi 2.3e-8, log_A 1.1e-7, mean 1.1e-6, scale_tril 2.3e-6."""
    import vqhmm
    B, T, S, D = 6, 40, 3, 4
    model, x, _ = make_case(800, B, T, S, D)
    Lc = F.scale_tril_of(model[3]).astype(np.float32)
    L = np.array([40, 1, 2, 33, 40, 17])
    c = np.random.default_rng(801).standard_normal(B)
    p32 = [torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_() for a in model[:3] + (Lc,)]
    ll = vqhmm.gauss_full_log_prob(*p32, torch.from_numpy(x).cuda(), torch.from_numpy(L).cuda())
    (ll.double() * torch.from_numpy(c).cuda()).sum().backward()
    p64 = [torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_() for a in model[:3] + (Lc,)]
    ll64 = _dense_loglik(*p64, torch.from_numpy(x).double(), L)
    (ll64 * torch.from_numpy(c)).sum().backward()
    rel_ok(ll.detach().cpu().numpy(), ll64.detach().numpy())
    worst = {}
    for name, a, b in zip(("log_pi", "log_A", "mean", "scale_tril"), p32, p64):
        g, r = a.grad.double().cpu().numpy(), b.grad.numpy()
        worst[name] = np.abs(g - r).max() / np.abs(r).max()
    print("gauss_full_log_prob gradient errors (rel. to max-abs):", {k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= 1e-4 for v in worst.values()), worst
    assert not p32[3].grad.triu(1).any()
    with pytest.raises(ValueError):
        vqhmm.gauss_full_log_prob(*p32, torch.from_numpy(x).cuda().requires_grad_())
