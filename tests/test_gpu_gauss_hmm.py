"""GPU checks of the Gaussian HMM (vqhmm_gauss_emission_f32 / vqhmm_gauss_estep_f32 / vqhmm_gauss_sample_f32,
hmm_gauss.hip, vqhmm.GaussianHMM, vqhmm.gauss_log_prob) against the fp64 restatement in tests/gauss_hmm_ref.py.

Emissions: against fp64 on the same fp32 inputs, |d| <= (D + 16) 2^-23 A[b,t,s] with A = sum_d (z^2/2 +
|log_var|/2) + (D/2) ln 2 pi: the bound of a D-term fp32 sum in any order, with slack for the exp.

E-step: against the fp64 reference fed the emission tensor the emission entry wrote (the chain's error apart
from the emission rounding), with the project's bounds for these chain numerics: gamma abs 1e-5, loglik rel 1e-5
of max(1, |ref|), pi_cnt 1e-5 x (sequences with L > 0), trans_cnt 2e-5 x (transition positions), occ 1e-5 x
(in-length positions), m1 / m2 [s,d] 2e-5 x the sum of |x_d - shift_d| / (x_d - shift_d)^2 over the in-length
positions.  With weights every position counts |w_b| times (w = 1 gives the bounds as stated).
The sampler is compared exactly: tests/test_gauss_hmm_ref.py vets the uniforms' distance from every CDF boundary.
"""
import itertools

import numpy as np
import pytest
import torch

import gauss_hmm_ref as R
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
NINF = -np.inf
COUNTS = ("pi_cnt", "trans_cnt", "occ", "m1", "m2")
SHAPES = ((5, 1, 1, 1), (6, 63, 3, 5), (7, 65, 17, 33), (5, 130, 32, 64))   # (B, T, S, D)


def ragged(seed, B, T):
    """Lengths with T, 0, 1 and 2 first (as far as B and T allow), then random ones."""
    rng = np.random.default_rng(seed)
    L = np.concatenate([[T, 0, 1, 2], rng.integers(0, T + 1, max(B - 4, 0))])[:B]
    return np.minimum(L, T).astype(np.int64)


def dev_f32(a, offset=False):
    """On the device; offset: an exact-size view 4 bytes into its allocation (16-byte alignment broken, the last
    element is the allocation's last)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32)
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def raw_emission(model, x, lengths, offset=False, fill=7.0):
    from vqhmm import _ext
    lib = _ext.load()
    mean, log_var = (dev_f32(a, offset) for a in model[2:])
    S, D = mean.shape
    B, T = x.shape[:2]
    d_x = dev_f32(x, offset)
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    em = guarded((B, T, S), torch.float32, fill=fill)
    rc = lib.vqhmm_gauss_emission_f32(_ext.ptr(mean), _ext.ptr(log_var), _ext.ptr(d_x), _ext.ptr(d_len), B, T, S, D,
                                      em.ptr, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(em)
    return em.t


def raw_estep(model, x, lengths, shift=None, weights=None, loglik=True, gamma=True, offset=False):
    """vqhmm_gauss_estep_f32 through ctypes on guarded exact-size buffers and a guarded, poisoned workspace of exactly the
    queried size (gpu_buffers.guarded); the counts start as NaN (the call must write
    every element) -> dict of device tensors."""
    from vqhmm import _ext
    lib = _ext.load()
    log_pi, log_A, mean, log_var = (dev_f32(a, offset) for a in model)
    S, D = mean.shape
    B, T = x.shape[:2]
    d_x = dev_f32(x, offset)
    d_len = torch.from_numpy(np.asarray(lengths, np.int64)).cuda()
    d_sh, d_w = dev_f32(shift, offset), dev_f32(weights, offset)
    cnt = {k: guarded(sh, torch.float64, fill=float("nan"))
           for k, sh in zip(COUNTS, ((S,), (S, S), (S,), (S, D), (S, D)))}
    ll = guarded((B,), torch.float32, fill=7.0) if loglik else None
    gm = guarded((B, T, S), torch.float32, fill=7.0) if gamma else None
    nb = lib.vqhmm_gauss_estep_workspace_size(B, T, S, D)
    ws = guarded(nb, torch.uint8)  # exactly the queried size, poisoned
    rc = lib.vqhmm_gauss_estep_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(log_var), _ext.ptr(d_x),
                                   _ext.ptr(d_len), _ext.ptr(d_sh), _ext.ptr(d_w), B, T, S, D,
                                   *(cnt[k].ptr for k in COUNTS), ll.ptr if loglik else None, gm.ptr if gamma else None, ws.ptr, nb,
                                   _ext.stream_ptr())
    assert rc == 0, rc
    check_all(*cnt.values(), ll, gm, ws)
    return dict({k: g.t for k, g in cnt.items()}, loglik=ll.t if loglik else None, gamma=gm.t if gamma else None)


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


def count_bounds(ref, x, lengths, shift, weights):
    """The per-position contracts summed over the sequences that count -> dict of bounds (m1, m2: (D,))."""
    B, T, D = x.shape
    L = np.clip(np.asarray(lengths, np.int64), 0, T)
    w = np.ones(B) if weights is None else np.abs(np.asarray(weights, np.float64))
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    counted = np.isfinite(ref["loglik"]) & (L > 0)
    s1, s2 = np.zeros(D), np.zeros(D)
    for b in np.nonzero(counted)[0]:
        y = np.asarray(x[b, :L[b]], np.float64) - sh
        s1 += w[b] * np.abs(y).sum(0)
        s2 += w[b] * (y * y).sum(0)
    return dict(pi_cnt=1e-5 * w[counted].sum(), trans_cnt=2e-5 * (w[counted] * (L[counted] - 1)).sum(),
                occ=1e-5 * (w[counted] * L[counted]).sum(), m1=2e-5 * s1[None, :], m2=2e-5 * s2[None, :])


def check_counts(got, ref, x, lengths, shift=None, weights=None, tag=""):
    bounds = count_bounds(ref, x, lengths, shift, weights)
    msg = []
    bad = []
    for k in COUNTS:
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
    ref = R.estep_ref(*model, x, lengths, shift=shift, weights=weights, em=em)
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
    return ref, got


def make_case(seed, B, T, S, D, lengths=None, centre=0.0):
    """A random model and data scattered around its means (every state gets visited)."""
    rng = np.random.default_rng(seed)
    log_pi, log_A, mean, log_var = R.random_model(rng, S, D)
    mean = (mean + centre).astype(np.float32)
    z = rng.integers(0, S, (B, T))
    x = (mean[z] + np.exp(0.5 * log_var[z]) * rng.standard_normal((B, T, D)) * 1.5).astype(np.float32)
    L = ragged(seed + 1, B, T) if lengths is None else np.asarray(lengths, np.int64)
    return (log_pi, log_A, mean, log_var), x, L


def bits_equal(a, b, keys):
    for k in keys:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


# ---------------------------------------------------------------------------- emissions
@pytest.mark.parametrize("fill", (7.0, float("nan")))
@pytest.mark.parametrize("B,T,S,D", SHAPES)
def test_emission_against_fp64(B, T, S, D, fill):
    model, x, L = make_case(100 + T, B, T, S, D)
    x[0, T - 1] += 40.0   # a far observation: the bound scales with z^2
    got = raw_emission(model, x, L, offset=True, fill=fill).cpu().numpy().astype(np.float64)
    ref, mag = R.emission_ref(model[2], model[3], x, L)
    pad = np.arange(T)[None, :] >= L[:, None]
    assert np.isneginf(got[pad]).all()
    assert np.isfinite(got[~pad]).all()
    err = np.abs(got[~pad] - ref[~pad])
    bound = (D + 16) * 2.0 ** -23 * mag[~pad]
    print(f"emission S={S} D={D}: worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), np.max(err / bound)
    # the module's method is the same entry
    import vqhmm
    hmm = vqhmm.GaussianHMM(S, D).cuda()
    for k, v in zip(("log_pi", "log_A", "mean", "log_var"), model):
        getattr(hmm, k).data.copy_(torch.from_numpy(v))
    em2 = hmm.emission_log_prob(torch.from_numpy(x).cuda(), torch.from_numpy(L).cuda())
    assert np.array_equal(em2.cpu().numpy().astype(np.float64), got)


# ------------------------------------------------------------------------------- E-step
@pytest.mark.parametrize("B,T,S,D", SHAPES)
def test_estep_shapes(B, T, S, D):
    model, x, L = make_case(200 + T, B, T, S, D)
    shift = x.reshape(-1, D).mean(0)
    check_case(model, x, L, shift=shift, offset=True, tag="shapes")


@pytest.mark.parametrize("T", (64, 128, 129))
def test_estep_chunk_edges(T):
    model, x, L = make_case(300 + T, 6, T, 8, 16)
    check_case(model, x, L, tag="edges")


def test_estep_lengths_around_a_chunk():
    model, x, _ = make_case(400, 3, 65, 8, 16)
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
    """B*T == 0: VQHMM_OK, the five counts zeroed (they start as NaN) and loglik NaN for B > 0."""
    model = R.random_model(np.random.default_rng(650), 2, 3)
    got = raw_estep(model, np.zeros((B, T, 3), np.float32), np.zeros(B, np.int64))
    for k in COUNTS:
        assert not got[k].any() and not torch.isnan(got[k]).any(), k
    assert got["loglik"].shape == (B,) and torch.isnan(got["loglik"]).all()


@pytest.mark.parametrize("T,D", ((1, 1), (64, 5), (130, 33)))
def test_estep_emissions_are_the_emission_entry_bits(T, D):
    """With one state and log_pi = log_A = 0 every step's mass is exactly 1, so loglik is the fp64 sum in time
    order of the emissions the chain used, rounded once: it must equal that sum of the tensor the emission
    entry writes bit for bit, and for L = 1 the emission itself (a one-ulp difference in the internal emission,
    such as a contracted multiply-add, shows)."""
    rng = np.random.default_rng(660 + T)
    B = 6
    model = (np.zeros(1, np.float32), np.zeros((1, 1), np.float32), rng.standard_normal((1, D)).astype(np.float32),
             rng.uniform(-1, 1, (1, D)).astype(np.float32))
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
    """An observation 60 sigma from every mean at t = T // 3 and at t = 0: the step runs on exp(em - max em)."""
    model, x, _ = make_case(700, **HARD)
    L = np.array([70, 70, 30, 70, 1, 24])
    sd_max = float(np.exp(0.5 * model[3]).max())
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
    ref = R.estep_ref(*model, x[keep], L[keep], em=em)
    check_counts(got, ref, x[keep], L[keep], tag="nan")
    assert np.abs(got["gamma"].cpu().numpy()[keep] - ref["gamma"]).max() <= 1e-5
    rel_ok(ll[keep], ref["loglik"])


def test_hard_impossible_sequence():
    """log_A closes every way out of the only start state: the one sequence longer than 1 is impossible."""
    (log_pi, log_A, mean, log_var), x, _ = make_case(720, **HARD)
    log_pi = np.array([0.0, NINF, NINF, NINF], np.float32)
    log_A = log_A.copy()
    log_A[0, :] = NINF
    L = np.array([1, 70, 1, 1, 0, 1])
    ref, got = check_case((log_pi, log_A, mean, log_var), x, L, tag="impossible")
    ll = got["loglik"].cpu().numpy()
    assert ll[1] == NINF and np.isnan(ll[4]) and np.isfinite(ll[[0, 2, 3, 5]]).all()
    assert not got["gamma"][1].any() and got["trans_cnt"].abs().max().item() == 0.0
    assert abs(got["occ"].sum().item() - 4.0) <= 4e-5


def test_hard_length_one_sequences_only():
    model, x, _ = make_case(730, **HARD)
    ref, got = check_case(model, x, np.ones(6, np.int64), shift=np.ones(3, np.float32), tag="L=1")
    assert got["trans_cnt"].abs().max().item() == 0.0
    assert np.abs(got["pi_cnt"].cpu().numpy() - got["occ"].cpu().numpy()).max() == 0.0


# ------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("S,D,seed", R.SAMPLER_CASES)
def test_sampler_bit_equal(S, D, seed):
    from vqhmm import _ext
    log_pi, log_A, mean, log_var, u, nr = R.sampler_case(S, D, seed)
    st_ref, x_ref, _ = R.sample_ref(log_pi, log_A, mean, log_var, u, nr)
    N, T = u.shape
    d = [dev_f32(a, True) for a in (log_pi, log_A, mean, log_var, u, nr)]
    states = torch.full((N, T), -7, dtype=torch.int32, device="cuda")
    x = torch.full((N, T, D), float("nan"), dtype=torch.float32, device="cuda")
    rc = _ext.load().vqhmm_gauss_sample_f32(*(_ext.ptr(t) for t in d), N, T, S, D, _ext.ptr(states), _ext.ptr(x),
                                            _ext.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(states.cpu().numpy(), st_ref)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), x_ref.view(np.uint32))


def test_sample_method_is_reproducible_and_plausible():
    import vqhmm
    hmm = vqhmm.GaussianHMM(3, 2, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        hmm.mean.copy_(torch.tensor([[-5.0, -5.0], [0.0, 0.0], [5.0, 5.0]]))
    g = torch.Generator(device="cuda")
    a = hmm.sample(64, 50, generator=g.manual_seed(5))
    b = hmm.sample(64, 50, generator=g.manual_seed(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape == (64, 50) and a[1].shape == (64, 50, 2) and a[0].dtype == torch.int64
    assert (a[1] - hmm.mean[a[0]]).abs().max().item() < 6.0   # unit variances
    mp = hmm.mean_path(50)
    assert np.abs(mp.numpy() - R.mean_path_ref(hmm.log_pi.cpu().numpy(), hmm.log_A.cpu().numpy(),
                                               hmm.mean.cpu().numpy(), 50)).max() <= 1e-12


# ----------------------------------------------------------------------- gauss_log_prob
def _dense_loglik(log_pi, log_A, mean, log_var, x, lengths):
    """The forward algorithm in torch fp64 (autograd reference)."""
    D = x.shape[-1]
    em = -0.5 * (((x[:, :, None, :] - mean) ** 2) * torch.exp(-log_var) + log_var).sum(-1) - 0.5 * D * R.LN2PI
    out = []
    for b in range(x.shape[0]):
        al = log_pi + em[b, 0]
        for t in range(1, int(lengths[b])):
            al = torch.logsumexp(al[:, None] + log_A, 0) + em[b, t]
        out.append(torch.logsumexp(al, 0))
    return torch.stack(out)


def test_gauss_log_prob_gradients():
    """Against fp64 autograd of the dense forward algorithm, rel 1e-4 of each gradient's max-abs.
    Measured on an MI355X: log_pi 6.8e-8, log_A 1.0e-7, mean 4.4e-7, log_var 9.3e-7."""
    import vqhmm
    B, T, S, D = 6, 40, 3, 4
    model, x, _ = make_case(800, B, T, S, D)
    L = np.array([40, 1, 2, 33, 40, 17])
    c = np.random.default_rng(801).standard_normal(B)
    p32 = [torch.from_numpy(a).cuda().requires_grad_() for a in model]
    ll = vqhmm.gauss_log_prob(*p32, torch.from_numpy(x).cuda(), torch.from_numpy(L).cuda())
    (ll.double() * torch.from_numpy(c).cuda()).sum().backward()
    p64 = [torch.from_numpy(a).double().requires_grad_() for a in model]
    ll64 = _dense_loglik(*p64, torch.from_numpy(x).double(), L)
    (ll64 * torch.from_numpy(c)).sum().backward()
    rel_ok(ll.detach().cpu().numpy(), ll64.detach().numpy())
    worst = {}
    for name, a, b in zip(("log_pi", "log_A", "mean", "log_var"), p32, p64):
        g, r = a.grad.double().cpu().numpy(), b.grad.numpy()
        worst[name] = np.abs(g - r).max() / np.abs(r).max()
    print("gauss_log_prob gradient errors (rel. to max-abs):", {k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= 1e-4 for v in worst.values()), worst
    with pytest.raises(ValueError):
        vqhmm.gauss_log_prob(*p32, torch.from_numpy(x).cuda().requires_grad_())


# ---------------------------------------------------------------------------------- fit
def _fit_model(init):
    import vqhmm
    hmm = vqhmm.GaussianHMM(3, R.FIT_D).cuda()
    for k, v in zip(("log_pi", "log_A", "mean", "log_var"), init):
        getattr(hmm, k).data.copy_(torch.from_numpy(np.asarray(v, np.float32)))
    return hmm


def _monotone(hist):
    hist = [float(h) for h in hist]
    assert all(np.isfinite(hist))
    for a, b in zip(hist, hist[1:]):
        assert b >= a - 1e-4 * max(1.0, abs(a)), hist


def test_fit_recovers_planted_states():
    x, lengths, init = R.fit_case()
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    hmm = _fit_model(init)
    hist = hmm.fit(dx, dl, n_iter=10, init=None)
    assert len(hist) == 10
    _monotone(hist)
    mean = hmm.mean.detach().cpu().numpy().astype(np.float64)
    best = min(np.abs(mean[list(p)] - R.FIT_MEANS[:, None]).max() for p in itertools.permutations(range(3)))
    assert best <= 0.1, best
    # the fp64 reference EM from the same start ends at the same place
    shift = np.concatenate([x[b, :lengths[b]] for b in range(len(lengths))]).astype(np.float64).mean(0)
    (rpi, rA, rmean, rlv), rhist = R.em_ref(*init, x, lengths, n_iter=10, shift=shift)
    assert np.abs(mean - rmean).max() <= 1e-3 and np.abs(hmm.log_var.detach().cpu().numpy() - rlv).max() <= 1e-3
    rel_ok(np.array([float(h) for h in hist]), np.array(rhist), tol=1e-4)
    # predict follows the posterior
    pred = hmm.predict(dx, dl)
    assert (pred[1, int(lengths[1]):] == -1).all() and pred[:, 0].min().item() >= 0
    assert torch.equal(pred[0], hmm.posterior(dx, dl)[0].argmax(-1))
    assert torch.equal(hmm.log_prob(dx, dl), hmm.e_step(dx, dl)["loglik"])


def test_fit_kmeans_init_and_mixture():
    x, lengths, init = R.fit_case()
    dx, dl = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    hmm = _fit_model(init)
    hist = hmm.fit(dx, dl, n_iter=10, generator=torch.Generator(device="cuda").manual_seed(1))
    _monotone(hist)
    assert torch.isfinite(hmm.mean).all() and torch.isfinite(hmm.log_var).all()
    mix = _fit_model(init)
    hist = mix.fit(dx, dl, n_iter=10, init=None, mixture=True)
    _monotone(hist)
    for i in range(3):
        assert torch.equal(mix.log_A[i], mix.log_pi)
    assert abs(torch.exp(mix.log_pi.double()).sum().item() - 1.0) <= 1e-6
    mean = mix.mean.detach().cpu().numpy().astype(np.float64)
    best = min(np.abs(mean[list(p)] - R.FIT_MEANS[:, None]).max() for p in itertools.permutations(range(3)))
    assert best <= 0.1, best


# ---------------------------------------------------------------------------- old route
def test_counts_agree_with_the_pairwise_route():
    """The time-varying kernels on the expanded tables (emission tensor -> log_A (B,T,S,S) -> pairwise_posteriors
    -> moment sums in torch) give the same counts within the bounds above."""
    import vqhmm
    B, T, S, D = 8, 65, 5, 7
    model, x, L = make_case(900, B, T, S, D)
    shift = x.reshape(-1, D).mean(0).astype(np.float32)
    got = raw_estep(model, x, L, shift=shift)
    em = raw_emission(model, x, L)
    d = [torch.from_numpy(a).cuda() for a in model]
    dl = torch.from_numpy(L).cuda()
    gamma, xi, logz = vqhmm.pairwise_posteriors(d[0], d[1].expand(B, T, S, S).contiguous(), em, dl)
    ok = (torch.isfinite(logz) & (dl > 0)).double()
    g = gamma.double() * ok[:, None, None]
    y = torch.from_numpy(x).cuda().double() - torch.from_numpy(shift).cuda().double()
    y = torch.where((torch.arange(T, device="cuda")[None, :] < dl[:, None])[:, :, None], y, 0.0)
    old = dict(pi_cnt=g[:, 0].sum(0), trans_cnt=(xi.double() * ok[:, None, None, None]).sum((0, 1)), occ=g.sum((0, 1)),
               m1=torch.einsum("bts,btd->sd", g, y), m2=torch.einsum("bts,btd->sd", g, y * y))
    ref = {k: v.cpu().numpy() for k, v in old.items()}
    ref["loglik"] = logz.double().cpu().numpy()
    check_counts(got, ref, x, L, shift=shift, tag="old route")
    assert (gamma - got["gamma"]).abs().max().item() <= 1e-5
    rel_ok(got["loglik"].cpu().numpy(), np.where(L > 0, ref["loglik"], np.nan))
