"""CPU checks of the Gaussian HMM: the fp64 helper (tests/gauss_hmm_ref.py) against brute force, the M-step,
shift invariance, the reference EM on the fit test's data, the C-ABI's host-side behaviour, the Python surface
and the margins of the sampler test's uniforms.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import gauss_hmm_ref as R
from conftest import ROOT

NINF = -np.inf
NEW_SYMBOLS = ("vqhmm_gauss_emission_f32", "vqhmm_gauss_estep_workspace_size", "vqhmm_gauss_estep_f32",
               "vqhmm_gauss_sample_f32")
COUNTS = ("pi_cnt", "trans_cnt", "occ", "m1", "m2")


@pytest.mark.parametrize("S,T,D", [(1, 3, 1), (2, 5, 2), (3, 4, 2), (3, 5, 1)])
def test_helper_matches_brute_force(S, T, D):
    rng = np.random.default_rng(13 * S + 5 * T + D)
    log_pi, log_A, mean, log_var = (a.astype(np.float64) for a in R.random_model(rng, S, D))
    if S >= 2:
        log_A[0, 1] = NINF   # a structural zero transition
    x = rng.standard_normal((4, T, D)) * 2
    lengths = np.array([T, T - 1, 1, 0])
    shift = rng.standard_normal(D)
    w = np.array([1.0, -0.5, 2.0, 3.0])
    got = R.estep_ref(log_pi, log_A, mean, log_var, x, lengths, shift=shift, weights=w)
    want = {k: 0.0 for k in COUNTS}
    for b in range(4):
        n = int(lengths[b])
        bf = R.brute_force(log_pi, log_A, mean, log_var, x[b, :n], shift=shift, weight=w[b])
        if n == 0:
            assert np.isnan(got["loglik"][b]) and np.isnan(bf["loglik"])
        else:
            assert abs(got["loglik"][b] - bf["loglik"]) <= 1e-12
        assert np.abs(got["gamma"][b, :n] - bf["gamma"]).max(initial=0.0) <= 1e-12
        assert not got["gamma"][b, n:].any()
        for k in COUNTS:
            want[k] = want[k] + bf[k]
    for k in COUNTS:
        assert np.abs(got[k] - want[k]).max() <= 1e-12, k
    if S >= 2:
        assert got["trans_cnt"][0, 1] == 0.0
    # xi sums to the transition counts, gamma to the occupancies
    assert np.abs((got["xi"] * w[:, None, None, None]).sum((0, 1)) - got["trans_cnt"]).max() <= 1e-12
    assert np.abs((got["gamma"] * w[:, None, None]).sum((0, 1)) - got["occ"]).max() <= 1e-12


def test_helper_degenerate_sequences():
    rng = np.random.default_rng(3)
    S, T, D = 2, 4, 2
    log_pi, log_A, mean, log_var = (a.astype(np.float64) for a in R.random_model(rng, S, D))
    x = rng.standard_normal((3, T, D))
    base = R.estep_ref(log_pi, log_A, mean, log_var, x[:2])
    # an impossible sequence: state 1 cannot start and nothing leads to it, state 0 cannot stay
    imp_pi, imp_A = np.array([0.0, NINF]), np.array([[NINF, NINF], [0.0, 0.0]])
    got = R.estep_ref(imp_pi, imp_A, mean, log_var, x[:1])
    assert got["loglik"][0] == NINF and R.brute_force(imp_pi, imp_A, mean, log_var, x[0])["loglik"] == NINF
    for k in COUNTS + ("gamma",):
        assert not got[k].any()
    # NaN inside the length: loglik NaN, out of the counts; beyond the length: nothing changes
    xn = x.copy()
    xn[2, 1, 0] = np.nan
    got = R.estep_ref(log_pi, log_A, mean, log_var, xn)
    assert np.isnan(got["loglik"][2]) and not got["gamma"][2].any()
    for k in COUNTS:
        assert np.array_equal(got[k], base[k])
    got = R.estep_ref(log_pi, log_A, mean, log_var, xn, lengths=[T, T, 1])
    ref = R.estep_ref(log_pi, log_A, mean, log_var, x, lengths=[T, T, 1])
    for k in COUNTS + ("loglik", "gamma"):
        assert np.array_equal(got[k], ref[k])


def test_emission_helper_is_the_normal_density():
    rng = np.random.default_rng(4)
    S, D = 3, 4
    _, _, mean, log_var = R.random_model(rng, S, D)
    x = rng.standard_normal((2, 5, D))
    em, mag = R.emission_ref(mean, log_var, x, [5, 2])
    var = np.exp(log_var.astype(np.float64))
    for s in range(S):
        want = (-0.5 * np.log(2 * np.pi * var[s]) - (x - mean[s]) ** 2 / (2 * var[s])).sum(-1)
        assert np.abs(em[0, :, s] - want[0]).max() <= 1e-12
    assert np.isneginf(em[1, 2:]).all() and np.isfinite(em[1, :2]).all()
    assert (mag >= np.abs(np.where(np.isfinite(em), em, 0)) - 1e-9).all()


def test_mstep_reproduces_planted_moments():
    rng = np.random.default_rng(8)
    S, D = 3, 2
    old = [a.astype(np.float64) for a in R.random_model(rng, S, D)]
    old[1][0, 2] = NINF
    mu = rng.standard_normal((S, D)) * 3 + 100.0
    var = rng.uniform(0.5, 2.0, (S, D))
    occ = np.array([10.0, 0.0, 2.5])
    shift = np.full(D, 99.0)
    counts = dict(pi_cnt=rng.random(S), trans_cnt=rng.random((S, S)), occ=occ,
                  m1=occ[:, None] * (mu - shift), m2=occ[:, None] * (var + (mu - shift) ** 2))
    counts["trans_cnt"][0, 2] = 0.0
    npi, nA, nmean, nlv = R.mstep_ref(counts, *old, shift=shift)
    assert np.abs(nmean[[0, 2]] - mu[[0, 2]]).max() <= 1e-12
    assert np.abs(np.exp(nlv[[0, 2]]) - var[[0, 2]]).max() <= 1e-10
    assert np.array_equal(nmean[1], old[2][1]) and np.array_equal(nlv[1], old[3][1])  # occ = 0 keeps its row
    assert nA[0, 2] == NINF and np.abs(np.exp(nA).sum(1) - 1).max() <= 1e-12
    assert np.allclose(np.exp(npi), counts["pi_cnt"] / counts["pi_cnt"].sum())
    # the floor
    counts["m2"][0] = occ[0] * (mu[0] - shift) ** 2
    assert np.allclose(np.exp(R.mstep_ref(counts, *old, shift=shift, var_floor=1e-3)[3][0]), 1e-3)
    # a mixture: pi from the occupancies, every row of A equal to it
    mpi, mA, _, _ = R.mstep_ref(counts, old[0], np.zeros((S, S)), old[2], old[3], shift=shift, mixture=True)
    assert np.allclose(np.exp(mpi), occ / occ.sum()) and all(np.array_equal(mA[i], mpi) for i in range(S))


def test_mstep_of_the_package_matches_the_helper():
    import torch
    import vqhmm
    rng = np.random.default_rng(2)
    S, D = 3, 2
    hmm = vqhmm.GaussianHMM(S, D, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        hmm.log_A[0, 2] = float("-inf")
    old = [p.detach().numpy().copy() for p in (hmm.log_pi, hmm.log_A, hmm.mean, hmm.log_var)]
    occ = np.array([4.0, 0.0, 1.5])
    shift = np.array([0.5, -2.0], np.float32)
    counts = dict(pi_cnt=rng.random(S), trans_cnt=rng.random((S, S)), occ=occ, m1=rng.standard_normal((S, D)),
                  m2=rng.random((S, D)) + 3.0)
    for mixture in (False, True):
        for k, v in zip(("log_pi", "log_A", "mean", "log_var"), old):
            getattr(hmm, k).data.copy_(torch.tensor(v))
        hmm.mixture = mixture
        t = {k: torch.tensor(v) for k, v in counts.items()}
        t["shift"] = torch.tensor(shift)
        hmm.m_step(t, prior_count=0.25, var_floor=1e-4)
        ref = R.mstep_ref(counts, *old, shift=shift, prior_count=0.25, var_floor=1e-4, mixture=mixture)
        for got, want in zip((hmm.log_pi, hmm.log_A, hmm.mean, hmm.log_var), ref):
            assert np.allclose(got.detach().numpy(), want, rtol=0, atol=2e-6)
            assert np.array_equal(np.isinf(got.detach().numpy()), np.isinf(want))


def test_shift_invariance():
    """The M-step's result does not depend on the shift the moments were taken about."""
    rng = np.random.default_rng(6)
    S, T, D = 3, 12, 2
    model = [a.astype(np.float64) for a in R.random_model(rng, S, D)]
    x = R.sample_data(rng, model, 5, T).astype(np.float64) + 50.0
    model[2] = model[2] + 50.0
    outs = []
    for shift in (None, np.full(D, 50.0), x.reshape(-1, D).mean(0)):
        c = R.estep_ref(*model, x, [T, 3, 0, T, 7], shift=shift)
        outs.append(R.mstep_ref(c, *model, shift=shift))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.abs(a - b).max() <= 1e-9


def test_mean_path_helper():
    rng = np.random.default_rng(1)
    log_pi, log_A, mean, _ = R.random_model(rng, 3, 2)
    mp = R.mean_path_ref(log_pi, log_A, mean, 4)
    pi, A = np.exp(log_pi.astype(np.float64)), np.exp(log_A.astype(np.float64))
    pi, A = pi / pi.sum(), A / A.sum(1, keepdims=True)
    assert np.allclose(mp[0], pi @ mean) and np.allclose(mp[3], pi @ A @ A @ A @ mean)
    import torch
    import vqhmm
    hmm = vqhmm.GaussianHMM(3, 2)
    for k, v in zip(("log_pi", "log_A", "mean"), (log_pi, log_A, mean)):
        getattr(hmm, k).data.copy_(torch.tensor(v))
    assert np.abs(hmm.mean_path(4).numpy() - mp).max() <= 1e-12


def test_reference_em_recovers_the_planted_states():
    """The conditions the GPU fit test sets, met by the fp64 reference EM alone on the same data and
    initialisation: loglik never decreases by more than 1e-4 max(1, |ll|) over 10 iterations and every
    recovered mean is within 0.1 of its planted value, up to permutation."""
    x, lengths, init = R.fit_case()
    shift = np.concatenate([x[b, :lengths[b]] for b in range(len(lengths))]).astype(np.float64).mean(0)
    (_, nA, nmean, nlv), hist = R.em_ref(*init, x, lengths, n_iter=10, shift=shift)
    for a, b in zip(hist, hist[1:]):
        assert b >= a - 1e-4 * max(1.0, abs(a))
    best = min(np.abs(nmean[list(p)] - R.FIT_MEANS[:, None]).max() for p in itertools.permutations(range(3)))
    assert best <= 0.1, best
    assert np.abs(np.exp(nlv) - 1.0).max() <= 0.1
    # ... and as a mixture every row of A is pi
    (mpi, mA, _, _), _ = R.em_ref(*init, x, lengths, n_iter=3, shift=shift, mixture=True)
    assert all(np.array_equal(mA[i], mpi) for i in range(3))


def test_new_symbols_declared_exported_and_bound():
    import vqhmm
    from vqhmm import _ext
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vqhmm.h")).read(), flags=re.S)
    lib = _ext.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _ext.exported_symbols(), name
    assert lib.vqhmm_abi_version() == 8
    assert "GaussianHMM" in vqhmm.__all__ and "gauss_log_prob" in vqhmm.__all__
    assert callable(vqhmm.gauss_log_prob)


def test_host_checks_without_gpu():
    """Every VQHMM_E* path, in the documented order: they run before any launch."""
    from vqhmm import _ext
    lib = _ext.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, T, S, D = 2, 3, 2, 4
    need = lib.vqhmm_gauss_estep_workspace_size(B, T, S, D)
    assert need > 0

    def estep(B=B, T=T, S=S, D=D, hole=None, ws=1 << 20):
        args = [p, p, p, p, p, p, None, None, B, T, S, D, p, p, p, p, p, None, None, p, ws, None]
        if hole is not None:
            args[hole] = None
        return lib.vqhmm_gauss_estep_f32(*args)

    # a negative size first, whatever else is wrong
    for kw in (dict(B=-1), dict(T=-1), dict(S=-1), dict(D=-1), dict(B=-1, S=33)):
        assert estep(**kw) == -1, kw
    # then the supported range, before any pointer is looked at
    for kw in (dict(S=0), dict(S=33), dict(D=0), dict(D=65)):
        assert estep(**kw) == -4, kw
        assert lib.vqhmm_gauss_estep_f32(*([None] * 8), B, T, kw.get("S", S), kw.get("D", D), *([None] * 7), None, 0,
                                         None) == -4
    # required pointers, each on its own (shift, weights, loglik and gamma are nullable)
    for hole in (0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 19):
        assert estep(hole=hole) == -1, hole
    assert estep(ws=need - 1) == -1
    # the emission entry and the sampler
    em = lambda *a: lib.vqhmm_gauss_emission_f32(*a)  # noqa: E731
    assert em(p, p, p, p, -1, T, S, D, p, None) == -1
    assert em(p, p, p, p, B, T, 33, D, p, None) == -4
    assert em(p, p, p, p, B, T, S, 65, p, None) == -4
    assert em(None, None, None, None, 0, T, S, D, None, None) == 0
    assert em(None, None, None, None, B, 0, S, D, None, None) == 0
    for hole in (0, 1, 2, 3, 8):
        args = [p, p, p, p, B, T, S, D, p, None]
        args[hole] = None
        assert em(*args) == -1, hole
    sm = lambda *a: lib.vqhmm_gauss_sample_f32(*a)  # noqa: E731
    assert sm(p, p, p, p, p, p, 2, -3, S, D, p, p, None) == -1
    assert sm(p, p, p, p, p, p, 2, 3, 0, D, p, p, None) == -4
    assert sm(p, p, p, p, p, p, 2, 3, S, 65, p, p, None) == -4
    assert sm(None, None, None, None, None, None, 0, 3, S, D, None, None, None) == 0
    for hole in (0, 1, 2, 3, 4, 5, 10, 11):
        args = [p, p, p, p, p, p, 2, 3, S, D, p, p, None]
        args[hole] = None
        assert sm(*args) == -1, hole


def test_workspace_query_limits():
    from vqhmm import _ext
    lib = _ext.load()
    q = lib.vqhmm_gauss_estep_workspace_size
    assert q(4, 16, 32, 64) > 0
    for S, D in ((33, 8), (0, 8), (8, 65), (8, 0)):
        assert q(4, 16, S, D) == 0
    assert q(-1, 16, 8, 8) == 0
    assert q(1024, 512, 8, 5) >= 1024 * 512 * 8 * 4  # at least the scaled forward vectors
    # sizes the launch refuses (T > 2^28, B >= 2^31, B*T > 2^40) have no workspace size either, and the product
    # never wraps into a small one
    for B, T in (((1 << 31), 16), (4, (1 << 28) + 1), ((1 << 31) - 1, 1 << 28), ((1 << 20) + 1, 1 << 20)):
        assert q(B, T, 32, 64) == 0, (B, T)
    assert q(1 << 20, 1 << 20, 32, 64) >= (1 << 40) * 32 * 4


def test_python_surface_and_cpu_refusal():
    import torch
    import vqhmm
    for m in ("emission_log_prob", "e_step", "log_prob", "posterior", "predict", "m_step", "init_kmeans", "fit",
              "mean_path", "sample", "as_mixture"):
        assert callable(getattr(vqhmm.GaussianHMM, m))
    hmm = vqhmm.GaussianHMM(3, 5, generator=torch.Generator().manual_seed(1))
    assert {k: tuple(v.shape) for k, v in hmm.named_parameters()} == {
        "log_pi": (3,), "log_A": (3, 3), "mean": (3, 5), "log_var": (3, 5)}
    other = vqhmm.GaussianHMM(3, 5, generator=torch.Generator().manual_seed(2))
    assert not torch.equal(other.mean, hmm.mean)
    other.load_state_dict(hmm.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), hmm.state_dict().values()))
    mix = vqhmm.GaussianHMM(3, 5).as_mixture()
    assert all(torch.equal(mix.log_A[i], mix.log_pi) for i in range(3))
    x = torch.zeros(2, 4, 5)
    for call in (lambda: hmm.e_step(x), lambda: hmm.log_prob(x), lambda: hmm.posterior(x), lambda: hmm.predict(x),
                 lambda: hmm.emission_log_prob(x), lambda: hmm.fit(x, n_iter=1), lambda: hmm.sample(2, 3),
                 lambda: vqhmm.gauss_log_prob(hmm.log_pi, hmm.log_A, hmm.mean, hmm.log_var, x)):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(ValueError):
        vqhmm.gauss_log_prob(hmm.log_pi, hmm.log_A, hmm.mean, hmm.log_var, x.requires_grad_())
    with pytest.raises(ValueError):
        vqhmm.GaussianHMM(33, 5)
    with pytest.raises(ValueError):
        vqhmm.GaussianHMM(3, 65)


@pytest.mark.parametrize("S,D,seed", R.SAMPLER_CASES)
def test_sampler_uniforms_keep_their_distance(S, D, seed):
    """The GPU test demands exact equality with nothing excluded, so no uniform may sit near a CDF boundary:
    every draw along the reference path is at least 1e-4 from the nearest one (the fp32 CDF's error is
    (S + 4) 2^-23 <= 4.3e-6)."""
    log_pi, log_A, mean, log_var, u, nr = R.sampler_case(S, D, seed)
    assert u.shape == (R.SAMPLER_N, R.SAMPLER_T) and u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    assert nr.shape == (R.SAMPLER_N, R.SAMPLER_T, D) and nr.dtype == np.float32
    states, x, margins = R.sample_ref(log_pi, log_A, mean, log_var, u, nr)
    if S > 1:
        assert margins.min() >= R.SAMPLER_MARGIN
    assert states.min() >= 0 and states.max() < S and x.dtype == np.float32 and np.isfinite(x).all()
