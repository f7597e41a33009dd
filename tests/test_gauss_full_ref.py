"""The fp64 restatement of the full-covariance Gaussian HMM (tests/gauss_full_ref.py) checked against independent
statements of the same mathematics: a brute-force enumeration of the state paths, the diagonal model's
restatement, scikit-learn's full-covariance GaussianMixture, and EM's monotonicity.  No GPU."""
import numpy as np
import pytest

import gauss_full_ref as F
import gauss_hmm_ref as G

COUNTS = ("pi_cnt", "trans_cnt", "occ", "m1", "m2")


@pytest.mark.parametrize("S,L,D,seed", ((2, 5, 2, 0), (3, 4, 3, 1), (1, 3, 2, 2), (3, 1, 2, 3)))
def test_estep_against_brute_force(S, L, D, seed):
    rng = np.random.default_rng(seed)
    log_pi, log_A, mean, W = F.random_model(rng, S, D)
    if S > 1:
        log_A = log_A.copy()
        log_A[0, 1] = -np.inf   # a structural zero
    x = (rng.standard_normal((1, L, D)) * 2).astype(np.float32)
    shift = rng.standard_normal(D)
    Lc = F.scale_tril_of(W)
    cov = Lc @ Lc.transpose(0, 2, 1)
    ref = F.estep_ref(log_pi, log_A, mean, W, x, shift=shift, weights=np.array([1.7]))
    bf = F.brute_force(log_pi, log_A, mean, cov, x[0], shift=shift, weight=1.7)
    assert abs(ref["loglik"][0] - bf["loglik"]) <= 1e-10 * max(1.0, abs(bf["loglik"]))
    assert np.abs(ref["gamma"][0] - bf["gamma"]).max() <= 1e-10
    for k in COUNTS:
        assert np.abs(ref[k] - bf[k]).max() <= 1e-9 * max(1.0, np.abs(bf[k]).max()), k
    assert np.abs(ref["m2"] - ref["m2"].transpose(0, 2, 1)).max() <= 1e-12 * max(1.0, np.abs(ref["m2"]).max())


def test_reduces_to_the_diagonal_model():
    """A diagonal W = diag(exp(-log_var / 2)): the emissions are the diagonal restatement's, m2's diagonal is the
    diagonal model's m2, and the other counts agree."""
    rng = np.random.default_rng(5)
    S, D, B, T = 4, 5, 3, 17
    log_pi, log_A, mean, log_var = G.random_model(rng, S, D)
    W = np.zeros((S, D, D))
    W[:, np.arange(D), np.arange(D)] = np.exp(-0.5 * log_var.astype(np.float64))
    x = (rng.standard_normal((B, T, D)) * 2).astype(np.float32)
    L = np.array([T, 0, 9])
    em_f, _ = F.emission_ref(mean, W, x, L)
    em_d, _ = G.emission_ref(mean, log_var, x, L)
    fin = np.isfinite(em_d)
    assert np.array_equal(fin, np.isfinite(em_f))
    assert np.abs(em_f[fin] - em_d[fin]).max() <= 1e-12 * np.abs(em_d[fin]).max()
    shift = x.reshape(-1, D).mean(0)
    w = np.array([0.5, 2.0, -1.0])
    full = F.estep_ref(log_pi, log_A, mean, W, x, L, shift=shift, weights=w)
    diag = G.estep_ref(log_pi, log_A, mean, log_var, x, L, shift=shift, weights=w)
    for k in ("pi_cnt", "trans_cnt", "occ", "m1", "gamma"):
        assert np.abs(full[k] - diag[k]).max() <= 1e-10, k
    d2 = np.diagonal(full["m2"], axis1=1, axis2=2)
    assert np.abs(d2 - diag["m2"]).max() <= 1e-10 * max(1.0, np.abs(diag["m2"]).max())
    # moments_ref under the E-step's own gamma gives the E-step's moments
    mom = F.moments_ref(x, full["gamma"], L, shift=shift, weights=w)
    for k in ("occ", "m1", "m2"):
        assert np.abs(mom[k] - full[k]).max() <= 1e-10 * max(1.0, np.abs(full[k]).max()), k


def test_bound_magnitude_dominates_the_emission():
    rng = np.random.default_rng(6)
    _, _, mean, W = F.random_model(rng, 3, 6)
    x = (rng.standard_normal((2, 9, 6)) * 3).astype(np.float32)
    em, mag = F.emission_ref(mean, W, x)
    assert (mag >= np.abs(em) - 1e-12).all()


def test_mixture_em_against_sklearn():
    """em_ref(mixture=True) is sklearn's GaussianMixture(covariance_type="full") run for the same number of
    iterations from the same parameters (S = 3, D = 12, N = 600, 7 iterations): weights, means and covariances
    within 1e-10 of the largest entry."""
    mixture = pytest.importorskip("sklearn.mixture")
    import warnings
    rng = np.random.default_rng(12)
    S, D, N, n_it = 3, 12, 600, 7
    _, _, mean, W = F.random_model(rng, S, D, spread=1.5)
    Lc = F.scale_tril_of(W)
    z = rng.integers(0, S, N)
    x = (mean[z] + np.einsum("nij,nj->ni", Lc[z], rng.standard_normal((N, D)))).astype(np.float32)
    w0 = np.full(S, 1.0 / S)
    mu0 = x[rng.choice(N, S, replace=False)].astype(np.float64)
    cov0 = np.repeat(np.cov(x.T.astype(np.float64))[None], S, 0)
    gm = mixture.GaussianMixture(n_components=S, covariance_type="full", weights_init=w0, means_init=mu0,
                                 precisions_init=np.linalg.inv(cov0), max_iter=n_it, tol=0.0, reg_covar=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # "did not converge": the iteration count is the point
        gm.fit(x.astype(np.float64))
    assert gm.n_iter_ == n_it
    # the mixture as an HMM whose rows of A are pi, on N sequences of length 1
    log_pi = np.log(w0)
    (rpi, rA, rmean, rcov), hist = F.em_ref(log_pi, np.repeat(log_pi[None], S, 0), mu0, cov0, x[:, None, :],
                                            n_iter=n_it, reg_covar=1e-6, mixture=True)
    for name, got, ref in (("weights", np.exp(rpi), gm.weights_), ("means", rmean, gm.means_),
                           ("covariances", rcov, gm.covariances_)):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"{name}: {err:.2e}")
        assert err <= 1e-10, (name, err)
    assert np.array_equal(rA, np.repeat(rpi[None], S, 0))


def test_em_is_monotone_on_hmm_data():
    x, lengths, init = F.fit_case()
    cov0 = init[3].astype(np.float64) @ init[3].astype(np.float64).transpose(0, 2, 1)
    shift = np.concatenate([x[b, :lengths[b]] for b in range(len(lengths))]).astype(np.float64).mean(0)
    p, hist = F.em_ref(init[0], init[1], init[2], cov0, x, lengths, n_iter=8, shift=shift)
    assert all(np.isfinite(hist))
    for a, b in zip(hist, hist[1:]):
        assert b >= a - 1e-9 * abs(a), hist
    assert hist[-1] > hist[0] + 1.0
    for c in p[3]:
        assert np.linalg.eigvalsh(c).min() > 0
