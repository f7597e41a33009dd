"""CPU checks of tests/code_ens_ref.py, the fp64 reference the GPU tests of the batched / weighted E-step, the
gradient and the mixture of HMMs are held to (tests/test_gpu_code_ensemble.py)."""
import numpy as np

import code_ens_ref as E
import code_hmm_ref as R


def test_integer_weights_equal_repeated_sequences():
    rng = np.random.default_rng(1)
    S, V, B, T = 3, 5, 6, 9
    models = [R.random_model(np.random.default_rng(10 + m), S, V) for m in range(2)]
    codes = rng.integers(0, V, (B, T)).astype(np.int32)
    L = np.array([T, 0, 1, 2, 5, 7], np.int64)
    w = np.array([[2, 3, 1, 0, 4, 1], [1, 1, 0, 3, 2, 2]])
    got = E.estep_ens_ref(models, codes, L, w)
    for m in range(2):
        rep = np.repeat(np.arange(B), w[m])
        ref = R.estep_ref(*models[m], codes[rep], L[rep])
        for k in ("pi_cnt", "trans_cnt", "emit_cnt"):
            assert np.allclose(got[m][k], ref[k], rtol=0, atol=1e-12), (m, k)
        assert np.array_equal(got[m]["loglik"], R.estep_ref(*models[m], codes, L)["loglik"], equal_nan=True)
    # a (B,) weight is every member's
    one = E.estep_ens_ref(models, codes, L, w[0])
    assert np.array_equal(one[1]["emit_cnt"], E.estep_ens_ref(models[1:], codes, L, w[:1])[0]["emit_cnt"])


def test_weighted_counts_are_the_gradient_finite_difference():
    """d/d(log-parameter) of sum_b g_b loglik_b = the weighted counts: central differences, h = 1e-5, at
    S = 2, V = 3, B = 3, T = 4.  Error of the difference quotient: O(h^2) + rounding 1e-16 / h ~ 1e-10."""
    rng = np.random.default_rng(2)
    S, V, B, T = 2, 3, 3, 4
    model = [a.astype(np.float64) for a in R.random_model(rng, S, V)]
    codes = rng.integers(0, V, (B, T)).astype(np.int32)
    L = np.array([4, 2, 3], np.int64)
    g = np.array([0.7, -1.3, 2.0])
    cnt = E.estep_ens_ref([tuple(model)], codes, L, g)[0]

    def f(mod):
        return float((g * R.estep_ref(*mod, codes, L)["loglik"]).sum())

    h = 1e-5
    for k, name in enumerate(("pi_cnt", "trans_cnt", "emit_cnt")):
        for idx in np.ndindex(model[k].shape):
            up = [a.copy() for a in model]
            dn = [a.copy() for a in model]
            up[k][idx] += h
            dn[k][idx] -= h
            fd = (f(up) - f(dn)) / (2 * h)
            assert abs(fd - cnt[name][idx]) <= 1e-8, (name, idx, fd, cnt[name][idx])


def test_responsibilities_rule():
    ll = np.array([[-1.0, np.nan, -np.inf, np.nan], [-2.0, -3.0, -np.inf, -np.inf]])
    r, ok, tot = E.responsibilities_ref(np.log([0.5, 0.5]), ll)
    assert ok.tolist() == [True, True, False, False]
    assert np.allclose(r[:, 0], np.exp([-1.0, -2.0]) / np.exp([-1.0, -2.0]).sum())
    assert r[:, 1].tolist() == [0.0, 1.0] and not r[:, 2:].any()
    assert np.isclose(tot, np.log(0.5 * (np.exp(-1) + np.exp(-2))) + np.log(0.5) - 3.0)


def test_mixture_reference_on_the_planted_case():
    codes, L, labels, start, log_mix = E.planted_mixture_case()
    assert codes.shape == (E.MIX_B, E.MIX_T) and len(start) == E.MIX_M
    hist, models, mix, r = E.mixture_ref(start, log_mix, codes, L, n_iter=5)
    assert len(hist) == 5 and np.isfinite(hist).all()
    # the exact EM (prior_count = 0) never decreases the log-likelihood; the slack is fp64 rounding
    assert (np.diff(hist) >= -1e-9 * np.abs(hist[:-1])).all(), hist
    # the input condition of the GPU test: the reference alone assigns all 24, up to a label swap
    hist6, _, _, r6 = E.mixture_ref(start, log_mix, codes, L, n_iter=6)
    for rr in (r, r6):
        assign = rr.argmax(0)
        assert max((assign == labels).sum(), (assign == 1 - labels).sum()) == E.MIX_B
        # ... and decisively: the GPU's responsibilities move by 2 delta << this margin
        assert np.abs(rr[0] - rr[1]).min() > 0.5
    assert np.isclose(np.exp(mix).sum(), 1.0)
