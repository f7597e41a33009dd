"""CPU checks of tests/gauss_ens_ref.py, the fp64 reference the GPU tests of the batched / weighted Gaussian E-step,
the ensemble's padding, M-step and BIC and the mixture of Gaussian HMMs are held to
(tests/test_gpu_gauss_ensemble.py)."""
import numpy as np
import pytest

import gauss_ens_ref as E
import gauss_full_ref as F
import gauss_hmm_ref as G

FORMS = pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])


def _models(full, M, S, D, seed):
    return [(F if full else G).random_model(np.random.default_rng(seed + m), S, D) for m in range(M)]


@FORMS
def test_weighted_counts_against_brute_force(full):
    """S = 2, D = 2, T <= 5: the weighted sum of each sequence's enumerated counts, to fp64 rounding."""
    rng = np.random.default_rng(5)
    S, D, B, T = 2, 2, 4, 5
    models = _models(full, 2, S, D, 40)
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    L = np.array([5, 3, 0, 1], np.int64)
    shift = np.array([0.25, -0.5], np.float32)
    w = np.array([[1.5, -0.75, 2.0, 0.0], [0.5, 1.0, -1.0, 3.0]])
    got = E.estep_ens_ref(models, x, L, shift=shift, weights=w, full=full)
    for m, model in enumerate(models):
        acc = None
        for b in range(B):
            last = model[3]
            if full:   # brute_force takes the covariances
                Ls = F.scale_tril_of(last)
                last = np.einsum("sij,skj->sik", Ls, Ls)
            one = (F if full else G).brute_force(model[0], model[1], model[2], last, x[b, :L[b]], shift=shift,
                                                 weight=w[m, b])
            if L[b] == 0:
                assert np.isnan(got[m]["loglik"][b])
                continue
            assert abs(got[m]["loglik"][b] - one["loglik"]) <= 1e-10 * max(1.0, abs(one["loglik"]))
            acc = one if acc is None else {k: acc[k] + one[k] for k in ("pi_cnt", "trans_cnt", "occ", "m1", "m2")}
        for k in ("pi_cnt", "trans_cnt", "occ", "m1", "m2"):
            assert np.allclose(got[m][k], acc[k], rtol=0, atol=1e-10), (m, k)
        assert got[m]["abs_w"].tolist() == [abs(w[m, 0]), abs(w[m, 1]), 0.0, abs(w[m, 3])]


@FORMS
def test_padded_member_equals_the_unpadded_model(full):
    rng = np.random.default_rng(6)
    D, B, T, S = 3, 3, 9, 5
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    L = np.array([9, 4, 1], np.int64)
    for s in (2, 3):
        model = _models(full, 1, s, D, 60 + s)[0]
        padded = E.pad_model(model, S)
        assert padded[0].shape == (S,) and np.isneginf(padded[0][s:]).all()
        assert np.isneginf(padded[1][s:]).all() and np.isneginf(padded[1][:, s:]).all()
        assert np.array_equal(padded[3][s:], np.repeat(model[3][:1], S - s, 0))
        a = E.estep_ens_ref([model], x, L, full=full)[0]
        b = E.estep_ens_ref([padded], x, L, full=full)[0]
        assert np.allclose(a["loglik"], b["loglik"], rtol=1e-13, atol=0)
        assert np.allclose(b["gamma"][:, :, :s], a["gamma"], rtol=0, atol=1e-13)
        assert not b["gamma"][:, :, s:].any() and not b["occ"][s:].any() and not b["m1"][s:].any()
        for k in ("pi_cnt", "occ", "m1", "m2"):
            assert np.allclose(b[k][:s], a[k], rtol=0, atol=1e-11), k
        assert np.allclose(b["trans_cnt"][:s, :s], a["trans_cnt"], rtol=0, atol=1e-11)
        assert not b["trans_cnt"][s:].any() and not b["trans_cnt"][:, s:].any()


def test_free_parameters_and_bic_formula():
    lp = np.log(np.full(3, 1 / 3))
    A = np.log(np.full((3, 3), 1 / 3))
    mean = np.zeros((3, 4))
    assert E.num_free_parameters_ref((lp, A, mean, None)) == 2 + 6 + 2 * 3 * 4
    assert E.num_free_parameters_ref((lp, A, mean, None), full=True) == 2 + 6 + 3 * (4 + 10)
    assert E.num_free_parameters_ref((lp, A, mean, None), full=True, mixture=True) == 2 + 2 + 3 * (4 + 10)
    A2 = A.copy()
    A2[0, 2] = -np.inf          # a structural zero is no parameter
    lp2 = np.array([0.0, -np.inf, -np.inf])
    assert E.num_free_parameters_ref((lp2, A2, mean, None)) == 0 + 5 + 24
    assert E.bic_ref(-100.0, 7, 50) == 200.0 + 7 * np.log(50)


@FORMS
def test_mixture_reference_is_monotone(full):
    rng = np.random.default_rng(8)
    D, T = 2, 12
    centres = (-3.0, 3.0)
    x = np.concatenate([c + rng.standard_normal((5, T, D)) for c in centres]).astype(np.float32)
    L = np.full(10, T, np.int64)
    L[[2, 7]] = [5, 9]
    models = []
    for m in range(2):
        lp, A, mean, _ = G.random_model(np.random.default_rng(80 + m), 2, D)
        last = np.repeat(np.eye(D)[None] * 4.0, 2, 0) if full else np.full((2, D), np.log(4.0))
        models.append((lp, A, mean, last))
    hist, out, mix, r = E.mixture_ref(models, np.log([0.5, 0.5]), x, L, n_iter=5, shift=E.data_shift(x, L), full=full)
    assert np.isfinite(hist).all()
    # the exact EM with a variance floor far below the fitted variances never decreases the log-likelihood
    assert (np.diff(hist) >= -1e-9 * np.abs(hist[:-1])).all(), hist
    assert np.isclose(np.exp(mix).sum(), 1.0) and np.allclose(r.sum(0), 1.0)


@FORMS
def test_planted_selection_case_selects_three_states(full):
    """The input condition of the GPU test: the fp64 reference EM alone selects S = 3 by BIC, and by more than
    SEL_MARGIN, far above what the kernels' loglik tolerance (1e-5 of ~1e3) can move a BIC."""
    bic, ll, p = E.selection_ref(full)
    print("bic", bic, "loglik", ll, "free", p)
    assert E.SEL_SIZES[int(np.argmin(bic))] == 3
    others = np.delete(bic, E.SEL_SIZES.index(3))
    assert (others - bic[E.SEL_SIZES.index(3)] > E.SEL_MARGIN).all()
