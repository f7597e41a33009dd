"""CPU checks of the regime-path samplers: the numpy reference's draw rule IS the posterior (and the
prior walk), its corner cases, the margins of every exact GPU case, and the host-only side of the
two C-ABI entry points.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import sample_ref as SR
from hmm_pair_ref import brute_force
from test_cabi import declared_functions

NEW_SYMBOLS = ("vqhmm_ffbs_sample_f32", "vqhmm_markov_sample_f32")
PY_NAMES = ("sample_posterior_paths", "simulate_paths", "sampled_regimes", "simulate_regimes")


def _cond_prob(rows_of, first, path, backward):
    """product of the reference's conditional draw probabilities along one path"""
    order = list(range(len(path) - 1, -1, -1)) if backward else list(range(len(path)))
    p = 1.0
    for n, t in enumerate(order):
        if n == 0:
            w = first
        else:
            prev_t = order[n - 1]
            w = rows_of(max(t, prev_t))[path[prev_t]]
        p *= w[path[t]] / w.sum()
    return p


@pytest.mark.parametrize("K,T", [(2, 4), (3, 3), (3, 4), (2, 1), (1, 3)])
def test_rule_is_the_posterior_and_the_prior(K, T):
    rng = np.random.default_rng(10 * K + T)
    log_pi, log_A, em = SR.random_tables(rng, 1, T, K)
    filt, loglik, _, _ = brute_force(log_pi, log_A[0], em[0], T)
    f64 = lambda a: np.asarray(a, np.float64)
    # the reference's tables, on the exact fp64 filter (no fp32 rounding in this check)
    ffbs_rows = lambda t: (filt[t - 1][:, None] * np.exp(f64(log_A[0, t]) - f64(log_A[0, t]).max(0))).T
    mk_rows = lambda t: np.exp(f64(log_A[0, t]) - f64(log_A[0, t]).max(1, keepdims=True))
    pi_w = np.exp(f64(log_pi) - f64(log_pi).max())
    # the prior walk's law is pi * prod A with every row normalised (the fp32 tables' rows sum to 1
    # only to fp32 precision, and the walk normalises each row it draws from)
    npi, nA = SR.log_softmax(log_pi), SR.log_softmax(log_A, axis=3)
    tot_post = tot_prior = 0.0
    for path in itertools.product(range(K), repeat=T):
        lw = f64(log_pi)[path[0]] + f64(em)[0, 0, path[0]]
        lp = npi[path[0]]
        for t in range(1, T):
            lw += f64(log_A)[0, t, path[t - 1], path[t]] + f64(em)[0, t, path[t]]
            lp += nA[0, t, path[t - 1], path[t]]
        post = np.exp(lw - loglik)
        got = _cond_prob(ffbs_rows, filt[T - 1], path, True)
        assert abs(got - post) <= 1e-12 * post, (path, got, post)
        gotp = _cond_prob(mk_rows, pi_w, path, False)
        assert abs(gotp - np.exp(lp)) <= 1e-12 * np.exp(lp), (path, gotp, np.exp(lp))
        tot_post += got
        tot_prior += gotp
    assert abs(tot_post - 1) < 1e-12 and abs(tot_prior - 1) < 1e-12


def test_reference_walk_uses_the_rule_tables():
    """ffbs_ref / markov_ref draw by draw_rule on exactly the tables of the check above: with K = 2
    and u = 0 every draw is the first state of positive weight, with u just under 1 the last."""
    rng = np.random.default_rng(3)
    log_pi, log_A, em = SR.random_tables(rng, 2, 5, 2)
    filt = SR.pair_ref(log_pi, log_A, em)["filt"].astype(np.float32)
    L = np.array([5, 3])
    for u, want in ((0.0, 0), (np.float32(1) - np.float32(2.0 ** -24), 1)):
        uu = np.full((2, 3, 5), u, np.float32)
        for paths in (SR.ffbs_ref(filt, log_A, L, uu)[0], SR.markov_ref(log_pi, log_A, L, uu)[0]):
            assert (paths[0] == want).all() and (paths[1, :, :3] == want).all() and (paths[1, :, 3:] == -1).all()


def test_draw_rule_corner_cases():
    w = np.array([[0.0, 0.5, 0.0, 0.5, 0.0]])
    # zero-weight states are never drawn, at u = 0, on a boundary and just under 1
    assert SR.draw_rule(w, [0.0])[0][0] == 1
    assert SR.draw_rule(w, [0.25])[0][0] == 1
    assert SR.draw_rule(w, [0.5])[0][0] == 3  # cdf_1 = 0.5 is not > u: the next positive state
    assert SR.draw_rule(w, [float(np.float32(1) - np.float32(2.0 ** -24))])[0][0] == 3
    # margins: the only interior boundary is 0.5 (0 and 1 are excluded)
    assert SR.draw_rule(w, [0.0])[1][0] == 0.5
    assert abs(SR.draw_rule(w, [0.5 + 1e-9])[1][0] - 1e-9) < 1e-15
    # a single state has no boundary
    z, m = SR.draw_rule(np.array([[3.0]]), [0.7])
    assert z[0] == 0 and m[0] == np.inf
    # all-zero, NaN and infinite totals fail
    for bad in ([0.0, 0.0], [np.nan, 1.0], [np.inf, 1.0]):
        z, m = SR.draw_rule(np.array([bad]), [0.3])
        assert z[0] == -1 and m[0] == np.inf


def test_failed_draw_gives_minus_one_onward():
    K, T = 3, 6
    rng = np.random.default_rng(5)
    log_pi, log_A, em = SR.random_tables(rng, 1, T, K)
    u = rng.random((1, 4, T), dtype=np.float32)
    # simulation: every row of step 3 is -inf, so z_3 and everything after fails
    A = log_A.copy()
    A[0, 3] = -np.inf
    p = SR.markov_ref(log_pi, A, [T], u)[0]
    assert (p[0, :, :3] >= 0).all() and (p[0, :, 3:] == -1).all()
    # FFBS walks backward: an all-zero filt row at t = 2 fails z_2 and leaves z_1, z_0 at -1
    filt = SR.pair_ref(log_pi, log_A, em)["filt"].astype(np.float32)
    filt[0, 2] = 0
    p = SR.ffbs_ref(filt, log_A, [T], u)[0]
    assert (p[0, :, 3:] >= 0).all() and (p[0, :, :3] == -1).all()
    # a column of -inf (state 1 unreachable at step 4) fails only the samples that sit in it
    A = log_A.copy()
    A[0, 4, :, 1] = -np.inf
    filt = SR.pair_ref(log_pi, log_A, em)["filt"].astype(np.float32)
    p = SR.ffbs_ref(filt, A, [T], u)[0]
    hit = p[0, :, 4] == 1
    assert (p[0, hit, :4] == -1).all() and (p[0, ~hit] >= 0).all()


@pytest.mark.parametrize("K,T,N", SR.EXACT_CASES)
def test_exact_case_margins_and_range(K, T, N):
    c = SR.exact_case(K, T, N)
    L = c["lengths"]
    for paths, u_used, margins in (c["ffbs"], c["markov"]):
        assert u_used.dtype == np.float32 and (u_used >= 0).all() and (u_used < 1).all()
        assert (margins >= SR.bound(K)).all()
        assert paths.dtype == np.int32 and paths.max() < K
        for b in range(SR.B_CASE):
            assert (paths[b, :, :L[b]] >= 0).all() and (paths[b, :, L[b]:] == -1).all()
        # the fixed-up uniforms reproduce the same paths without any further fix
    again = SR.ffbs_ref(c["filt"], c["log_A"], L, c["ffbs"][1])[0]
    assert np.array_equal(again, c["ffbs"][0])


def test_bulk_case_excludes_at_most_a_thousandth():
    c = SR.bulk_case()
    for paths, keep in (c["ffbs"], c["markov"]):
        assert paths.shape == (1, 50000, 4) and (paths >= 0).all()
        assert (~keep).sum() <= 0.001 * keep.size


def test_stat_case_reference_within_four_sigma():
    """The committed seed of the end-to-end statistics test: the numpy reference on the same
    uniforms stays within 4 standard deviations (+ 2 / N), so the GPU test's 5 leave margin."""
    c = SR.stat_case()
    L = c["lengths"]
    post = SR.ffbs_ref(c["filt"].astype(np.float32), c["log_A"], L, c["u"])[0]
    assert SR.freq_excess(post, c["gamma"], L, 4.0) <= 0
    sim = SR.markov_ref(c["log_pi"], c["log_A"], L, c["u"])[0]
    assert SR.freq_excess(sim, c["prior"], L, 4.0) <= 0
    assert abs(c["prior"][0, -1].sum() - 1) < 1e-12


def test_symbols_declared_exported_and_bound():
    from vqhmm import _ext
    lib = _ext.load()
    names = declared_functions()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(lib, n) and n in _ext.exported_symbols()
    assert lib.vqhmm_abi_version() == _ext.ABI_VERSION == 8


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_host_only_return_codes(name):
    from vqhmm import _ext
    fn = getattr(_ext.load(), name)
    one = ctypes.c_void_p(16)  # never dereferenced: every call below returns before a launch
    assert fn(None, None, None, None, 2, 4, 3, 5, None, None) == -1  # null pointers, non-empty problem
    assert fn(one, one, one, one, 2, 4, 3, 5, None, None) == -1
    assert fn(one, one, one, one, 2, 4, 33, 5, one, None) == -4  # K outside [1, 32]
    assert fn(one, one, one, one, 2, 4, 0, 5, one, None) == -4
    assert fn(None, None, None, None, 2, 4, 33, 5, None, None) == -4  # ... is checked before the pointers
    assert fn(None, None, None, None, 2, 4, 3, 0, None, None) == 0  # N = 0: nothing to do
    assert fn(None, None, None, None, 0, 4, 3, 5, None, None) == 0
    assert fn(None, None, None, None, 2, 0, 3, 5, None, None) == 0
    assert fn(one, one, one, one, 2, 4, 3, -1, one, None) == -1  # a negative size
    assert fn(one, one, one, one, -2, 4, 33, 5, one, None) == -1  # ... comes first


def test_python_names_exported():
    import vqhmm
    for n in PY_NAMES:
        assert callable(getattr(vqhmm, n)) and n in vqhmm.__all__


def test_cpu_tensors_fail_loudly():
    import torch
    import vqhmm
    log_pi, log_A, em = torch.zeros(2), torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2)
    with pytest.raises(RuntimeError, match="HIP"):
        vqhmm.sample_posterior_paths(log_pi, log_A, em, n_samples=2)
    with pytest.raises(RuntimeError, match="HIP"):
        vqhmm.simulate_paths(log_pi, log_A, n_samples=2)
