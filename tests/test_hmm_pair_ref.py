"""CPU checks for the pairwise-posterior feature: the fp64 helper (tests/hmm_pair_ref.py) pinned by
brute-force enumeration, its marginal identities, and the C-ABI boundary of the three new entry
points (declared, exported, bound, null pointers rejected on the host).  No GPU needed."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import hmm_pair_ref as PR

HEADER = os.path.join(ROOT, "include", "vqhmm.h")
NEW = ("vqhmm_filter_f32", "vqhmm_fwdbwd_xi_workspace_size", "vqhmm_fwdbwd_xi_f32")


def log_softmax(a, axis=-1):
    m = a.max(axis=axis, keepdims=True)
    return a - m - np.log(np.exp(a - m).sum(axis=axis, keepdims=True))


def tables(seed, B, T, K):
    rng = np.random.default_rng(seed)
    return (log_softmax(rng.standard_normal(K)), log_softmax(rng.standard_normal((B, T, K, K)) * 1.5),
            log_softmax(rng.standard_normal((B, T, K)) * 2.0))


@pytest.mark.parametrize("K,T", [(1, 3), (2, 6), (3, 6), (4, 5)])
def test_helper_vs_brute_force(K, T):
    B = 4
    log_pi, log_A, em = tables(10 * K + T, B, T, K)
    if K > 1:
        log_A[1, :, 0, K - 1] = -np.inf  # one structurally impossible transition
    L = np.array([T, max(T - 2, 1), 1, 0])
    r = PR.pair_ref(log_pi, log_A, em, L)
    for b in range(B):
        n = int(L[b])
        if n == 0:
            assert np.isnan(r["loglik"][b]) and not r["filt"][b].any() and not r["xi"][b].any()
            continue
        filt, ll, gamma, xi = PR.brute_force(log_pi, log_A[b], em[b], n)
        assert abs(r["loglik"][b] - ll) <= 1e-12 * max(1.0, abs(ll))
        assert np.abs(r["filt"][b, :n] - filt).max() <= 1e-12
        assert np.abs(r["gamma"][b, :n] - gamma).max() <= 1e-12
        assert np.abs(r["xi"][b, :n] - xi).max() <= 1e-12
        assert not r["filt"][b, n:].any() and not r["xi"][b, n:].any() and not r["gamma"][b, n:].any()
        assert not r["xi"][b, 0].any()
    if K > 1:
        assert not r["xi"][1, :, 0, K - 1].any()


@pytest.mark.parametrize("K,B,T", [(3, 4, 50), (8, 3, 120), (17, 2, 40)])
def test_helper_marginals(K, B, T):
    """sum_j xi_t(i,j) = gamma_{t-1}(i), sum_i xi_t(i,j) = gamma_t(j); filt rows sum to 1; the last
    filtered row is the last smoothed row."""
    log_pi, log_A, em = tables(K + B + T, B, T, K)
    L = np.array([T, T // 2, 2, 1][:B])
    r = PR.pair_ref(log_pi, log_A, em, L)
    for b in range(B):
        n = int(L[b])
        assert np.abs(r["xi"][b, 1:n].sum(2) - r["gamma"][b, :n - 1]).max(initial=0) <= 1e-12
        assert np.abs(r["xi"][b, 1:n].sum(1) - r["gamma"][b, 1:n]).max(initial=0) <= 1e-12
        assert np.abs(r["filt"][b, :n].sum(1) - 1).max() <= 1e-12
        assert np.abs(r["filt"][b, n - 1] - r["gamma"][b, n - 1]).max() <= 1e-12


def test_helper_agrees_with_oracle_forward_backward():
    from oracle import hmm_ref
    log_pi, log_A, em = tables(5, 3, 30, 4)
    L = np.array([30, 7, 0])
    r = PR.pair_ref(log_pi, log_A, em, L)
    g, z = hmm_ref.forward_backward_f64(log_pi, log_A, em, L)
    assert np.abs(r["gamma"] - g).max() <= 1e-12
    assert np.allclose(r["logZ"][:2], z[:2], rtol=1e-13, atol=0)


def test_new_entry_points_declared_and_bound():
    from vqhmm import _ext
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(vqhmm_\w+)\s*\(", src))
    lib = _ext.load()
    for name in NEW:
        assert name in declared, name
        assert name in _ext.exported_symbols(), name
        assert hasattr(lib, name), name
    assert lib.vqhmm_abi_version() == _ext.ABI_VERSION >= 7


def test_null_pointers_rejected_without_gpu():
    from vqhmm import _ext
    lib = _ext.load()
    assert lib.vqhmm_filter_f32(None, None, None, None, 2, 8, 3, None, None, None) == -1
    assert lib.vqhmm_fwdbwd_xi_f32(None, None, None, None, 2, 8, 3, None, None, None, None, 0, None) == -1
    # host-only queries: the workspace holds the forward-backward workspace and the filter's output
    assert lib.vqhmm_fwdbwd_xi_workspace_size(2, 8, 3) >= lib.vqhmm_fwdbwd_workspace_size(2, 8, 3) + 2 * 8 * 3 * 4
    assert lib.vqhmm_fwdbwd_xi_workspace_size(2, 8, 33) == 0


def test_python_surface_exports():
    import vqhmm
    for name in ("forward_filter", "pairwise_posteriors", "filtered_regimes"):
        assert callable(getattr(vqhmm, name)) and name in vqhmm.__all__
    import torch
    with pytest.raises(RuntimeError, match="HIP"):
        vqhmm.forward_filter(torch.zeros(2), torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2))
