"""CPU checks of the code-index HMM: the fp64 helper (tests/code_hmm_ref.py) against brute force and
against tests/hmm_pair_ref.py, the counts' identities, the M-step, the C-ABI's host-side behaviour,
the Python surface, and the margins of the sampler test's uniforms.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import code_hmm_ref as R
from conftest import ROOT
from hmm_pair_ref import pair_ref

NINF = -np.inf
NEW_SYMBOLS = ("vqhmm_code_estep_workspace_size", "vqhmm_code_estep_f32", "vqhmm_code_sample_f32")


def _brute_model(S, V, seed):
    rng = np.random.default_rng(seed)
    log_pi, log_A, log_B = (a.astype(np.float64) for a in R.random_model(rng, S, V))
    if S >= 2:
        log_A[0, 1] = NINF   # a structural zero transition
        log_B[1, 0] = NINF   # ... and emission
    return rng, log_pi, log_A, log_B


@pytest.mark.parametrize("S,V,L", [(1, 1, 3), (2, 3, 6), (3, 5, 6), (4, 2, 5)])
def test_helper_matches_brute_force(S, V, L):
    rng, log_pi, log_A, log_B = _brute_model(S, V, 11 * S + V)
    seqs = [rng.integers(0, V, size=n) for n in (L, L, 1, 0)]
    if S >= 2:
        # an impossible sequence: only state 0 can emit code 0 twice running, and 0 -> 0 is closed too
        imp_B = log_B.copy()
        imp_B[1:, 0] = NINF
        imp_A = log_A.copy()
        imp_A[0, 0] = NINF
        bf = R.brute_force(log_pi, imp_A, imp_B, [0, 0])
        assert bf["loglik"] == NINF
        got = R.estep_ref(log_pi, imp_A, imp_B, np.zeros((1, 2), np.int64))
        assert got["loglik"][0] == NINF
        for k in ("pi_cnt", "trans_cnt", "emit_cnt", "gamma"):
            assert not got[k].any()
    for c in seqs:
        n = len(c)
        codes = np.zeros((1, L), np.int64)
        codes[0, :n] = c
        codes[0, n:] = -1  # never looked at
        got = R.estep_ref(log_pi, log_A, log_B, codes, [n])
        bf = R.brute_force(log_pi, log_A, log_B, c)
        if n == 0:
            assert np.isnan(got["loglik"][0]) and np.isnan(bf["loglik"])
        else:
            assert abs(got["loglik"][0] - bf["loglik"]) <= 1e-12
        for k in ("pi_cnt", "trans_cnt", "emit_cnt"):
            assert np.abs(got[k] - bf[k]).max() <= 1e-12, k
        assert np.abs(got["gamma"][0, :n] - bf["gamma"]).max(initial=0.0) <= 1e-12
        assert not got["gamma"][0, n:].any()


def test_helper_matches_pair_ref_on_broadcast_tables():
    rng = np.random.default_rng(5)
    S, V, B, T = 4, 6, 5, 12
    log_pi, log_A, log_B = R.random_model(rng, S, V)
    log_A[2, 1] = NINF
    codes = rng.integers(0, V, size=(B, T))
    lengths = np.array([T, 0, 1, 2, 7])
    got = R.estep_ref(log_pi, log_A, log_B, codes, lengths)
    em = np.asarray(log_B, np.float64)[:, codes].transpose(1, 2, 0)
    ref = pair_ref(log_pi, np.broadcast_to(np.asarray(log_A, np.float64), (B, T, S, S)), em, lengths)
    assert np.abs(got["gamma"] - ref["gamma"]).max() <= 1e-10
    assert np.allclose(got["loglik"], ref["loglik"], rtol=0, atol=1e-10, equal_nan=True)
    assert np.abs(got["trans_cnt"] - ref["xi"].sum((0, 1))).max() <= 1e-10
    assert np.abs(got["pi_cnt"] - ref["gamma"][:, 0].sum(0)).max() <= 1e-10
    emit = np.zeros((S, V))
    for b in range(B):
        for t in range(int(lengths[b])):
            emit[:, codes[b, t]] += ref["gamma"][b, t]
    assert np.abs(got["emit_cnt"] - emit).max() <= 1e-10
    # identities of the counts
    assert abs(got["trans_cnt"].sum() - np.maximum(lengths - 1, 0).sum()) <= 1e-9
    assert abs(got["emit_cnt"].sum() - lengths.sum()) <= 1e-9
    assert np.abs(got["emit_cnt"].sum(1) - got["gamma"].sum((0, 1))).max() <= 1e-9
    assert got["trans_cnt"][2, 1] == 0.0


def test_mstep_keeps_zero_rows_and_structural_zeros():
    rng = np.random.default_rng(9)
    S, V = 3, 4
    log_pi, log_A, log_B = (a.astype(np.float64) for a in R.random_model(rng, S, V))
    log_A[0, 2] = NINF
    log_B[1, 3] = NINF
    counts = dict(pi_cnt=rng.random(S), trans_cnt=rng.random((S, S)), emit_cnt=rng.random((S, V)))
    counts["trans_cnt"][1] = 0.0       # nothing counted into row 1
    counts["trans_cnt"][0, 2] = 0.0
    counts["emit_cnt"][1, 3] = 0.0
    npi, nA, nB = R.mstep_ref(counts, log_pi, log_A, log_B)
    assert np.array_equal(nA[1], log_A[1])
    assert nA[0, 2] == NINF and nB[1, 3] == NINF
    for m in (npi[None], nA[[0, 2]], nB):
        assert np.abs(np.exp(m).sum(-1) - 1).max() <= 1e-12
    assert np.allclose(np.exp(nB[0]), counts["emit_cnt"][0] / counts["emit_cnt"][0].sum())
    # the prior count reaches every entry but the structural zeros, and revives the empty row
    _, pA, pB = R.mstep_ref(counts, log_pi, log_A, log_B, prior_count=0.5)
    assert pA[0, 2] == NINF and pB[1, 3] == NINF
    assert np.allclose(np.exp(pA[1]), 1.0 / S)
    assert np.allclose(np.exp(pA[0, :2]), (counts["trans_cnt"][0, :2] + 0.5) / (counts["trans_cnt"][0, :2] + 0.5).sum())


def test_mstep_of_the_package_matches_the_helper():
    import torch
    import vqhmm
    rng = np.random.default_rng(3)
    S, V = 3, 5
    hmm = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        hmm.log_A[0, 2] = float("-inf")
        hmm.log_B[1, 3] = float("-inf")
    old = [hmm.log_pi.numpy().copy(), hmm.log_A.numpy().copy(), hmm.log_B.numpy().copy()]
    for m in old:
        assert np.abs(np.exp(m[np.isfinite(m).all(-1)].astype(np.float64)).sum(-1) - 1).max() <= 1e-6
    counts = dict(pi_cnt=rng.random(S), trans_cnt=rng.random((S, S)), emit_cnt=rng.random((S, V)))
    counts["trans_cnt"][1] = 0.0
    for pc in (0.0, 0.25):
        hmm.load_state_dict({"log_pi": torch.tensor(old[0]), "log_A": torch.tensor(old[1]), "log_B": torch.tensor(old[2])})
        hmm.m_step({k: torch.tensor(v) for k, v in counts.items()}, prior_count=pc)
        ref = R.mstep_ref(counts, *old, prior_count=pc)
        for got, want in zip((hmm.log_pi, hmm.log_A, hmm.log_B), ref):
            assert np.allclose(got.numpy(), want, rtol=0, atol=1e-6)
            assert np.array_equal(np.isinf(got.numpy()), np.isinf(want))


def test_new_symbols_declared_exported_and_bound():
    from vqhmm import _ext
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vqhmm.h")).read(), flags=re.S)
    lib = _ext.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _ext.exported_symbols(), name
    assert lib.vqhmm_abi_version() == 8


def test_null_pointers_rejected_without_gpu():
    from vqhmm import _ext
    lib = _ext.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.vqhmm_code_estep_f32(None, None, None, None, None, 2, 3, 2, 4, None, None, None, None, None, None, 0,
                                    None) == -1
    # every required pointer on its own (loglik and gamma are nullable; the workspace is a size matter)
    for hole in (0, 1, 2, 3, 4, 9, 10, 11):
        args = [p, p, p, p, p, 2, 3, 2, 4, p, p, p, None, None, p, 1 << 20, None]
        args[hole] = None
        assert lib.vqhmm_code_estep_f32(*args) == -1, hole
    assert lib.vqhmm_code_sample_f32(None, None, None, None, 2, 3, 2, 4, None, None, None) == -1
    for hole in (0, 1, 2, 3, 8, 9):
        args = [p, p, p, p, 2, 3, 2, 4, p, p, None]
        args[hole] = None
        assert lib.vqhmm_code_sample_f32(*args) == -1, hole
    # unsupported sizes and a short workspace are refused on the host too
    assert lib.vqhmm_code_estep_f32(p, p, p, p, p, 2, 3, 33, 4, p, p, p, None, None, p, 1 << 20, None) == -4
    assert lib.vqhmm_code_sample_f32(p, p, p, p, 2, 3, 2, 65537, p, p, None) == -4
    need = lib.vqhmm_code_estep_workspace_size(2, 3, 2, 4)
    assert need > 0
    assert lib.vqhmm_code_estep_f32(p, p, p, p, p, 2, 3, 2, 4, p, p, p, None, None, p, need - 1, None) == -3


def test_workspace_query_limits():
    from vqhmm import _ext
    lib = _ext.load()
    assert lib.vqhmm_code_estep_workspace_size(4, 16, 32, 65536) > 0
    assert lib.vqhmm_code_estep_workspace_size(4, 16, 33, 8) == 0
    assert lib.vqhmm_code_estep_workspace_size(4, 16, 8, 65537) == 0
    assert lib.vqhmm_code_estep_workspace_size(4, 16, 0, 8) == 0
    assert lib.vqhmm_code_estep_workspace_size(4, 16, 8, 0) == 0
    # at least the scaled forward vectors
    assert lib.vqhmm_code_estep_workspace_size(1024, 512, 8, 512) >= 1024 * 512 * 8 * 4


def test_python_surface_and_cpu_refusal():
    import torch
    import vqhmm
    assert "CodeHMM" in vqhmm.__all__
    for m in ("e_step", "log_prob", "posterior", "m_step", "fit", "sample"):
        assert callable(getattr(vqhmm.CodeHMM, m))
    hmm = vqhmm.CodeHMM(3, 5, generator=torch.Generator().manual_seed(1))
    assert hmm.log_pi.shape == (3,) and hmm.log_A.shape == (3, 3) and hmm.log_B.shape == (3, 5)
    assert set(hmm.state_dict()) == {"log_pi", "log_A", "log_B"}
    other = vqhmm.CodeHMM(3, 5, generator=torch.Generator().manual_seed(2))
    assert not torch.equal(other.log_B, hmm.log_B)
    other.load_state_dict(hmm.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), hmm.state_dict().values()))
    codes = torch.zeros(2, 4, dtype=torch.int64)
    for call in (lambda: hmm.e_step(codes), lambda: hmm.log_prob(codes), lambda: hmm.posterior(codes),
                 lambda: hmm.fit(codes, n_iter=1), lambda: hmm.sample(2, 3)):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    with pytest.raises(ValueError):
        vqhmm.CodeHMM(33, 5)
    with pytest.raises(ValueError):
        vqhmm.CodeHMM(3, 65537)


@pytest.mark.parametrize("S,V,seed", R.SAMPLER_CASES)
def test_sampler_uniforms_keep_their_distance(S, V, seed):
    """The GPU test demands exact equality with nothing excluded, so its uniforms must not sit on a CDF
    boundary: every draw along the reference path is at least (n + 4) 2^-23 from the nearest one, n the
    draw's number of categories (twice the sequential fp32 sum's error bound, n 2^-24 relative to a CDF
    <= 1, plus a few ulp for exp)."""
    log_pi, log_A, log_B, u = R.sampler_case(S, V, seed)
    assert u.shape == (R.SAMPLER_N, R.SAMPLER_T, 2) and u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    states, codes, margins = R.sample_ref(log_pi, log_A, log_B, u)
    assert margins[..., 0].min() >= (S + 4) * 2.0 ** -23
    assert margins[..., 1].min() >= (V + 4) * 2.0 ** -23
    assert states.min() >= 0 and states.max() < S and codes.min() >= 0 and codes.max() < V


def test_sampler_helper_rule():
    lp = np.log(np.array([0.0, 0.25, 0.0, 0.75, 0.0], np.float32), where=np.array([0, 1, 0, 1, 0], bool),
                out=np.full(5, NINF, np.float32))
    assert R._draw(lp, 0.0)[0] == 1
    assert R._draw(lp, 0.2499)[0] == 1
    assert R._draw(lp, 0.25)[0] == 3
    assert R._draw(lp, np.nextafter(np.float32(1), np.float32(0)))[0] == 3
    assert R._draw(lp, 1.0)[0] == 3  # no k with u < cdf_k: the last k with p_k > 0
    ps, pc = R.state_marginals(*R.random_model(np.random.default_rng(0), 3, 4), 5)
    assert np.allclose(ps.sum(1), 1) and np.allclose(pc.sum(1), 1)
