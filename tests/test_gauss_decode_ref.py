"""CPU checks of tests/gauss_decode_ref.py (the restatements the GPU tests of GaussianHMM's decode and filter
compare with) against enumeration over all state paths, and of the new entries' host-side surface: the symbols,
the return codes that are decided before any launch, the workspace query and the Python methods."""
import ctypes
import os
import re

import numpy as np
import pytest

import gauss_decode_ref as D
import gauss_full_ref as GF
import gauss_hmm_ref as G
from conftest import ROOT

NINF = -np.inf
NEW_SYMBOLS = ("vqhmm_gauss_viterbi_workspace_size", "vqhmm_gauss_viterbi_f32", "vqhmm_gauss_filter_f32",
               "vqhmm_gauss_full_viterbi_workspace_size", "vqhmm_gauss_full_viterbi_f32",
               "vqhmm_gauss_full_filter_f32")


def small_models():
    """(name, log_pi, log_A, em (B,L,S) fp32): diagonal and full emissions of random data, S^L <= 10^4."""
    out = []
    rng = np.random.default_rng(11)
    m = G.random_model(rng, 3, 2)
    x = G.sample_data(rng, m, 3, 7)
    out.append(("diag", m[0], m[1], G.emission_ref(m[2], m[3], x)[0].astype(np.float32)))
    m = GF.random_model(rng, 4, 3)
    x = rng.standard_normal((2, 6, 3)).astype(np.float32) * 2
    out.append(("full", m[0], m[1], GF.emission_ref(m[2], m[3], x)[0].astype(np.float32)))
    # structural zeros: a left-to-right chain
    m = G.random_model(rng, 3, 2)
    log_A = m[1].copy()
    log_A[np.tril_indices(3, -1)] = NINF
    x = G.sample_data(rng, m, 3, 7)
    out.append(("ninf", m[0], log_A, G.emission_ref(m[2], m[3], x)[0].astype(np.float32)))
    return out


@pytest.mark.parametrize("case", small_models(), ids=lambda c: c[0])
def test_viterbi_restatement_finds_the_best_path(case):
    _, log_pi, log_A, em = case
    path, score = D.viterbi_em_f32(log_pi, log_A, em)
    for b in range(em.shape[0]):
        best, _ = D.brute_best(log_pi, log_A, em[b])
        w = D.path_weight(log_pi, log_A, em[b], path[b])
        # the fp32 rule's path is optimal up to the rounding of its L sums of three terms
        tol = 8 * em.shape[1] * 2.0 ** -23 * max(1.0, abs(best))
        assert abs(w - best) <= tol and abs(float(score[b]) - best) <= tol


def test_viterbi_restatement_ties_keep_the_lowest_index():
    """States 0 and 1 identical (and 2 and 3): every tie is exact, and the lowest index must win each."""
    rng = np.random.default_rng(12)
    S, L = 4, 6
    log_pi, log_A, mean, log_var = G.random_model(rng, S, 2)
    for a in (log_pi, mean, log_var):
        a[1], a[3] = a[0], a[2]
    log_A[1], log_A[3] = log_A[0], log_A[2]
    log_A[:, 1], log_A[:, 3] = log_A[:, 0], log_A[:, 2]
    x = rng.standard_normal((2, L, 2)).astype(np.float32) * 2
    em = G.emission_ref(mean, log_var, x)[0].astype(np.float32)
    path, score = D.viterbi_em_f32(log_pi, log_A, em)
    assert np.isin(path, (0, 2)).all()
    for b in range(2):
        best, arg = D.brute_best(log_pi, log_A, em[b])
        assert np.isin(arg, (0, 2)).all()
        assert abs(D.path_weight(log_pi, log_A, em[b], path[b]) - best) <= 1e-4


def test_viterbi_restatement_conventions():
    rng = np.random.default_rng(13)
    log_pi, log_A, mean, log_var = G.random_model(rng, 3, 2)
    x = rng.standard_normal((4, 5, 2)).astype(np.float32)
    L = np.array([5, 0, 3, 4])
    em = G.emission_ref(mean, log_var, x, L)[0].astype(np.float32)
    em[2, 1, 0] = np.nan            # inside the length
    em[3, 4, :] = np.inf            # past the length
    log_pi = log_pi.copy()
    path, score = D.viterbi_em_f32(log_pi, log_A, em, L)
    assert (path[1] == -1).all() and score[1] == NINF
    assert (path[2] == -1).all() and np.isnan(score[2])
    assert (path[0] >= 0).all() and (path[3, :4] >= 0).all() and path[3, 4] == -1 and np.isfinite(score[[0, 3]]).all()
    # an impossible sequence: score -inf and the path of the tie rule
    dead = np.full((3, 3), NINF, np.float32)
    p2, s2 = D.viterbi_em_f32(log_pi, dead, em[:1], L[:1])
    assert s2[0] == NINF and (p2[0] == 0).all()


@pytest.mark.parametrize("with_prev", (False, True))
@pytest.mark.parametrize("case", small_models(), ids=lambda c: c[0])
def test_filter_restatement_against_enumeration(case, with_prev):
    _, log_pi, log_A, em = case
    B, L, S = em.shape
    prev = np.random.default_rng(14).random((B, S)) * 3 if with_prev else None
    ref = D.filter_em_ref(log_pi, log_A, em, prev=prev)
    for b in range(B):
        filt, ll = D.brute_filter(log_pi, log_A, em[b], None if prev is None else prev[b])
        assert np.abs(ref["filt"][b] - filt).max() <= 1e-12
        assert abs(ref["loglik"][b] - ll) <= 1e-10 * max(1.0, abs(ll))
        assert np.array_equal(ref["last"][b], ref["filt"][b, L - 1])
    assert np.abs(ref["filt"].sum(-1) - 1).max() <= 1e-12


@pytest.mark.parametrize("split", (1, 3, 6))
def test_filter_restatement_chunked_equals_the_single_call(split):
    rng = np.random.default_rng(15)
    log_pi, log_A, mean, log_var = G.random_model(rng, 5, 3)
    B, T = 4, 9
    x = G.sample_data(rng, (log_pi, log_A, mean, log_var), B, T)
    L = np.array([T, 0, 2, 7])
    em = G.emission_ref(mean, log_var, x)[0]
    whole = D.filter_em_ref(log_pi, log_A, em, L)
    a = D.filter_em_ref(log_pi, log_A, em[:, :split], np.minimum(L, split))
    b = D.filter_em_ref(None, log_A, em[:, split:], np.maximum(L - split, 0), prev=a["last"])
    assert np.abs(np.concatenate([a["filt"], b["filt"]], 1) - whole["filt"]).max() <= 1e-12
    assert np.abs(b["last"] - whole["last"]).max() <= 1e-12
    tot = np.nansum(np.stack([a["loglik"], b["loglik"]]), 0)
    live = L > 0
    assert np.abs(tot[live] - whole["loglik"][live]).max() <= 1e-12 * np.abs(whole["loglik"][live]).max()
    assert np.isnan(whole["loglik"][1]) and not whole["last"][1].any()


def test_filter_restatement_conventions():
    rng = np.random.default_rng(16)
    log_pi, log_A, mean, log_var = G.random_model(rng, 3, 2)
    x = rng.standard_normal((5, 6, 2)).astype(np.float32)
    L = np.array([6, 0, 5, 6, 6])
    em = G.emission_ref(mean, log_var, x, L)[0]
    em[2, 3, 1] = NINF               # a non-finite emission at t = 3
    log_A = log_A.copy()
    prev = rng.random((5, 3)) + 0.1
    prev[3] = 0                      # a dead carry
    prev[4, 0] = np.inf              # and one whose sum is not finite
    ref = D.filter_em_ref(log_pi, log_A, em, L, prev=prev)
    assert np.isnan(ref["loglik"][1]) and np.array_equal(ref["last"][1], prev[1]) and not ref["filt"][1].any()
    assert np.isnan(ref["loglik"][2]) and ref["filt"][2, :3].any(-1).all() and not ref["filt"][2, 3:].any()
    assert not ref["last"][2].any()
    for b in (3, 4):
        assert ref["loglik"][b] == NINF and not ref["filt"][b].any() and not ref["last"][b].any()
    assert np.isfinite(ref["loglik"][0])
    # mass truly 0 at t = 1: every transition is forbidden
    dead = np.full((3, 3), NINF)
    r2 = D.filter_em_ref(log_pi, dead, em[:1], L[:1])
    assert r2["loglik"][0] == NINF and r2["filt"][0, 0].any() and not r2["filt"][0, 1:].any()


# ------------------------------------------------------------------------------ the host-side surface
def test_new_symbols_declared_exported_and_bound():
    from vqhmm import _ext
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vqhmm.h")).read(), flags=re.S)
    lib = _ext.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _ext.exported_symbols(), name
    assert lib.vqhmm_abi_version() == _ext.ABI_VERSION == 8


def _entries(lib):
    """(viterbi, filter, query, an unsupported (S, D) list) per covariance type; every pointer is a host buffer
    that no call here reaches."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30

    def make(vit_fn, fil_fn):
        def vit(B=2, T=3, S=2, D=4, holes=(), ws=big):
            args = [p, p, p, p, p, p, B, T, S, D, p, p, p, ws, None]
            for h in holes:
                args[h] = None
            return vit_fn(*args)

        def fil(B=2, T=3, S=2, D=4, holes=(), ws=None):
            args = [p, p, p, p, p, p, p, B, T, S, D, p, p, p, None]
            for h in holes:
                args[h] = None
            return fil_fn(*args)
        return vit, fil

    diag = make(lib.vqhmm_gauss_viterbi_f32, lib.vqhmm_gauss_filter_f32)
    full = make(lib.vqhmm_gauss_full_viterbi_f32, lib.vqhmm_gauss_full_filter_f32)
    return ((*diag, lib.vqhmm_gauss_viterbi_workspace_size, ((33, 4), (2, 65), (0, 4), (2, 0))),
            (*full, lib.vqhmm_gauss_full_viterbi_workspace_size, ((33, 4), (2, 33), (32, 17), (9, 31), (0, 4), (2, 0))))


def test_return_codes_on_the_host():
    """The order of include/vqhmm.h: a negative size, an unsupported S / D or batch, B = 0, then a null required
    pointer or a short workspace -> VQHMM_EINVAL.  Nothing here launches."""
    from vqhmm import _ext
    lib = _ext.load()
    for vit, fil, query, unsupported in _entries(lib):
        for f in (vit, fil):
            assert f(B=-1, S=33) == -1 and f(T=-1, D=65) == -1 and f(S=-1) == -1 and f(D=-1) == -1
            for S, Dm in unsupported:
                assert f(S=S, D=Dm) == -4, (S, Dm)
                assert query(4, 16, S, Dm) == 0
            assert f(S=33, holes=(0, 1, 2)) == -4          # the size first, then the pointers
            assert f(T=(1 << 28) + 1) == -4 and f(B=1 << 31) == -4 and f(B=1 << 20, T=(1 << 20) + 1) == -4
            assert f(B=0, holes=(0, 1, 2, 3, 4, 5)) == 0 and f(B=0, T=0) == 0
        for hole in (0, 1, 2, 3, 4, 5, 10, 11, 12):
            assert vit(holes=(hole,)) == -1, hole
        for hole in (1, 2, 3, 4, 5):
            assert fil(holes=(hole,)) == -1, hole
        assert fil(holes=(0, 6)) == -1                      # log_pi is required without prev
        need = query(2, 3, 2, 4)
        assert need > 0 and vit(ws=need - 1) == -1 and vit(ws=0) == -1


def test_workspace_query():
    from vqhmm import _ext
    lib = _ext.load()
    for q in (lib.vqhmm_gauss_viterbi_workspace_size, lib.vqhmm_gauss_full_viterbi_workspace_size):
        assert q(-1, 16, 8, 8) == 0 and q(4, -1, 8, 8) == 0
        assert q(1, (1 << 28) + 1, 8, 8) == 0 and q(1 << 31, 1, 8, 8) == 0 and q(1 << 20, (1 << 20) + 1, 8, 8) == 0
        # one backpointer byte per step (rounded up to four) and padded state, rounded up to 256
        for B, T, S, SP in ((1024, 512, 8, 8), (3, 5, 9, 16), (7, 130, 32, 32), (2, 1, 1, 1)):
            need = B * 4 * ((T + 3) // 4) * SP
            assert need <= q(B, T, S, 8) < need + 256
    assert lib.vqhmm_gauss_viterbi_workspace_size(4, 16, 32, 64) > 0
    assert lib.vqhmm_gauss_full_viterbi_workspace_size(4, 16, 8, 32) > 0


@pytest.mark.parametrize("cov", ("diag", "full"))
def test_python_surface_and_cpu_refusal(cov):
    import torch
    import vqhmm
    hmm = vqhmm.GaussianHMM(3, 2, covariance_type=cov)
    for name in ("decode", "filter", "update", "predict_next"):
        assert callable(getattr(hmm, name))
    x = torch.zeros((2, 4, 2))
    with pytest.raises(RuntimeError, match="HIP"):
        hmm.decode(x)
    with pytest.raises(RuntimeError, match="HIP"):
        hmm.filter(x)
    with pytest.raises(RuntimeError, match="HIP"):
        hmm.update(x)
    with pytest.raises(RuntimeError, match="HIP"):
        hmm.predict_next(torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        hmm.predict_next(torch.zeros((2, 4)))
    with pytest.raises(ValueError):
        hmm.predict_next(torch.zeros((2, 3), dtype=torch.float64))
