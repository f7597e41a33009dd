"""CPU checks of CodeHMM's decode / filter helpers (tests/code_decode_ref.py): the fp32 Viterbi restatement and
the fp64 filter against enumeration of the S^L paths, the filter's chunking identity, and the C-ABI's
host-side behaviour for the four new entry points.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import code_decode_ref as D
import code_hmm_ref as R
from conftest import ROOT

NINF = -np.inf
NEW_SYMBOLS = ("vqhmm_code_viterbi_workspace_size", "vqhmm_code_viterbi_f32",
               "vqhmm_code_filter_workspace_size", "vqhmm_code_filter_f32")


def _model(S, V, seed, holes=True):
    rng = np.random.default_rng(seed)
    log_pi, log_A, log_B = R.random_model(rng, S, V)
    if holes and S >= 2:
        log_A[0, 1] = NINF   # a structural zero transition
        log_B[1, 0] = NINF   # ... and emission
    return rng, log_pi, log_A, log_B


@pytest.mark.parametrize("S,V,L", [(1, 1, 3), (1, 3, 6), (2, 3, 6), (2, 2, 1), (3, 5, 6), (3, 2, 4)])
def test_viterbi_matches_brute_force(S, V, L):
    rng, log_pi, log_A, log_B = _model(S, V, 7 * S + V + L)
    B = 6
    codes = rng.integers(0, V, size=(B, L))
    path, score = D.viterbi_f32(log_pi, log_A, log_B, codes)
    for b in range(B):
        best = D.brute_best(log_pi, log_A, log_B, codes[b])
        if best == NINF:
            assert score[b] == NINF
            continue
        assert abs(float(score[b]) - best) <= 1e-5 * max(1.0, abs(best))
        assert (path[b] >= 0).all() and (path[b] < S).all()
        own = D.path_weight(log_pi, log_A, log_B, codes[b], path[b])
        assert abs(own - best) <= 1e-4, (own, best)


def test_viterbi_conventions():
    _, log_pi, log_A, log_B = _model(3, 4, 5)
    codes = np.array([[1, 2, 3, 0], [1, 2, 3, 0], [1, 9, 3, 0], [1, 2, 9, 0], [0, 0, 0, 0]])
    path, score = D.viterbi_f32(log_pi, log_A, log_B, codes, [4, 0, 4, 2, 9])
    assert (path[0] >= 0).all() and np.isfinite(score[0])
    assert (path[1] == -1).all() and score[1] == NINF
    assert (path[2] == -1).all() and np.isnan(score[2])          # a bad code inside the length
    assert (path[3, :2] >= 0).all() and (path[3, 2:] == -1).all()  # ... and past it: never looked at
    short = D.viterbi_f32(log_pi, log_A, log_B, codes[3:4, :2])
    assert np.array_equal(path[3, :2], short[0][0]) and score[3] == short[1][0]
    assert (path[4] >= 0).all()                                   # lengths clamp to T
    # ties keep the lowest index: an all-equal model decodes to state 0 throughout
    z = np.zeros
    path, score = D.viterbi_f32(z(3, np.float32), z((3, 3), np.float32), z((3, 2), np.float32), z((1, 5), np.int64))
    assert not path.any() and score[0] == 0
    # an impossible sequence: score -inf, the path of the tie rule
    imp = np.full((2, 2), NINF, np.float32)
    path, score = D.viterbi_f32(z(2, np.float32), z((2, 2), np.float32), imp, z((1, 3), np.int64))
    assert score[0] == NINF and not path.any()


@pytest.mark.parametrize("S,V,L", [(1, 2, 4), (2, 3, 6), (3, 4, 5)])
def test_filter_matches_brute_force_prefix_marginals(S, V, L):
    rng, log_pi, log_A, log_B = _model(S, V, 13 * S + V)
    codes = rng.integers(0, V, size=(4, L))
    got = D.filter_ref(log_pi, log_A, log_B, codes)
    for b in range(4):
        filt, ll = D.brute_filter(log_pi, log_A, log_B, codes[b])
        if not np.isfinite(ll):
            assert got["loglik"][b] == NINF
            continue
        assert np.abs(got["filt"][b] - filt).max() <= 1e-12
        assert abs(got["loglik"][b] - ll) <= 1e-12
        assert np.abs(got["last"][b] - filt[-1]).max() <= 1e-12
    # the filter's loglik is the E-step's
    ref = R.estep_ref(log_pi, log_A, log_B, codes)
    ok = np.isfinite(ref["loglik"])
    assert np.abs(got["loglik"][ok] - ref["loglik"][ok]).max(initial=0) <= 1e-12
    # smoothed = filtered at the last position
    assert np.abs(got["last"][ok] - ref["gamma"][ok, L - 1]).max(initial=0) <= 1e-12


@pytest.mark.parametrize("split", (1, 3, 6))
def test_filter_chunking_identity(split):
    S, V, T, B = 3, 5, 7, 6
    rng, log_pi, log_A, log_B = _model(S, V, 3)
    codes = rng.integers(1, V, size=(B, T))
    L = np.array([T, 0, 1, 2, 4, 6])
    whole = D.filter_ref(log_pi, log_A, log_B, codes, L)
    L1, L2 = np.minimum(L, split), np.maximum(L - split, 0)
    a = D.filter_ref(log_pi, log_A, log_B, codes[:, :split], L1)
    b = D.filter_ref(log_pi, log_A, log_B, codes[:, split:], L2, prev=a["last"])
    assert np.abs(np.concatenate([a["filt"], b["filt"]], 1) - whole["filt"]).max() <= 1e-12
    assert np.abs(b["last"] - whole["last"]).max() <= 1e-12
    tot = np.nansum(np.stack([a["loglik"], b["loglik"]]), 0)
    live = L > 0
    assert np.abs(tot[live] - whole["loglik"][live]).max() <= 1e-12
    # an unnormalised carry is the same carry
    b3 = D.filter_ref(log_pi, log_A, log_B, codes[:, split:], L2, prev=3.0 * a["last"])
    assert np.abs(b3["filt"] - b["filt"]).max() <= 1e-12


def test_filter_conventions():
    _, log_pi, log_A, log_B = _model(2, 3, 9, holes=False)
    codes = np.array([[1, 2, 7, 0], [1, 2, 0, 0], [1, 2, 0, 0]])
    prev = np.array([[0.5, 0.5], [0.25, 0.75], [0.0, 0.0]])
    got = D.filter_ref(log_pi, log_A, log_B, codes, [4, 0, 3], prev=prev)
    assert np.isnan(got["loglik"][0]) and got["filt"][0, :2].all() and not got["filt"][0, 2:].any()
    assert not got["last"][0].any()
    assert np.isnan(got["loglik"][1]) and np.array_equal(got["last"][1], prev[1]) and not got["filt"][1].any()
    assert got["loglik"][2] == NINF and not got["filt"][2].any() and not got["last"][2].any()
    got = D.filter_ref(log_pi, log_A, log_B, codes, [2, 0, 3])
    assert np.isfinite(got["loglik"][0]) and not got["last"][1].any() and np.isnan(got["loglik"][1])


def test_new_symbols_declared_exported_and_bound():
    from vqhmm import _ext
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vqhmm.h")).read(), flags=re.S)
    lib = _ext.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _ext.exported_symbols(), name
    assert lib.vqhmm_abi_version() == _ext.ABI_VERSION == 8


def test_return_codes_on_the_host():
    """The order of include/vqhmm.h: negative size, unsupported S / V, (T = 0 and B = 0 need no pointer,) then a
    null required pointer or a short workspace -> VQHMM_EINVAL.  Nothing here launches."""
    from vqhmm import _ext
    lib = _ext.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30

    def vit(B=2, T=3, S=2, V=4, holes=(), ws=big):
        args = [p, p, p, p, p, B, T, S, V, p, p, p, ws, None]
        for h in holes:
            args[h] = None
        return lib.vqhmm_code_viterbi_f32(*args)

    def fil(B=2, T=3, S=2, V=4, holes=(), ws=big):
        args = [p, p, p, p, p, p, B, T, S, V, p, p, p, p, ws, None]
        for h in holes:
            args[h] = None
        return lib.vqhmm_code_filter_f32(*args)

    for f in (vit, fil):
        assert f(B=-1, S=33) == -1 and f(T=-1, V=65537) == -1 and f(S=-1) == -1 and f(V=-1) == -1
        assert f(S=33) == -4 and f(V=65537) == -4 and f(S=0) == -4 and f(V=0) == -4
        assert f(S=33, holes=(0, 1, 2)) == -4          # the size first, then the pointers
        assert f(B=0, holes=(0, 1, 2, 3, 4)) == 0 and f(B=0, T=0) == 0
    for hole in (0, 1, 2, 3, 4, 9, 10, 11):
        assert vit(holes=(hole,)) == -1, hole
    for hole in (1, 2, 3, 4, 13):
        assert fil(holes=(hole,)) == -1, hole
    assert fil(holes=(0, 5)) == -1                      # log_pi is required without prev
    need = lib.vqhmm_code_viterbi_workspace_size(2, 3, 2, 4)
    assert need > 0 and vit(ws=need - 1) == -1
    need = lib.vqhmm_code_filter_workspace_size(2, 3, 2, 4)
    assert need > 0 and fil(ws=need - 1) == -1


def test_workspace_query_limits():
    from vqhmm import _ext
    lib = _ext.load()
    for q in (lib.vqhmm_code_viterbi_workspace_size, lib.vqhmm_code_filter_workspace_size):
        assert q(4, 16, 32, 65536) > 0
        assert q(4, 16, 33, 8) == 0 and q(4, 16, 8, 65537) == 0 and q(4, 16, 0, 8) == 0 and q(4, 16, 8, 0) == 0
        assert q(-1, 16, 8, 8) == 0 and q(4, -1, 8, 8) == 0
    # one backpointer byte per step and padded state, plus the table; the filter only the table
    B, T, S, V = 1024, 512, 8, 512
    assert B * T * 8 <= lib.vqhmm_code_viterbi_workspace_size(B, T, S, V) <= B * T * 8 + S * V * 4 + 512
    assert lib.vqhmm_code_filter_workspace_size(B, T, S, V) <= S * V * 4 + 256


def test_python_surface_and_cpu_refusal():
    import torch
    import vqhmm
    hmm = vqhmm.CodeHMM(3, 5)
    for name in ("decode", "filter", "update", "predict_next"):
        assert callable(getattr(hmm, name))
    codes = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP"):
        hmm.decode(codes)
    with pytest.raises(RuntimeError, match="HIP"):
        hmm.filter(codes)
    with pytest.raises(RuntimeError, match="HIP"):
        hmm.predict_next(torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        hmm.predict_next(torch.zeros((2, 4)))
    with pytest.raises(ValueError):
        hmm.predict_next(torch.zeros((2, 3), dtype=torch.float64))
