"""CPU checks of tests/gauss_scenario_ref.py, the reference the GPU scenario tests compare with: Philox4x32-10
against the Random123 known answers, the counter layout, the draw rule against gauss_hmm_ref._draw, Box-Muller, the
literal one-path loop against the vectorised reference, the cap on left-out paths for the GPU cases, and the
host-only return codes of vqhmm_gauss_scenario_f32 (no launch happens in any of them)."""
import ctypes

import numpy as np
import pytest

import gauss_hmm_ref as G
import gauss_scenario_ref as R
from gauss_scenario_ref import EXACT_CASES, case_inputs

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        got = R.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert " ".join("%08x" % v for v in got) == want
    # vectorised over counters and keys at once
    got = R.philox4x32_10(np.array([k[0] for k in KNOWN], np.uint64), np.array([k[1] for k in KNOWN], np.uint64))
    assert [" ".join("%08x" % v for v in row) for row in got] == [k[2] for k in KNOWN]


def test_counter_layout():
    """counter = (n, b, t, j), key = (seed low, seed high)."""
    seed = 0x299f31d0a4093822
    w = R.path_words(seed, np.array([0x85a308d3]), np.array([0x243f6a88]), 0x13198a2e, 0x03707344)
    assert " ".join("%08x" % v for v in w[0]) == KNOWN[2][2]
    # the words differ in each of the four coordinates
    base = R.path_words(5, np.array([1]), np.array([2]), 3, 0)[0]
    for other in (R.path_words(6, [1], [2], 3, 0), R.path_words(5, [2], [2], 3, 0), R.path_words(5, [1], [3], 3, 0),
                  R.path_words(5, [1], [2], 4, 0), R.path_words(5, [1], [2], 3, 1)):
        assert (np.asarray(other)[0] != base).any()


def test_uniform_and_box_muller():
    assert R.uniform_of(np.uint32(0xffffffff)) == np.float32(1 - 2.0 ** -24) and R.uniform_of(np.uint32(255)) == 0
    # u1 = 1 gives r = 0; u1 = 2^-24 the tail cut sqrt(48 ln 2) = 5.77
    e0, e1 = R.box_muller(np.uint32(0xffffffff), np.uint32(0))
    assert e0 == 0 and e1 == 0
    e0, e1 = R.box_muller(np.uint32(0), np.uint32(0))
    assert abs(e0 - np.sqrt(48 * np.log(2))) < 1e-12 and abs(e1) < 1e-12 and e0 < 5.77
    # moments of 2^16 draws: mean 0, variance 1, no correlation between the pair (5 sigma)
    w = R.path_words(7, np.zeros(1 << 14, np.uint64), np.arange(1 << 14), 0, 1)
    a, b = R.box_muller(w[:, 0], w[:, 1])
    c, d = R.box_muller(w[:, 2], w[:, 3])
    e = np.stack([a, b, c, d], 1)
    n = e.shape[0]
    assert np.abs(e.mean(0)).max() < 5 / np.sqrt(n)
    assert np.abs(e.var(0) - 1).max() < 5 * np.sqrt(2 / n)
    assert abs((e[:, 0] * e[:, 1]).mean()) < 5 / np.sqrt(n)
    assert np.array_equal(R.normals(7, np.zeros(4, np.uint64), np.arange(4), 0, 3), e[:4, :3])


def test_draw_rows_is_gauss_hmm_refs_draw():
    rng = np.random.default_rng(0)
    for S in (1, 3, 8, 32):
        lp = np.log(rng.random((50, S)) + 0.05).astype(np.float32)
        lp[rng.random((50, S)) < 0.2] = -np.inf
        lp[:, 0] = np.where(np.isinf(lp).all(1), 0.0, lp[:, 0])
        u = rng.random(50).astype(np.float32)
        u[:3] = [0.0, np.float32(1 - 2.0 ** -24), 0.5]
        k, m = R.draw_rows(np.exp(lp).astype(np.float32), u)
        for i in range(50):
            ki, mi = G._draw(lp[i], u[i])
            assert (ki, mi) == (k[i], m[i])
            assert R._draw_weights(np.exp(lp[i]).astype(np.float32), u[i]) == ki
            assert np.exp(lp[i, ki]) > 0


@pytest.mark.parametrize("kind,B,N,H,S,D", [("diag", 2, 3, 9, 1, 1), ("full", 2, 3, 12, 3, 5), ("diag", 1, 2, 7, 4, 6)])
def test_path_loop_agrees_with_vectorised(kind, B, N, H, S, D):
    c = case_inputs(kind, B, N, H, S, D)
    for reb, tx in ((1, 0.0), (5, 1e-3), (H + 3, 1e-3)):
        ref = R.scenario_ref(c["start"], c["log_A"], c["mean"], c["scale"], c["full"], c["port"], reb, tx, 11, 3, 5,
                             B, N, H)
        for b in range(B):
            for n in range(N):
                st, x, wl, fin, dd = R.scenario_path_loop(c["start"][b], c["log_A"], c["mean"], c["scale"], c["full"],
                                                          c["port"], reb, tx, 11, 3 + b, 5 + n, H)
                assert np.array_equal(st, ref["states"][b, n])
                np.testing.assert_allclose(x, ref["x"][b, n], rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(wl, ref["wealth"][b, n], rtol=1e-12)
                np.testing.assert_allclose([fin, dd], [ref["final"][b, n], ref["drawdown"][b, n]], rtol=1e-12,
                                           atol=1e-15)


def test_failed_paths_in_the_reference():
    log_A, mean, scale = R.make_case(1, 3, 2, False)
    log_A[2] = -np.inf                       # entering regime 2 fails the path at the next step
    start = np.array([[1, 0, 0], [0, 0, 0], [0.5, -1, 1], [0, 0, 2], [np.nan, 1, 1]], np.float32)
    port = R.make_port(2, 3, 2)
    ref = R.scenario_ref(start, log_A, mean, scale, False, port, 1, 0.0, 3, 0, 0, 5, 4, 6)
    assert (ref["states"][0, :, 0] == 0).all()
    for b in (1, 2, 4):
        assert (ref["states"][b] == -1).all() and np.isnan(ref["x"][b]).all() and np.isnan(ref["final"][b]).all()
    assert (ref["states"][3, :, 0] == 2).all() and (ref["states"][3, :, 1:] == -1).all()
    assert np.isfinite(ref["wealth"][3, :, 0]).all() and np.isnan(ref["wealth"][3, :, 1:]).all()
    assert np.isnan(ref["drawdown"][3]).all() and np.isfinite(ref["final"][0]).any()
    st, x, wl, fin, dd = R.scenario_path_loop(start[3], log_A, mean, scale, False, port, 1, 0.0, 3, 3, 1, 6)
    assert st.tolist() == [2, -1, -1, -1, -1, -1] and np.isnan(fin) and np.isnan(dd) and np.isnan(x[1:]).all()
    np.testing.assert_allclose(wl[0], ref["wealth"][3, 1, 0], rtol=1e-12)


@pytest.mark.parametrize("kind,B,N,H,S,D", EXACT_CASES)
def test_left_out_paths_stay_under_the_cap(kind, B, N, H, S, D):
    """The chain of each exact GPU case (the draws need no x: D = 1 here keeps this quick)."""
    c = case_inputs(kind, B, N, H, S, D)
    ref = R.scenario_ref(c["start"], c["log_A"], c["mean"][:, :1], np.ones((S, 1), np.float32), False, None, 1, 0.0,
                         1234, 0, 0, B, N, H)
    left = 1.0 - ref["keep"].mean()
    print(f"{kind} {B} {N} {H} {S} {D}: left out {int((~ref['keep']).sum())} / {B * N}")
    assert left <= R.MAX_LEFT_OUT


def test_wealth_bound_covers_a_perturbed_x():
    """wealth_bound is a bound: move x by +-xtol (worst signs) and the wealth stays inside it."""
    c = case_inputs("full", 2, 8, 40, 3, 5)
    ref = R.scenario_ref(c["start"], c["log_A"], c["mean"], c["scale"], True, c["port"], 5, 1e-3, 9, 0, 0, 2, 8, 40)
    P = 16
    st = ref["states"].reshape(P, 40)
    for sign in (1.0, -1.0):
        xp = (ref["x"] + sign * ref["xtol"]).reshape(P, 40, 5)
        wl, fin, dd, _ = R.wealth_ref(xp, st, c["port"], 5, 1e-3)
        assert (np.abs(wl - ref["wealth"].reshape(P, 40)) <= ref["wealth_tol"].reshape(P, 40)).all()
        assert (np.abs(dd - ref["drawdown"].reshape(P)) <= ref["drawdown_tol"].reshape(P)).all()


def test_host_return_codes():
    """The header's order: negative size -> EINVAL, domain -> EUNSUPPORTED, B N H == 0 -> OK without a launch, a
    null required pointer / rebalance < 1 / a counter past 2^32 -> EINVAL.  None of these reaches a launch."""
    from vqhmm import _ext
    lib = _ext.load()
    one = (ctypes.c_float * 8192)()
    p = ctypes.cast(one, ctypes.c_void_p)

    def call(start=p, log_A=p, mean=p, scale=p, full=0, port=p, reb=1, tx=0.0, seed=0, b0=0, n0=0, B=2, N=3, H=4,
             S=3, D=2, states=None, x=None, wealth=None, final=p, dd=p):
        return lib.vqhmm_gauss_scenario_f32(start, log_A, mean, scale, full, port, reb, tx, seed, b0, n0, B, N, H, S,
                                            D, states, x, wealth, final, dd, None)

    EINVAL, EUNS, OK = -1, -4, 0
    for neg in ("B", "N", "H", "S", "D", "b0", "n0"):
        assert call(**{neg: -1}) == EINVAL
    assert call(B=-1, S=99) == EINVAL                      # the negative size is seen first
    assert call(S=0) == EUNS and call(S=33) == EUNS and call(D=0) == EUNS and call(D=65) == EUNS
    assert call(full=1, D=33) == EUNS and call(full=1, S=9, D=31) == EUNS    # S D D > 8192
    assert call(H=(1 << 28) + 1) == EUNS and call(B=1 << 20, N=1 << 17) == EUNS
    assert call(S=33, B=0) == EUNS                          # the domain before the empty problem
    for empty in ("B", "N", "H"):
        assert call(**{empty: 0}, start=None, final=None, dd=None, reb=0) == OK   # nothing else is looked at
    for null in ("start", "log_A", "mean", "scale"):
        assert call(**{null: None}) == EINVAL
    assert call(final=None, dd=None) == EINVAL                                   # every output NULL
    assert call(port=None) == EINVAL and call(port=None, final=None, dd=None, wealth=p) == EINVAL
    assert call(reb=0) == EINVAL and call(reb=-5) == EINVAL
    assert call(b0=(1 << 32) - 1) == EINVAL and call(n0=(1 << 32) - 2) == EINVAL
