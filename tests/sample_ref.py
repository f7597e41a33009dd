"""numpy restatement of the regime-path samplers' draw rule (a helper for the tests, not a test).

include/vqhmm.h states the rule in fp32: weights w_i, their running sum c_i in index order, the
threshold u * c_{K-1}, the draw = the smallest i with c_i > thr.  Here the same draw is made on the
fp64 CDF c_i / c_{K-1}, and every draw reports its MARGIN: the distance |cdf_i - u| to the nearest
boundary between two states (boundaries at exactly 0 or 1 do not count: u = 0 and trailing
zero-weight states are unambiguous).  A draw whose margin clears

    BOUND(K) = (K + 8) * 2^-22

comes out the same in fp32.  Relative to the total, the kernel's c_i and thr differ from the exact
ones by: expf within 1 ulp (2^-23 on each weight, so on any partial sum of them), the product with
filt half an ulp more (2^-24), the K-term sequential fp32 sum (K - 1) * 2^-24, the threshold product
2^-24.  That is (2 + 1 + (K - 1) + 1) * 2^-24 on c_i and the same on the total that thr scales with:
below (K + 3) * 2^-23 < (K + 8) * 2^-23 on the normalised CDF, and the tests demand twice that.

The max-shift subtraction is done in fp32 as the kernel does it (so a -inf column gives NaN weights
and the draw fails, as there); exp and the product are fp64; a weight is rounded to fp32 only to
decide "w > 0".  With fix=rng a draw whose margin is below the bound has its uniform redrawn from
rng, in place, as the walk reaches it; u_used is the adjusted array the GPU then gets.
"""
import functools

import numpy as np

from hmm_pair_ref import pair_ref


def bound(K):
    return (K + 8) * 2.0 ** -22


def draw_rule(w, u):
    """w (M, K) fp64 weights (>= 0, NaN allowed), u (M,) -> (z (M,) int32, margin (M,)).
    z = -1 where the total is 0 or not finite; margin = inf there and where no boundary counts."""
    w = np.asarray(w, np.float64)
    u = np.asarray(u, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = np.cumsum(w, axis=1)
        tot = c[:, -1]
        ok = np.isfinite(tot) & (tot > 0)
        cdf = c / np.where(ok, tot, 1.0)[:, None]
        z = (cdf <= u[:, None]).sum(axis=1).astype(np.int32)
        inner = cdf[:, :-1]
        d = np.where((inner > 0) & (inner < 1), np.abs(inner - u[:, None]), np.inf)
    margin = d.min(axis=1) if d.shape[1] else np.full(len(u), np.inf)
    z = np.where(ok, np.minimum(z, w.shape[1] - 1), -1).astype(np.int32)
    return z, np.where(ok, margin, np.inf)


def _clean(W):
    """zero where the fp32 weight is not positive (NaN stays NaN, so the draw fails)"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        pos = W.astype(np.float32) > 0
    return np.where(pos | np.isnan(W), W, 0.0)


def _draw_fixed(rows, ucol, alive, K, fix):
    """draw for the alive samples; with fix, redraw the uniforms whose margin misses the bound"""
    z, mg = draw_rule(rows, ucol)
    if fix is not None:
        while True:
            bad = alive & (mg < bound(K))
            if not bad.any():
                break
            ucol[bad] = fix.random(int(bad.sum()), dtype=np.float32)
            z2, mg2 = draw_rule(rows[bad], ucol[bad])
            z[bad], mg[bad] = z2, mg2
    return np.where(alive, z, -1).astype(np.int32), np.where(alive, mg, np.inf)


def _shifted(a32, axis):
    """exp(a - max a) with the subtraction in fp32, the exponential in fp64"""
    with np.errstate(invalid="ignore", over="ignore"):
        m = a32.max(axis=axis, keepdims=True)
        d = (a32 - m).astype(np.float32)
        return np.exp(d.astype(np.float64))


def _walk(first_w, trans_rows, lengths, u32, K, backward, fix):
    B, N, T = u32.shape
    paths = np.full((B, N, T), -1, np.int32)
    margins = np.full((B, N, T), np.inf)
    u_used = np.array(u32, np.float32, copy=True)
    for b in range(B):
        L = int(min(max(int(lengths[b]), 0), T))
        if L == 0:
            continue
        order = range(L - 1, -1, -1) if backward else range(L)
        z = None
        for n, t in enumerate(order):
            ucol = u_used[b, :, t].copy()
            if n == 0:
                rows = np.broadcast_to(first_w(b, L), (N, K)).copy()
                alive = np.ones(N, bool)
            else:
                # backward: the transition t + 1 conditions on z_{t+1}; forward: transition t on z_{t-1}
                table = trans_rows(b, t + 1 if backward else t)  # [conditioning state][drawn state]
                alive = z >= 0
                rows = table[np.maximum(z, 0)]
            z, mg = _draw_fixed(rows, ucol, alive, K, fix)
            u_used[b, :, t] = ucol
            paths[b, :, t] = z
            margins[b, :, t] = mg
    return paths, u_used, margins


def ffbs_ref(filt32, log_A32, lengths, u32, fix=None):
    """-> (paths (B,N,T) int32, u_used (B,N,T) fp32, margins (B,N,T) fp64)"""
    filt32 = np.asarray(filt32, np.float32)
    log_A32 = np.asarray(log_A32, np.float32)
    K = filt32.shape[2]

    def first_w(b, L):
        return _clean(filt32[b, L - 1].astype(np.float64))

    def trans_rows(b, t):  # [j = z_t][i = z_{t-1}] = filt_{t-1}(i) exp(log_A_t(i,j) - max_i)
        e = _shifted(log_A32[b, t], 0)
        with np.errstate(invalid="ignore"):
            return _clean((filt32[b, t - 1].astype(np.float64)[:, None] * e).T)

    return _walk(first_w, trans_rows, lengths, np.asarray(u32, np.float32), K, True, fix)


def markov_ref(log_pi32, log_A32, lengths, u32, fix=None):
    """-> (paths (B,N,T) int32, u_used (B,N,T) fp32, margins (B,N,T) fp64)"""
    log_pi32 = np.asarray(log_pi32, np.float32)
    log_A32 = np.asarray(log_A32, np.float32)
    K = log_pi32.shape[0]

    def first_w(b, L):
        return _clean(_shifted(log_pi32, 0))

    def trans_rows(b, t):  # [i = z_{t-1}][j = z_t] = exp(log_A_t(i,j) - max_j)
        return _clean(_shifted(log_A32[b, t], 1))

    return _walk(first_w, trans_rows, lengths, np.asarray(u32, np.float32), K, False, fix)


# ------------------------------------------------------------------ the shared exact cases
B_CASE = 5
# (K, T, N): every K on both sides of the 4 / 8 / 16 / 32 row widths, every T across the staging
# chunks, every N across one wave, a partly filled wave and several waves
EXACT_CASES = [(1, 1, 1), (2, 2, 3), (3, 63, 64), (5, 64, 65), (8, 65, 130), (9, 130, 3), (16, 64, 1),
               (17, 65, 64), (32, 130, 130), (8, 130, 1), (32, 63, 65), (2, 130, 64)]


def case_lengths(T):
    return np.clip(np.array([T, 0, 1, 2, T - 5], np.int64), 0, T)


def log_softmax(a, axis=-1):
    a = np.asarray(a, np.float64)
    m = a.max(axis=axis, keepdims=True)
    return a - m - np.log(np.exp(a - m).sum(axis=axis, keepdims=True))


def random_tables(rng, B, T, K, scale=2.0):
    log_pi = log_softmax(rng.standard_normal(K) * scale).astype(np.float32)
    log_A = log_softmax(rng.standard_normal((B, T, K, K)) * scale).astype(np.float32)
    em = log_softmax(rng.standard_normal((B, T, K)) * scale).astype(np.float32)
    return log_pi, log_A, em


@functools.lru_cache(maxsize=None)
def exact_case(K, T, N):
    """Tables, the fp64 filter rounded to fp32, and for both walks the reference paths on fixed-up
    uniforms.  Computed once per process and shared; callers must not modify the arrays."""
    rng = np.random.default_rng(1000 * K + 10 * T + N)
    log_pi, log_A, em = random_tables(rng, B_CASE, T, K)
    lengths = case_lengths(T)
    filt = pair_ref(log_pi, log_A, em, lengths)["filt"].astype(np.float32)
    u = rng.random((B_CASE, N, T), dtype=np.float32)
    fix = np.random.default_rng(77)
    fp, fu, fm = ffbs_ref(filt, log_A, lengths, u, fix=fix)
    mp, mu, mm = markov_ref(log_pi, log_A, lengths, u, fix=fix)
    return dict(log_pi=log_pi, log_A=log_A, em=em, lengths=lengths, filt=filt,
                ffbs=(fp, fu, fm), markov=(mp, mu, mm))


@functools.lru_cache(maxsize=None)
def bulk_case():
    """One sequence, K = 3, T = 4, N = 50,000, uniforms left as drawn: the rows whose margins all
    clear the bound must agree exactly, the others are excluded (and counted)."""
    K, T, N = 3, 4, 50000
    rng = np.random.default_rng(20240607)
    log_pi, log_A, em = random_tables(rng, 1, T, K)
    lengths = np.array([T], np.int64)
    filt = pair_ref(log_pi, log_A, em, lengths)["filt"].astype(np.float32)
    u = rng.random((1, N, T), dtype=np.float32)
    fp, _, fm = ffbs_ref(filt, log_A, lengths, u)
    mp, _, mm = markov_ref(log_pi, log_A, lengths, u)
    return dict(log_pi=log_pi, log_A=log_A, lengths=lengths, filt=filt, u=u, K=K,
                ffbs=(fp, (fm >= bound(K)).all(axis=2)), markov=(mp, (mm >= bound(K)).all(axis=2)))


# ------------------------------------------------------------------ the statistics case
STAT_SHAPE = dict(B=3, T=40, K=4, N=8192)
STAT_SEED = 4242


@functools.lru_cache(maxsize=None)
def stat_case():
    B, T, K, N = (STAT_SHAPE[k] for k in "BTKN")
    rng = np.random.default_rng(STAT_SEED)
    log_pi, log_A, em = random_tables(rng, B, T, K, scale=1.0)
    lengths = np.array([T, 17, 33], np.int64)
    u = rng.random((B, N, T), dtype=np.float32)
    ref = pair_ref(log_pi, log_A, em, lengths)
    # exact forward marginals of the prior walk, fp64
    prior = np.zeros((B, T, K))
    for b in range(B):
        p = np.exp(log_softmax(log_pi.astype(np.float64)))
        for t in range(int(lengths[b])):
            if t > 0:
                p = p @ np.exp(log_softmax(log_A[b, t].astype(np.float64), axis=1))
            prior[b, t] = p
    return dict(log_pi=log_pi, log_A=log_A, em=em, lengths=lengths, u=u, gamma=ref["gamma"], filt=ref["filt"],
                prior=prior)


def freq_excess(paths, probs, lengths, nsig):
    """max over (b, t < L, k) of |freq - p| - (nsig sqrt(p (1 - p) / N) + 2 / N): <= 0 passes"""
    paths = np.asarray(paths)
    B, N, T = paths.shape
    K = probs.shape[2]
    worst = -np.inf
    for b in range(B):
        for t in range(int(lengths[b])):
            freq = np.bincount(paths[b, :, t].astype(np.int64) + 1, minlength=K + 1)[1:] / N
            p = probs[b, t]
            worst = max(worst, float((np.abs(freq - p) - (nsig * np.sqrt(p * (1 - p) / N) + 2.0 / N)).max()))
    return worst
