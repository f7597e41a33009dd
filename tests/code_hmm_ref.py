"""fp64 numpy restatement of the stationary discrete HMM on code indices (a helper for the tests,
not a test): the Baum-Welch E-step in log space, a brute-force enumeration, the M-step and the
inverse-CDF sampler of include/vqhmm.h.

    log_pi (S), log_A (S,S) rows = from-state, log_B (S,V);  codes (B,T) int, lengths (B)
    alpha_0(j) = log_pi(j) + log_B(j, c_0),  alpha_t(j) = lse_i(alpha_{t-1}(i) + log_A(i,j)) + log_B(j, c_t)
    beta_{L-1} = 0,  beta_{t-1}(i) = lse_j(log_A(i,j) + log_B(j, c_t) + beta_t(j))
    loglik = lse_j alpha_{L-1}(j),  gamma_t = exp(alpha_t + beta_t - loglik)
    xi_t(i,j) = exp(alpha_{t-1}(i) + log_A(i,j) + log_B(j, c_t) + beta_t(j) - loglik)     (1 <= t < L)
    pi_cnt = sum_b gamma_0,  trans_cnt = sum_{b,t} xi_t,  emit_cnt[s,v] = sum_{b,t: c_t = v} gamma_t(s)

Conventions of include/vqhmm.h: a length-0 sequence has loglik = NaN; an impossible sequence has
loglik = -inf and a sequence with a code outside [0, V) inside its length has loglik = NaN; all three
contribute nothing to the counts and have zero gamma rows; codes at t >= length are not looked at.
"""
import itertools

import numpy as np

from hmm_pair_ref import lse


def estep_ref(log_pi, log_A, log_B, codes, lengths=None):
    """-> dict(pi_cnt (S), trans_cnt (S,S), emit_cnt (S,V), loglik (B), gamma (B,T,S)), all float64."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    log_B = np.asarray(log_B, np.float64)
    codes = np.asarray(codes)
    B, T = codes.shape
    S, V = log_B.shape
    lengths = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    pi_cnt, trans_cnt, emit_cnt = np.zeros(S), np.zeros((S, S)), np.zeros((S, V))
    loglik = np.full(B, np.nan)
    gamma = np.zeros((B, T, S))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(min(max(lengths[b], 0), T))
            if L == 0:
                continue
            c = codes[b, :L].astype(np.int64)
            if ((c < 0) | (c >= V)).any():
                continue
            em = log_B[:, c].T  # (L, S)
            al = np.empty((L, S))
            be = np.zeros((L, S))
            al[0] = log_pi + em[0]
            for t in range(1, L):
                al[t] = lse(al[t - 1][:, None] + log_A, 0) + em[t]
            for t in range(L - 1, 0, -1):
                be[t - 1] = lse(log_A + (em[t] + be[t])[None, :], 1)
            z = lse(al[L - 1], 0)
            loglik[b] = z
            if not np.isfinite(z):
                continue
            g = np.exp(al + be - z)
            gamma[b, :L] = g
            pi_cnt += g[0]
            np.add.at(emit_cnt.T, c, g)
            for t in range(1, L):
                trans_cnt += np.exp(al[t - 1][:, None] + log_A + (em[t] + be[t])[None, :] - z)
    return dict(pi_cnt=pi_cnt, trans_cnt=trans_cnt, emit_cnt=emit_cnt, loglik=loglik, gamma=gamma)


def brute_force(log_pi, log_A, log_B, codes):
    """One sequence (all of `codes`) by enumeration of the S^L paths -> the same dict for B = 1
    (gamma (L,S), loglik a scalar); an impossible sequence gives loglik = -inf and zeros."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    log_B = np.asarray(log_B, np.float64)
    S, V = log_B.shape
    c = [int(v) for v in codes]
    L = len(c)
    pi_cnt, trans_cnt, emit_cnt, gamma = np.zeros(S), np.zeros((S, S)), np.zeros((S, V)), np.zeros((L, S))
    if L == 0:
        return dict(pi_cnt=pi_cnt, trans_cnt=trans_cnt, emit_cnt=emit_cnt, loglik=np.nan, gamma=gamma)
    w = {}
    for path in itertools.product(range(S), repeat=L):
        lw = log_pi[path[0]] + log_B[path[0], c[0]]
        for t in range(1, L):
            lw += log_A[path[t - 1], path[t]] + log_B[path[t], c[t]]
        w[path] = np.exp(lw)
    Z = sum(w.values())
    if Z == 0:
        return dict(pi_cnt=pi_cnt, trans_cnt=trans_cnt, emit_cnt=emit_cnt, loglik=-np.inf, gamma=gamma)
    for path, v in w.items():
        p = v / Z
        pi_cnt[path[0]] += p
        for t in range(L):
            gamma[t, path[t]] += p
            emit_cnt[path[t], c[t]] += p
            if t >= 1:
                trans_cnt[path[t - 1], path[t]] += p
    return dict(pi_cnt=pi_cnt, trans_cnt=trans_cnt, emit_cnt=emit_cnt, loglik=np.log(Z), gamma=gamma)


def _m_rows(cnt, old, prior_count):
    cnt = np.asarray(cnt, np.float64).reshape(old.shape)
    old = np.asarray(old, np.float64)
    live = old != -np.inf
    w = np.where(live, cnt + prior_count, 0.0)
    tot = w.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        new = np.where(live, np.log(w / tot), -np.inf)
    return np.where(tot > 0, new, old)


def mstep_ref(counts, log_pi, log_A, log_B, prior_count=0.0):
    """(counts + prior_count where the parameter is not a structural zero), row-normalised, log; a row whose
    total is 0 keeps its parameters, -inf stays -inf -> (log_pi, log_A, log_B) float64."""
    return (_m_rows(counts["pi_cnt"], log_pi, prior_count), _m_rows(counts["trans_cnt"], log_A, prior_count),
            _m_rows(counts["emit_cnt"], log_B, prior_count))


def _draw(lp, u):
    """The contract's draw: p = exp(lp) in fp32, cdf = fp32 running sum in index order / its total, first k
    with u < cdf_k, else the last k with p_k > 0 -> (k, distance from u to the nearest cdf boundary)."""
    p = np.exp(np.asarray(lp, np.float32)).astype(np.float32)
    cdf = np.cumsum(p, dtype=np.float32)  # numpy's cumsum is the sequential running sum
    cdf = (cdf / cdf[-1]).astype(np.float32)
    u = np.float32(u)
    margin = float(np.abs(cdf.astype(np.float64) - float(u)).min())
    hit = np.nonzero((u < cdf) & (p > 0))[0]
    if hit.size:
        return int(hit[0]), margin
    pos = np.nonzero(p > 0)[0]
    return (int(pos[-1]) if pos.size else 0), margin


def sample_ref(log_pi, log_A, log_B, uniforms):
    """uniforms (N,T,2) fp32 -> states (N,T), codes (N,T) int64 and margins (N,T,2): per draw, the distance
    from u to the nearest boundary of that draw's fp32 CDF."""
    log_pi = np.asarray(log_pi, np.float32)
    log_A = np.asarray(log_A, np.float32)
    log_B = np.asarray(log_B, np.float32)
    u = np.asarray(uniforms, np.float32)
    N, T = u.shape[:2]
    states = np.zeros((N, T), np.int64)
    codes = np.zeros((N, T), np.int64)
    margins = np.zeros((N, T, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(N):
            z = 0
            for t in range(T):
                z, margins[n, t, 0] = _draw(log_pi if t == 0 else log_A[z], u[n, t, 0])
                c, margins[n, t, 1] = _draw(log_B[z], u[n, t, 1])
                states[n, t], codes[n, t] = z, c
    return states, codes, margins


def state_marginals(log_pi, log_A, log_B, T):
    """p(z_t) (T,S) = pi A^t and p(code_t) (T,V) = pi A^t B of the row-normalised model, float64."""
    pi = np.exp(np.asarray(log_pi, np.float64))
    A = np.exp(np.asarray(log_A, np.float64))
    Bm = np.exp(np.asarray(log_B, np.float64))
    pi, A, Bm = pi / pi.sum(), A / A.sum(1, keepdims=True), Bm / Bm.sum(1, keepdims=True)
    ps = np.empty((T, pi.shape[0]))
    ps[0] = pi
    for t in range(1, T):
        ps[t] = ps[t - 1] @ A
    return ps, ps @ Bm


# ------------------------------------------------------------------- shared cases
def random_model(rng, S, V, scale=1.0):
    """fp32 row-normalised log tables (what both the kernel and the helper are fed)."""
    def rows(*shape):
        a = rng.standard_normal(shape) * scale
        return (a - lse(a, -1)[..., None]).astype(np.float32)
    return rows(S), rows(S, S), rows(S, V)


# the sampler's exact-comparison cases: (S, V, numpy seed of the uniforms); N = 32, T = 48.  The seeds are
# vetted by tests/test_code_hmm_ref.py: every draw along the reference path lies at least (n + 4) 2^-23
# from the nearest CDF boundary.
SAMPLER_N, SAMPLER_T = 32, 48
SAMPLER_CASES = ((1, 1, 0), (3, 5, 0), (8, 16, 0))


def sampler_case(S, V, seed):
    log_pi, log_A, log_B = random_model(np.random.default_rng(1000 + 37 * S + V), S, V)
    u = np.random.default_rng(seed).random((SAMPLER_N, SAMPLER_T, 2), dtype=np.float32)
    return log_pi, log_A, log_B, u
