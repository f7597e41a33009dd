"""fp64 numpy restatement of the causal filter, the log-likelihood and the pairwise posteriors of
the HMM over per-step tables (a helper for the tests, not a test).

    alpha_0(j) = log_pi(j) + em_0(j),  alpha_t(j) = lse_i(alpha_{t-1}(i) + log_A_t(i,j)) + em_t(j)
    beta_{L-1} = 0,  beta_{t-1}(i) = lse_j(log_A_t(i,j) + em_t(j) + beta_t(j))
    filt_t   = softmax_j alpha_t,  loglik = logZ = lse_j alpha_{L-1}(j)
    gamma_t  = exp(alpha_t + beta_t - logZ)
    xi_t(i,j) = exp(alpha_{t-1}(i) + log_A_t(i,j) + em_t(j) + beta_t(j) - logZ)      (1 <= t < L)

Conventions of include/vqhmm.h: log_A[:, t] is the transition t-1 -> t, rows at t >= L are 0,
xi[:, 0] = 0, a length-0 sequence has loglik = logZ = NaN and zero rows.
"""
import itertools

import numpy as np


def lse(a, axis):
    a = np.asarray(a, np.float64)
    m = a.max(axis=axis, keepdims=True)
    mz = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = mz + np.log(np.exp(a - mz).sum(axis=axis, keepdims=True))
    return np.squeeze(r, axis=axis)


def pair_ref(log_pi, log_A, em, lengths=None):
    """-> dict(filt (B,T,K), loglik (B,), gamma (B,T,K), xi (B,T,K,K), logZ (B,)), all float64."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    em = np.asarray(em, np.float64)
    B, T, K = em.shape
    lengths = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    filt = np.zeros((B, T, K))
    gamma = np.zeros((B, T, K))
    xi = np.zeros((B, T, K, K))
    loglik = np.full(B, np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(min(max(lengths[b], 0), T))
            if L == 0:
                continue
            al = np.empty((L, K))
            be = np.zeros((L, K))
            al[0] = log_pi + em[b, 0]
            for t in range(1, L):
                al[t] = lse(al[t - 1][:, None] + log_A[b, t], 0) + em[b, t]
            for t in range(L - 1, 0, -1):
                be[t - 1] = lse(log_A[b, t] + (em[b, t] + be[t])[None, :], 1)
            z = lse(al[L - 1], 0)
            loglik[b] = z
            if not np.isfinite(z):  # impossible sequence: posteriors undefined, left at 0
                continue
            filt[b, :L] = np.exp(al - lse(al, 1)[:, None])
            gamma[b, :L] = np.exp(al + be - z)
            for t in range(1, L):
                xi[b, t] = np.exp(al[t - 1][:, None] + log_A[b, t] + (em[b, t] + be[t])[None, :] - z)
    return dict(filt=filt, loglik=loglik, gamma=gamma, xi=xi, logZ=loglik.copy())


def brute_force(log_pi, log_A, em, L):
    """One sequence (T,K,K) / (T,K) by enumeration of all K^L paths ->
    (filt (L,K), loglik, gamma (L,K), xi (L,K,K)); filt_t enumerates the paths of the prefix 0..t."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    em = np.asarray(em, np.float64)
    K = log_pi.shape[0]

    def joint(n):  # weights of all paths of length n
        out = {}
        for path in itertools.product(range(K), repeat=n):
            lw = log_pi[path[0]] + em[0, path[0]]
            for t in range(1, n):
                lw += log_A[t, path[t - 1], path[t]] + em[t, path[t]]
            out[path] = np.exp(lw)
        return out

    filt = np.zeros((L, K))
    for t in range(L):
        w = joint(t + 1)
        for path, v in w.items():
            filt[t, path[-1]] += v
        filt[t] /= filt[t].sum()
    w = joint(L)
    Z = sum(w.values())
    gamma = np.zeros((L, K))
    xi = np.zeros((L, K, K))
    for path, v in w.items():
        for t in range(L):
            gamma[t, path[t]] += v / Z
            if t >= 1:
                xi[t, path[t - 1], path[t]] += v / Z
    return filt, np.log(Z), gamma, xi
