"""fp64 numpy restatement of the stationary HMM with diagonal-Gaussian emissions (a helper for the tests,
not a test): the emission log-densities, the Baum-Welch E-step in log space with xi, a brute-force
enumeration, the M-step, EM, the sampler and mean_path of include/vqhmm.h / vqhmm.GaussianHMM.

    log_pi (S), log_A (S,S) rows = from-state, mean (S,D), log_var (S,D);  x (B,T,D), lengths (B), shift (D)
    em[t,s] = -1/2 sum_d ((x_d - mean_sd)^2 exp(-log_var_sd) + log_var_sd) - (D/2) ln 2 pi
    alpha_0 = log_pi + em_0,  alpha_t(j) = lse_i(alpha_{t-1}(i) + log_A(i,j)) + em_t(j)
    beta_{L-1} = 0,  beta_{t-1}(i) = lse_j(log_A(i,j) + em_t(j) + beta_t(j))
    gamma_t = exp(alpha_t + beta_t - loglik),  xi_t(i,j) = exp(alpha_{t-1}(i) + log_A(i,j) + em_t(j) + beta_t(j) - loglik)
    pi_cnt = sum_b w_b gamma_0, trans_cnt = sum w_b xi_t, occ = sum w_b gamma_t,
    m1 = sum w_b gamma_t(s) (x_t - shift), m2 = sum w_b gamma_t(s) (x_t - shift)^2

Conventions of include/vqhmm.h: length 0 -> loglik NaN; an impossible sequence -> loglik -inf; a non-finite x or
emission inside the length -> loglik NaN; all three contribute nothing and have zero gamma rows.
"""
import itertools

import numpy as np

from hmm_pair_ref import lse

LN2PI = float(np.log(2.0 * np.pi))


def emission_ref(mean, log_var, x, lengths=None):
    """-> em (B,T,S) float64 (rows at t >= length are -inf) and the bound's magnitude
    A (B,T,S) = sum_d (z^2/2 + |log_var|/2) + (D/2) ln 2 pi."""
    mean = np.asarray(mean, np.float64)
    log_var = np.asarray(log_var, np.float64)
    x = np.asarray(x, np.float64)
    B, T, D = x.shape
    lengths = np.full(B, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)
    with np.errstate(invalid="ignore", over="ignore"):
        z2 = (x[:, :, None, :] - mean[None, None]) ** 2 * np.exp(-log_var)[None, None]
        em = -0.5 * (z2 + log_var[None, None]).sum(-1) - 0.5 * D * LN2PI
        mag = 0.5 * (z2 + np.abs(log_var)[None, None]).sum(-1) + 0.5 * D * LN2PI
    pad = np.arange(T)[None, :] >= lengths[:, None]
    em[pad] = -np.inf
    return em, mag


def estep_ref(log_pi, log_A, mean, log_var, x, lengths=None, shift=None, weights=None, em=None):
    """-> dict(pi_cnt (S), trans_cnt (S,S), occ (S), m1 (S,D), m2 (S,D), loglik (B), gamma (B,T,S), xi (B,T,S,S)),
    all float64.  em (B,T,S): use these emissions in place of emission_ref's (the GPU tests feed the tensor the
    emission entry wrote)."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    xf = np.asarray(x, np.float64)
    B, T, D = xf.shape
    S = log_pi.shape[0]
    lengths = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    if em is None:
        em = emission_ref(mean, log_var, xf, lengths)[0]
    em = np.asarray(em, np.float64)
    pi_cnt, trans_cnt, occ = np.zeros(S), np.zeros((S, S)), np.zeros(S)
    m1, m2 = np.zeros((S, D)), np.zeros((S, D))
    loglik = np.full(B, np.nan)
    gamma = np.zeros((B, T, S))
    xi = np.zeros((B, T, S, S))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(min(max(lengths[b], 0), T))
            if L == 0:
                continue
            e = em[b, :L]
            if not (np.isfinite(e).all() and np.isfinite(xf[b, :L]).all()):
                continue
            al = np.empty((L, S))
            be = np.zeros((L, S))
            al[0] = log_pi + e[0]
            for t in range(1, L):
                al[t] = lse(al[t - 1][:, None] + log_A, 0) + e[t]
            for t in range(L - 1, 0, -1):
                be[t - 1] = lse(log_A + (e[t] + be[t])[None, :], 1)
            z = lse(al[L - 1], 0)
            loglik[b] = z
            if not np.isfinite(z):
                continue
            g = np.exp(al + be - z)
            gamma[b, :L] = g
            for t in range(1, L):
                xi[b, t] = np.exp(al[t - 1][:, None] + log_A + (e[t] + be[t])[None, :] - z)
            y = xf[b, :L] - sh
            pi_cnt += w[b] * g[0]
            trans_cnt += w[b] * xi[b].sum(0)
            occ += w[b] * g.sum(0)
            m1 += w[b] * (g.T @ y)
            m2 += w[b] * (g.T @ (y * y))
    return dict(pi_cnt=pi_cnt, trans_cnt=trans_cnt, occ=occ, m1=m1, m2=m2, loglik=loglik, gamma=gamma, xi=xi)


def brute_force(log_pi, log_A, mean, log_var, x, shift=None, weight=1.0):
    """One sequence (all rows of x (L,D)) by enumeration of the S^L paths -> the same dict for B = 1 (gamma (L,S),
    loglik a scalar, no xi); an impossible sequence gives loglik = -inf and zeros."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    mean = np.asarray(mean, np.float64)
    log_var = np.asarray(log_var, np.float64)
    x = np.asarray(x, np.float64)
    L, D = x.shape
    S = log_pi.shape[0]
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    out = dict(pi_cnt=np.zeros(S), trans_cnt=np.zeros((S, S)), occ=np.zeros(S), m1=np.zeros((S, D)),
               m2=np.zeros((S, D)), gamma=np.zeros((L, S)), loglik=np.nan)
    if L == 0:
        return out
    var = np.exp(log_var)

    def dens(s, t):  # log N(x_t; mean_s, var_s), written out on its own
        return float(np.sum(-0.5 * np.log(2 * np.pi * var[s]) - (x[t] - mean[s]) ** 2 / (2 * var[s])))

    w = {}
    with np.errstate(divide="ignore"):
        for path in itertools.product(range(S), repeat=L):
            lw = log_pi[path[0]] + dens(path[0], 0)
            for t in range(1, L):
                lw += log_A[path[t - 1], path[t]] + dens(path[t], t)
            w[path] = np.exp(lw)
        Z = sum(w.values())
        out["loglik"] = -np.inf if Z == 0 else np.log(Z)
    if Z == 0:
        return out
    for path, v in w.items():
        p = weight * v / Z
        out["pi_cnt"][path[0]] += p
        for t in range(L):
            s = path[t]
            out["gamma"][t, s] += v / Z
            out["occ"][s] += p
            out["m1"][s] += p * (x[t] - sh)
            out["m2"][s] += p * (x[t] - sh) ** 2
            if t >= 1:
                out["trans_cnt"][path[t - 1], s] += p
    return out


def _m_rows(cnt, old, prior_count):
    cnt = np.asarray(cnt, np.float64).reshape(old.shape)
    old = np.asarray(old, np.float64)
    live = old != -np.inf
    w = np.where(live, cnt + prior_count, 0.0)
    tot = w.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        new = np.where(live, np.log(w / tot), -np.inf)
    return np.where(tot > 0, new, old)


def mstep_ref(counts, log_pi, log_A, mean, log_var, shift=None, prior_count=0.0, var_floor=1e-6, mixture=False):
    """-> (log_pi, log_A, mean, log_var) float64: rows of pi and A as the code HMM's M-step; mean = shift + m1/occ,
    var = max(m2/occ - (m1/occ)^2, var_floor); a state with occ = 0 keeps its old row.  mixture: every row of A is
    the new pi, estimated from occ."""
    mean = np.asarray(mean, np.float64)
    log_var = np.asarray(log_var, np.float64)
    occ = np.asarray(counts["occ"], np.float64)
    m1 = np.asarray(counts["m1"], np.float64)
    m2 = np.asarray(counts["m2"], np.float64)
    sh = np.zeros(mean.shape[1]) if shift is None else np.asarray(shift, np.float64)
    if mixture:
        npi = _m_rows(occ, np.asarray(log_pi, np.float64), prior_count)
        nA = np.broadcast_to(npi, np.asarray(log_A).shape).copy()
    else:
        npi = _m_rows(counts["pi_cnt"], log_pi, prior_count)
        nA = _m_rows(counts["trans_cnt"], log_A, prior_count)
    live = occ > 0
    o = np.where(live, occ, 1.0)[:, None]
    mu = m1 / o
    var = np.maximum(m2 / o - mu * mu, var_floor)
    nmean = np.where(live[:, None], sh[None] + mu, mean)
    nlv = np.where(live[:, None], np.log(var), log_var)
    return npi, nA, nmean, nlv


def em_ref(log_pi, log_A, mean, log_var, x, lengths=None, n_iter=10, shift=None, prior_count=0.0, var_floor=1e-6,
           mixture=False):
    """n_iter rounds of estep_ref + mstep_ref -> (parameters, [total loglik before each M-step])."""
    p = [np.asarray(a, np.float64) for a in (log_pi, log_A, mean, log_var)]
    hist = []
    for _ in range(n_iter):
        c = estep_ref(*p, x, lengths, shift=shift)
        hist.append(float(np.nansum(c["loglik"])))
        p = list(mstep_ref(c, *p, shift=shift, prior_count=prior_count, var_floor=var_floor, mixture=mixture))
    return p, hist


def _draw(lp, u):
    """vqhmm_code_sample_f32's draw -> (k, distance from u to the nearest cdf boundary)."""
    p = np.exp(np.asarray(lp, np.float32)).astype(np.float32)
    cdf = np.cumsum(p, dtype=np.float32)
    cdf = (cdf / cdf[-1]).astype(np.float32)
    u = np.float32(u)
    margin = float(np.abs(cdf.astype(np.float64) - float(u)).min())
    hit = np.nonzero((u < cdf) & (p > 0))[0]
    if hit.size:
        return int(hit[0]), margin
    pos = np.nonzero(p > 0)[0]
    return (int(pos[-1]) if pos.size else 0), margin


def sample_ref(log_pi, log_A, mean, log_var, uniforms, normals):
    """uniforms (N,T) fp32, normals (N,T,D) fp32 -> states (N,T) int64, x (N,T,D) float32 by the contract's fp32
    rule (sd = exp(log_var / 2) in fp64 rounded once, x = one fma) and margins (N,T)."""
    log_pi = np.asarray(log_pi, np.float32)
    log_A = np.asarray(log_A, np.float32)
    mean = np.asarray(mean, np.float32)
    sd = np.exp(0.5 * np.asarray(log_var, np.float32).astype(np.float64)).astype(np.float32)
    u = np.asarray(uniforms, np.float32)
    nr = np.asarray(normals, np.float32)
    N, T = u.shape
    states = np.zeros((N, T), np.int64)
    margins = np.zeros((N, T))
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(N):
            z = 0
            for t in range(T):
                z, margins[n, t] = _draw(log_pi if t == 0 else log_A[z], u[n, t])
                states[n, t] = z
    # fmaf: the exact product and sum in fp64 (24 + 24 bits fit), rounded once
    xs = (sd[states].astype(np.float64) * nr.astype(np.float64) + mean[states].astype(np.float64)).astype(np.float32)
    return states, xs, margins


def mean_path_ref(log_pi, log_A, mean, T):
    """E[x_t] (T,D) of the row-normalised model: (pi A^t) mean."""
    pi = np.exp(np.asarray(log_pi, np.float64))
    A = np.exp(np.asarray(log_A, np.float64))
    pi, A = pi / pi.sum(), A / A.sum(1, keepdims=True)
    ps = np.empty((T, pi.shape[0]))
    if T:
        ps[0] = pi
    for t in range(1, T):
        ps[t] = ps[t - 1] @ A
    return ps @ np.asarray(mean, np.float64)


# ------------------------------------------------------------------- shared cases
def random_model(rng, S, D, scale=1.0, spread=2.0):
    """fp32 parameters (what both the kernels and the helper are fed): row-normalised log_pi, log_A, means of
    spread `spread`, log_var in [-1, 1]."""
    def rows(*shape):
        a = rng.standard_normal(shape) * scale
        return (a - lse(a, -1)[..., None]).astype(np.float32)
    mean = (rng.standard_normal((S, D)) * spread).astype(np.float32)
    log_var = rng.uniform(-1.0, 1.0, (S, D)).astype(np.float32)
    return rows(S), rows(S, S), mean, log_var


def sample_data(rng, model, B, T):
    """x (B,T,D) fp32 drawn from the model (fp64 arithmetic, numpy draws)."""
    log_pi, log_A, mean, log_var = (np.asarray(a, np.float64) for a in model)
    S, D = mean.shape
    pi = np.exp(log_pi) / np.exp(log_pi).sum()
    A = np.exp(log_A) / np.exp(log_A).sum(1, keepdims=True)
    x = np.empty((B, T, D))
    for b in range(B):
        z = rng.choice(S, p=pi)
        for t in range(T):
            if t:
                z = rng.choice(S, p=A[z])
            x[b, t] = mean[z] + np.exp(0.5 * log_var[z]) * rng.standard_normal(D)
    return x.astype(np.float32)


# the sampler's exact-comparison cases: (S, D, numpy seed of the draws); N = 32, T = 48.  The seeds are vetted by
# tests/test_gauss_hmm_ref.py: every uniform along the reference path lies at least 1e-4 from a CDF boundary.
SAMPLER_N, SAMPLER_T = 32, 48
SAMPLER_MARGIN = 1e-4
SAMPLER_CASES = ((1, 1, 0), (3, 5, 0), (8, 16, 0))


def sampler_case(S, D, seed):
    """-> (log_pi, log_A, mean, log_var, uniforms (N,T), normals (N,T,D)): uniforms closer than SAMPLER_MARGIN to a
    CDF boundary of their own draw are redrawn (from the same generator) until the whole path keeps its distance."""
    model = random_model(np.random.default_rng(2000 + 37 * S + D), S, D)
    rng = np.random.default_rng(seed)
    u = rng.random((SAMPLER_N, SAMPLER_T), dtype=np.float32)
    nr = rng.standard_normal((SAMPLER_N, SAMPLER_T, D), dtype=np.float32)
    for _ in range(100):
        _, _, margins = sample_ref(*model, u, nr)
        close = margins < SAMPLER_MARGIN
        if not close.any():
            break
        u[close] = rng.random(int(close.sum()), dtype=np.float32)
    return (*model, u, nr)


# the fit test's data: three planted states with means -5, 0, 5 in every dimension, unit variance, a sticky A
FIT_B, FIT_T, FIT_D = 64, 100, 2
FIT_MEANS = np.array([-5.0, 0.0, 5.0])


def fit_case(seed=7):
    """-> (x (B,T,D) fp32, lengths (B), init (log_pi, log_A, mean, log_var) fp32): the initial means are rough
    (-3, 1, 4 with a per-dimension offset), the variances 4, pi and A uniform."""
    rng = np.random.default_rng(seed)
    A = np.full((3, 3), 0.05) + np.eye(3) * 0.85
    model = (np.log(np.full(3, 1 / 3)), np.log(A), np.repeat(FIT_MEANS[:, None], FIT_D, 1), np.zeros((3, FIT_D)))
    x = sample_data(rng, model, FIT_B, FIT_T)
    lengths = np.full(FIT_B, FIT_T, np.int64)
    lengths[1::7] = rng.integers(FIT_T // 2, FIT_T, lengths[1::7].shape)
    init_mean = np.array([-3.0, 1.0, 4.0])[:, None] + np.array([0.0, 0.5])[None, :FIT_D]
    init = (np.log(np.full(3, 1 / 3)).astype(np.float32), np.log(np.full((3, 3), 1 / 3)).astype(np.float32),
            init_mean.astype(np.float32), np.full((3, FIT_D), np.log(4.0), np.float32))
    return x, lengths, init
