"""fp64 numpy restatement of the stationary HMM with full-covariance Gaussian emissions (a helper for the tests,
not a test): the emission log-densities, the Baum-Welch E-step, the moments under a given posterior, a brute-force
enumeration, the M-step and EM of include/vqhmm.h's full-covariance block / vqhmm.GaussianHMM(covariance_type=
"full").

    log_pi (S), log_A (S,S) rows = from-state, mean (S,D), prec_chol (S,D,D) = W_s = L_s^-1 lower-triangular with
    Sigma_s = L_s L_s^T (the strict upper triangle is ignored);  x (B,T,D), lengths (B), shift (D)
    em[t,s] = -1/2 |W_s (x_t - mean_s)|^2 + sum_i log W_s[i,i] - (D/2) ln 2 pi
    the chain, pi_cnt, trans_cnt, occ and m1 are gauss_hmm_ref's (its E-step runs on the emissions given here);
    m2[s] = sum_b w_b sum_t gamma_t(s) (x_t - shift)(x_t - shift)^T

The conventions are gauss_hmm_ref's: a length-0, impossible or non-finite sequence contributes nothing.
"""
import itertools

import numpy as np

import gauss_hmm_ref as G

LN2PI = G.LN2PI


def emission_ref(mean, prec_chol, x, lengths=None):
    """-> em (B,T,S) float64 (rows at t >= length are -inf) and the bound's magnitude
    A (B,T,S) = 1/2 sum_i (sum_{j<=i} |W_ij| |x_j - mean_j|)^2 + |sum_i log W_ii| + (D/2) ln 2 pi."""
    mean = np.asarray(mean, np.float64)
    W = np.tril(np.asarray(prec_chol, np.float64))
    x = np.asarray(x, np.float64)
    B, T, D = x.shape
    lengths = np.full(B, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = x[:, :, None, :] - mean[None, None]                       # (B,T,S,D)
        r = np.einsum("sij,btsj->btsi", W, z)
        ra = np.einsum("sij,btsj->btsi", np.abs(W), np.abs(z))
        ld = np.log(np.diagonal(W, axis1=1, axis2=2)).sum(-1)          # (S)
        em = -0.5 * (r * r).sum(-1) + ld[None, None] - 0.5 * D * LN2PI
        mag = 0.5 * (ra * ra).sum(-1) + np.abs(ld)[None, None] + 0.5 * D * LN2PI
    pad = np.arange(T)[None, :] >= lengths[:, None]
    em[pad] = -np.inf
    return em, mag


def _full_m2(gamma, loglik, x, lengths, shift, weights):
    xf = np.asarray(x, np.float64)
    B, T, D = xf.shape
    S = gamma.shape[2]
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    m2 = np.zeros((S, D, D))
    for b in range(B):
        L = int(min(max(lengths[b], 0), T))
        if L == 0 or not np.isfinite(loglik[b]):
            continue
        y = xf[b, :L] - sh
        m2 += w[b] * np.einsum("ts,ti,tj->sij", gamma[b, :L], y, y)
    return m2


def estep_ref(log_pi, log_A, mean, prec_chol, x, lengths=None, shift=None, weights=None, em=None):
    """-> dict(pi_cnt (S), trans_cnt (S,S), occ (S), m1 (S,D), m2 (S,D,D), loglik (B), gamma (B,T,S), xi (B,T,S,S)),
    all float64.  em (B,T,S): use these emissions in place of emission_ref's (the GPU tests feed the tensor the
    emission entry wrote)."""
    xf = np.asarray(x, np.float64)
    B, T, D = xf.shape
    lengths = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    if em is None:
        em = emission_ref(mean, prec_chol, xf, lengths)[0]
    out = G.estep_ref(log_pi, log_A, mean, None, xf, lengths, shift=shift, weights=weights, em=em)
    out["m2"] = _full_m2(out["gamma"], out["loglik"], xf, lengths, shift, weights)
    return out


def moments_ref(x, gamma, lengths=None, shift=None, weights=None):
    """occ (S), m1 (S,D), m2 (S,D,D) under a given gamma (B,T,S); a sequence with a non-finite x or gamma inside
    its length contributes nothing."""
    xf = np.asarray(x, np.float64)
    g = np.asarray(gamma, np.float64)
    B, T, D = xf.shape
    S = g.shape[2]
    lengths = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    occ, m1, m2 = np.zeros(S), np.zeros((S, D)), np.zeros((S, D, D))
    for b in range(B):
        L = int(min(max(lengths[b], 0), T))
        if L == 0 or not (np.isfinite(xf[b, :L]).all() and np.isfinite(g[b, :L]).all()):
            continue
        y = xf[b, :L] - sh
        occ += w[b] * g[b, :L].sum(0)
        m1 += w[b] * (g[b, :L].T @ y)
        m2 += w[b] * np.einsum("ts,ti,tj->sij", g[b, :L], y, y)
    return dict(occ=occ, m1=m1, m2=m2)


def brute_force(log_pi, log_A, mean, cov, x, shift=None, weight=1.0):
    """One sequence (all rows of x (L,D)) by enumeration of the S^L paths, with the density written from the
    covariances (solve and slogdet, no Cholesky) -> the E-step's dict for B = 1 (gamma (L,S), loglik a scalar)."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    mean = np.asarray(mean, np.float64)
    cov = np.asarray(cov, np.float64)
    x = np.asarray(x, np.float64)
    L, D = x.shape
    S = log_pi.shape[0]
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    out = dict(pi_cnt=np.zeros(S), trans_cnt=np.zeros((S, S)), occ=np.zeros(S), m1=np.zeros((S, D)),
               m2=np.zeros((S, D, D)), gamma=np.zeros((L, S)), loglik=np.nan)
    if L == 0:
        return out

    def dens(s, t):
        d = x[t] - mean[s]
        return float(-0.5 * d @ np.linalg.solve(cov[s], d) - 0.5 * np.linalg.slogdet(2 * np.pi * cov[s])[1])

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
            y = x[t] - sh
            out["gamma"][t, s] += v / Z
            out["occ"][s] += p
            out["m1"][s] += p * y
            out["m2"][s] += p * np.outer(y, y)
            if t >= 1:
                out["trans_cnt"][path[t - 1], s] += p
    return out


def prec_chol_of(cov):
    """W = L^-1 (S,D,D) float64 for cov = L L^T."""
    return np.stack([np.linalg.inv(np.linalg.cholesky(c)) for c in np.asarray(cov, np.float64)])


def mstep_ref(counts, log_pi, log_A, mean, cov, shift=None, prior_count=0.0, reg_covar=1e-6, mixture=False):
    """-> (log_pi, log_A, mean, cov) float64: rows of pi and A as gauss_hmm_ref's M-step; mean = shift + m1/occ,
    cov = m2/occ - mu mu^T + reg_covar I with mu = m1/occ; a state with occ = 0 keeps its old mean and cov."""
    mean = np.asarray(mean, np.float64)
    cov = np.asarray(cov, np.float64)
    occ = np.asarray(counts["occ"], np.float64)
    D = mean.shape[1]
    sh = np.zeros(D) if shift is None else np.asarray(shift, np.float64)
    if mixture:
        npi = G._m_rows(occ, np.asarray(log_pi, np.float64), prior_count)
        nA = np.broadcast_to(npi, np.asarray(log_A).shape).copy()
    else:
        npi = G._m_rows(counts["pi_cnt"], log_pi, prior_count)
        nA = G._m_rows(counts["trans_cnt"], log_A, prior_count)
    live = occ > 0
    o = np.where(live, occ, 1.0)
    mu = np.asarray(counts["m1"], np.float64) / o[:, None]
    ncov = np.asarray(counts["m2"], np.float64) / o[:, None, None] - mu[:, :, None] * mu[:, None, :]
    ncov = ncov + reg_covar * np.eye(D)
    return npi, nA, np.where(live[:, None], sh[None] + mu, mean), np.where(live[:, None, None], ncov, cov)


def em_ref(log_pi, log_A, mean, cov, x, lengths=None, n_iter=10, shift=None, prior_count=0.0, reg_covar=1e-6,
           mixture=False):
    """n_iter rounds of estep_ref + mstep_ref on (log_pi, log_A, mean, cov) -> (parameters, [total loglik before
    each M-step])."""
    p = [np.asarray(a, np.float64) for a in (log_pi, log_A, mean, cov)]
    hist = []
    for _ in range(n_iter):
        c = estep_ref(p[0], p[1], p[2], prec_chol_of(p[3]), x, lengths, shift=shift)
        hist.append(float(np.nansum(c["loglik"])))
        p = list(mstep_ref(c, *p, shift=shift, prior_count=prior_count, reg_covar=reg_covar, mixture=mixture))
    return p, hist


# ------------------------------------------------------------------- shared cases
def random_model(rng, S, D, spread=2.0):
    """fp32 parameters (what both the kernels and the helper are fed): row-normalised log_pi, log_A, means of
    spread `spread`, and prec_chol = the inverse of a random lower factor L (diagonal in [0.6, 1.6], off-diagonal
    0.4 N(0,1) / sqrt(D)), rounded to fp32 with an exactly zero upper triangle -> (log_pi, log_A, mean, prec_chol)."""
    log_pi, log_A, mean, _ = G.random_model(rng, S, D, spread=spread)
    L = np.tril(rng.standard_normal((S, D, D)) * 0.4 / np.sqrt(D), -1)
    L[:, np.arange(D), np.arange(D)] = rng.uniform(0.6, 1.6, (S, D))
    W = np.tril(np.stack([np.linalg.inv(l) for l in L])).astype(np.float32)
    return log_pi, log_A, mean, W


def scale_tril_of(prec_chol):
    """L = W^-1 (S,D,D) float64."""
    return np.stack([np.linalg.inv(np.tril(w)) for w in np.asarray(prec_chol, np.float64)])


def sample_data(rng, log_pi, log_A, mean, scale_tril, B, T):
    """x (B,T,D) fp32 and states (B,T) drawn from the model (fp64 arithmetic, numpy draws)."""
    log_pi, log_A, mean, Lc = (np.asarray(a, np.float64) for a in (log_pi, log_A, mean, scale_tril))
    S, D = mean.shape
    pi = np.exp(log_pi) / np.exp(log_pi).sum()
    A = np.exp(log_A) / np.exp(log_A).sum(1, keepdims=True)
    x = np.empty((B, T, D))
    zs = np.empty((B, T), np.int64)
    for b in range(B):
        z = rng.choice(S, p=pi)
        for t in range(T):
            if t:
                z = rng.choice(S, p=A[z])
            zs[b, t] = z
            x[b, t] = mean[z] + Lc[z] @ rng.standard_normal(D)
    return x.astype(np.float32), zs


# the module's fit test: three sticky regimes in D = 4 with correlated covariances
FIT_B, FIT_T, FIT_S, FIT_D = 8, 60, 3, 4


def fit_case(seed=11):
    """-> (x (B,T,D) fp32, lengths (B), init (log_pi, log_A, mean, scale_tril) fp32): data from a sticky
    three-state model with means -3, 0, 3 and random correlated covariances; the start is rough (means -2, 0.5,
    2.5, identity factors scaled by 1.5, uniform pi and A)."""
    rng = np.random.default_rng(seed)
    A = np.full((3, 3), 0.05) + np.eye(3) * 0.85
    _, _, _, W = random_model(rng, FIT_S, FIT_D)
    mean = np.repeat(np.array([-3.0, 0.0, 3.0])[:, None], FIT_D, 1)
    x, _ = sample_data(rng, np.log(np.full(3, 1 / 3)), np.log(A), mean, scale_tril_of(W), FIT_B, FIT_T)
    lengths = np.full(FIT_B, FIT_T, np.int64)
    lengths[1::3] = rng.integers(FIT_T // 2, FIT_T, lengths[1::3].shape)
    init_mean = np.array([-2.0, 0.5, 2.5])[:, None] + 0.25 * np.arange(FIT_D)[None, :]
    init = (np.log(np.full(3, 1 / 3)).astype(np.float32), np.log(np.full((3, 3), 1 / 3)).astype(np.float32),
            init_mean.astype(np.float32), np.repeat(1.5 * np.eye(FIT_D, dtype=np.float32)[None], 3, 0))
    return x, lengths, init
