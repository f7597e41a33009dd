"""Numpy reference of vqhmm_gauss_scenario_f32 (contract: include/vqhmm.h, "Gaussian HMM scenarios").

philox4x32_10: the Random123 generator, vectorised over counters.  scenario_ref: all B N paths at once (a Python
loop over the H steps only): the counter layout, the regime draw by gauss_hmm_ref._draw's rule and margin (fp32
running sum, u < run / total; draw_rows, which the CPU test checks against _draw itself), Box-Muller in fp64 from the same integers, x and the wealth recursion in fp64, and
the error bounds the GPU test asserts.  scenario_path_loop: one path, written separately as a literal day-by-day
loop in the style of the reference's monte_carlo_simulation, which the vectorised form must agree with.

Bounds (all derived, none measured):
  x: |x - x_ref| <= 1e-5 sum_j |L_ij| + 1e-6 (|mean_i| + sum_j |L_ij eps_j|).  The first term is the error of eps:
     ocml's bounds for logf (1 ulp), sqrtf (correctly rounded), sinpif / cospif (2 ulp) and the product's
     rounding give about 2.5e-6 absolute at r <= 5.77, times 4; the second the fp32 roundings of the fma chain
     (at most 33 of them, 6e-8 each, on partial sums below |mean_i| + sum_j |L_ij eps_j|).
  wealth, against the independent reference: to first order d(w_t) / w_t = sum_{s <= t} sum_d |held_d| dx_{s,d} /
     |1 + r_s| with dx the x bound, r_s the step's portfolio return; the bound is 1.05 times that (second order)
     plus 1e-6 (the fp32 store, 6e-8, and the fp64 recursion).  drawdown = 1 - w / peak moves by at most the
     relative errors of w and of peak: twice the largest relative bound over the path.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MARGIN = 1e-4          # a path with a regime uniform closer than this to a cdf boundary is left out of exact checks
MAX_LEFT_OUT = 0.25    # ... and at most this fraction of a case's paths may be


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) (broadcastable) unsigned 32-bit words -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def path_words(seed, bq, nq, t, j):
    """The Philox block of path (bq, nq) (global indices, arrays) at step t, block j: key = (seed low, seed high),
    counter = (nq, bq, t, j)."""
    bq, nq = np.broadcast_arrays(np.asarray(bq, np.uint64), np.asarray(nq, np.uint64))
    ctr = np.stack([nq, bq, np.full(nq.shape, t, np.uint64), np.full(nq.shape, j, np.uint64)], -1)
    return philox4x32_10(ctr, np.array([seed & MASK, (seed >> 32) & MASK], np.uint64))


def uniform_of(word):
    return ((np.asarray(word, np.uint32) >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def box_muller(wa, wb):
    """-> (eps_even, eps_odd) fp64 from two words."""
    u1 = ((np.asarray(wa, np.uint32) >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(wb, np.uint32) >> 8).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def normals(seed, bq, nq, t, D):
    """eps (..., D) fp64 of the paths at step t: block 1 + d // 4, word pairs (0,1) and (2,3)."""
    cols = []
    for j in range((D + 3) // 4):
        w = path_words(seed, bq, nq, t, 1 + j)
        cols += list(box_muller(w[..., 0], w[..., 1])) + list(box_muller(w[..., 2], w[..., 3]))
    return np.stack(cols[:D], -1)


def draw_rows(p, u):
    """gauss_hmm_ref._draw over rows of weights: p (P,S) fp32 >= 0, u (P,) fp32 -> (k (P,), margin (P,))."""
    p = np.asarray(p, np.float32)
    cdf = np.cumsum(p, axis=1, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        cdf = (cdf / cdf[:, -1:]).astype(np.float32)
    u = np.asarray(u, np.float32)[:, None]
    margin = np.abs(cdf.astype(np.float64) - u.astype(np.float64)).min(1)
    hit = (u < cdf) & (p > 0)
    S = p.shape[1]
    first = np.where(hit.any(1), hit.argmax(1), -1)
    last = np.where((p > 0).any(1), S - 1 - (p[:, ::-1] > 0).argmax(1), 0)
    return np.where(first >= 0, first, last).astype(np.int64), margin


def _bad_total(p):
    tot = np.cumsum(np.asarray(p, np.float32), axis=1, dtype=np.float32)[:, -1]
    return ~((tot > 0) & np.isfinite(tot))


def scale_matrix(scale, full):
    """L (S,D,D) fp64: the lower triangle of scale, or diag(sd)."""
    scale = np.asarray(scale, np.float32).astype(np.float64)
    if full:
        return np.tril(scale)
    S, D = scale.shape
    L = np.zeros((S, D, D))
    L[:, np.arange(D), np.arange(D)] = scale
    return L


def wealth_ref(x, states, port, rebalance, tx_cost):
    """The contract's fp64 wealth recursion on given x (P,H,D) (fp32 or fp64 values) and states (P,H) (-1 = failed)
    -> (wealth (P,H), final (P,), drawdown (P,), (rets (P,H), helds (P,H,D))): the step's portfolio return and
    holdings, which wealth_bound takes."""
    x = np.asarray(x, np.float64)
    states = np.asarray(states)
    port = np.asarray(port, np.float32).astype(np.float64)
    P, H, D = x.shape
    tx = float(np.float32(tx_cost))
    w, peak, dd = np.ones(P), np.ones(P), np.zeros(P)
    held = np.zeros((P, D))
    wealth = np.empty((P, H))
    rets = np.empty((P, H))
    helds = np.empty((P, H, D))
    bad = np.zeros(P, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(H):
            bad |= states[:, t] < 0
            z = np.where(bad, 0, states[:, t])
            if t % rebalance == 0:
                w = w - w * tx * np.abs(port[z] - held).sum(1)
                held = port[z]
            r = np.zeros(P)
            for d in range(D):
                r = r + held[:, d] * x[:, t, d]
            w = np.where(bad, np.nan, w * (1.0 + r))
            wealth[:, t], rets[:, t], helds[:, t] = w, r, held
            peak = np.where(w > peak, w, peak)
            dd = np.where(w < peak, np.maximum(dd, 1.0 - w / peak), dd)
    return wealth, np.where(bad, np.nan, w), np.where(bad, np.nan, dd), (rets, helds)


def wealth_bound(wealth, rets, helds, xtol):
    """The propagated x bound (module docstring) -> (wealth_tol (P,H), drawdown_tol (P,))."""
    with np.errstate(invalid="ignore", divide="ignore"):
        step = (np.abs(helds) * xtol).sum(2) / np.abs(1.0 + rets)
        rel = 1.05 * np.cumsum(step, axis=1) + 1e-6
    return np.abs(wealth) * rel, 2.0 * rel.max(1)


def scenario_ref(start, log_A, mean, scale, full, port, rebalance, tx_cost, seed, b0, n0, B, N, H):
    """-> dict: states (B,N,H) int64 (-1 from the failing step on), u (B,N,H) fp32, margin (B,N,H), eps, x, xtol
    (B,N,H,D) fp64 (x NaN on failed steps), keep (B,N) bool (the paths the exact checks keep), and with port:
    wealth (B,N,H), final, drawdown (B,N), wealth_tol, drawdown_tol."""
    start = np.asarray(start, np.float32)
    A = np.exp(np.asarray(log_A, np.float32)).astype(np.float32)
    mean = np.asarray(mean, np.float32).astype(np.float64)
    S, D = mean.shape
    L = scale_matrix(scale, full)
    bq = np.repeat(np.arange(B, dtype=np.uint64) + np.uint64(b0), N)
    nq = np.tile(np.arange(N, dtype=np.uint64) + np.uint64(n0), B)
    P = B * N
    states = np.empty((P, H), np.int64)
    us = np.empty((P, H), np.float32)
    margin = np.full((P, H), np.inf)
    eps = np.empty((P, H, D))
    sp = np.repeat(start, N, axis=0)
    bad = ~((sp >= 0) & np.isfinite(sp)).all(1)
    z = np.zeros(P, np.int64)
    for t in range(H):
        u = uniform_of(path_words(seed, bq, nq, t, 0)[:, 0])
        p = sp if t == 0 else A[z]
        bad = bad | _bad_total(p)
        z, m = draw_rows(np.where(bad[:, None], np.float32(1), p), u)
        states[:, t] = np.where(bad, -1, z)
        us[:, t] = u
        margin[:, t] = np.where(bad, np.inf, m)
        eps[:, t] = normals(seed, bq, nq, t, D)
    zc = np.maximum(states, 0)
    Lz = L[zc]                                             # (P,H,D,D)
    x = mean[zc] + np.einsum("phij,phj->phi", Lz, eps)
    xtol = 1e-5 * np.abs(Lz).sum(3) + 1e-6 * (np.abs(mean[zc]) + np.einsum("phij,phj->phi", np.abs(Lz), np.abs(eps)))
    x[states < 0] = np.nan
    out = {"states": states.reshape(B, N, H), "u": us.reshape(B, N, H), "margin": margin.reshape(B, N, H),
           "eps": eps.reshape(B, N, H, D), "x": x.reshape(B, N, H, D), "xtol": xtol.reshape(B, N, H, D),
           "keep": (margin.min(1) >= MARGIN).reshape(B, N)}
    if port is not None:
        wealth, final, dd, (rets, helds) = wealth_ref(x, states, port, rebalance, tx_cost)
        wtol, ddtol = wealth_bound(wealth, rets, helds, xtol)
        out.update(wealth=wealth.reshape(B, N, H), final=final.reshape(B, N), drawdown=dd.reshape(B, N),
                   wealth_tol=wtol.reshape(B, N, H), drawdown_tol=ddtol.reshape(B, N))
    return out


def scenario_path_loop(start_row, log_A, mean, scale, full, port, rebalance, tx_cost, seed, bq, nq, H):
    """One path (global indices bq, nq), day by day, in the style of the reference's monte_carlo_simulation: a
    regime, a return vector, a portfolio update with rebalancing and costs.  -> (states, x (H,D), wealth (H,),
    final, drawdown); a failed path ends in -1 / NaN."""
    log_A = np.asarray(log_A, np.float32)
    mean = np.asarray(mean, np.float32)
    S, D = mean.shape
    L = scale_matrix(scale, full)
    key = np.array([seed & MASK, (seed >> 32) & MASK], np.uint64)
    portfolio_value, peak, max_drawdown = 1.0, 1.0, 0.0
    current_weights = np.zeros(D)
    current_regime, failed = 0, False
    regimes, returns, path = [], [], []
    for day in range(H):
        word = philox4x32_10(np.array([nq, bq, day, 0], np.uint64), key)[0]
        u = np.float32((int(word) >> 8) * 2.0 ** -24)
        if day == 0:
            row = np.asarray(start_row, np.float32)
            failed = failed or not bool(np.all((row >= 0) & np.isfinite(row)))
            total = np.cumsum(row, dtype=np.float32)[-1]
            if not failed and total > 0 and np.isfinite(total):
                current_regime = _draw_weights(row, u)
            else:
                failed = True
        else:
            row = np.exp(log_A[current_regime]).astype(np.float32)
            total = np.cumsum(row, dtype=np.float32)[-1]
            if total > 0 and np.isfinite(total):
                current_regime = _draw_weights(row, u)
            else:
                failed = True
        if failed:
            regimes.append(-1)
            returns.append(np.full(D, np.nan))
            path.append(np.nan)
            continue
        regimes.append(current_regime)
        if port is not None and day % rebalance == 0:
            target_weights = np.asarray(port, np.float32)[current_regime].astype(np.float64)
            weight_change = np.abs(target_weights - current_weights).sum()
            cost = portfolio_value * float(np.float32(tx_cost)) * weight_change
            portfolio_value -= cost
            current_weights = target_weights
        eps = []
        for j in range((D + 3) // 4):
            w = philox4x32_10(np.array([nq, bq, day, 1 + j], np.uint64), key)
            for wa, wb in ((w[0], w[1]), (w[2], w[3])):
                u1 = ((int(wa) >> 8) + 1) * 2.0 ** -24
                u2 = (int(wb) >> 8) * 2.0 ** -24
                r = np.sqrt(-2.0 * np.log(u1))
                eps += [r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)]
        eps = np.array(eps[:D])
        sampled_returns = mean[current_regime].astype(np.float64) + L[current_regime] @ eps
        returns.append(sampled_returns)
        if port is not None:
            port_return = (current_weights * sampled_returns).sum()
            portfolio_value *= (1 + port_return)
            peak = max(peak, portfolio_value)
            max_drawdown = max(max_drawdown, 1.0 - portfolio_value / peak)
        path.append(portfolio_value)
    final = np.nan if failed else portfolio_value
    return (np.array(regimes), np.array(returns), np.array(path), final, np.nan if failed else max_drawdown)


def _draw_weights(p, u):
    """gauss_hmm_ref._draw's rule on linear weights, one row (the scalar twin of draw_rows)."""
    run = np.float32(0)
    total = np.cumsum(p, dtype=np.float32)[-1]
    last = 0
    for k in range(len(p)):
        run = np.float32(run + p[k])
        if p[k] > 0:
            last = k
            if u < np.float32(run / total):
                return k
    return last


def make_case(seed, S, D, full, zero_frac=0.0):
    """A random row-normalised model: (log_A (S,S), mean (S,D), scale) fp32 with returns of a percent or so per
    step (mean ~ 1e-3, sd ~ 1e-2), so that wealth stays positive; zero_frac of the transitions are structural
    zeros (-inf), never a whole row."""
    rng = np.random.default_rng(seed)
    A = rng.random((S, S)) + 0.2
    if zero_frac > 0:
        A[rng.random((S, S)) < zero_frac] = 0.0
        A[np.arange(S), np.arange(S)] += 0.3
    with np.errstate(divide="ignore"):
        log_A = np.log(A / A.sum(1, keepdims=True)).astype(np.float32)
    mean = (1e-3 * rng.standard_normal((S, D))).astype(np.float32)
    if full:
        M = rng.standard_normal((S, D, D)) / np.sqrt(D)
        scale = np.tril(1e-2 * (M + 1.5 * np.eye(D))).astype(np.float32)
        scale[:, np.arange(D), np.arange(D)] = np.abs(scale[:, np.arange(D), np.arange(D)]) + 1e-3
        scale += np.triu(np.full((D, D), 7.0, np.float32), 1)   # the strict upper triangle must not be read
    else:
        scale = (1e-2 * (0.5 + rng.random((S, D)))).astype(np.float32)
    return log_A, mean, scale


def make_start(seed, B, S):
    rng = np.random.default_rng(seed)
    return (rng.random((B, S)) + 0.1).astype(np.float32)   # not normalised: the rule divides by the total


def make_port(seed, S, D):
    rng = np.random.default_rng(seed)
    w = rng.random((S, D)) + 0.1
    w = w / w.sum(1, keepdims=True)
    w[S - 1] *= 0.5    # the last regime holds half in cash
    return w.astype(np.float32)


# (kind, B, N, H, S, D): the exact cases of tests/test_gpu_gauss_scenario.py
EXACT_CASES = [("diag", 2, 32, 48, 1, 1), ("full", 3, 32, 48, 3, 5), ("diag", 2, 64, 40, 8, 64),
               ("full", 2, 64, 40, 8, 32), ("full", 1, 128, 16, 32, 16), ("full", 4, 70, 33, 3, 12)]


def case_inputs(kind, B, N, H, S, D, seed=0):
    full = kind == "full"
    log_A, mean, scale = make_case(100 + seed, S, D, full, zero_frac=0.2 if S >= 3 else 0.0)
    return dict(start=make_start(200 + seed, B, S), log_A=log_A, mean=mean, scale=scale, full=full,
                port=make_port(300 + seed, S, D))
