"""Numpy fp64 reference of vqhmm_backtest_f32 / vqhmm_backtest_bwd_f32 (contract: include/vqhmm.h, "Historical
back-test").

backtest_ref: the contract's recursion, vectorised over windows x policies (a Python loop over the steps only), ->
stats (B,P,12), wealth (B,P,T) and the per-step quantities the bounds and the gradient take.
reference_order_loop: one window, one policy, day by day in the order of the reference's backtest(): per-step
target weights, a list of portfolio values whose last entry pays the day's cost before the day's return is
applied, and the list without its last entry as the result.  Written separately; the vectorised form must agree.
backtest_grad_ref: dLoss/dweights from dLoss/dstats by the contract's formulas (a_t, u_k, abar_k), date by date.
backtest_torch: the recursion in torch fp64 (differentiable), which the analytic gradient is checked against.

Bounds (derived, not fitted): tol = 4 (T + S + D + B + 8) 2^-53 mag, the first-order fp64 bound of a sum or
product of that many roundings with a factor 4, mag = the sum of the absolute values of the terms that enter the
output:
  1 + rho_t = (1 - c tau_t)(1 + g_t): terms_t = (1 + c sum_d (|q| |W| + |q'| |W|)_d) (1 + sum_d |q| |W| |r|_d);
  final, wealth[t]: |V_t| sum_{u <= t} terms_u / |1 + rho_u|;   sum: sum_t (terms_t + 1);
  sumsq: sum_t (2 |rho_t| (terms_t + 1) + rho_t^2), sum_neg / sumsq_neg: the same over the steps with rho_t < 0;
  turnover: sum_t sum_d (|q| |W| + |q'| |W|)_d;   drawdown: 1 + (V_j* / V_i*) (1 + sum_{i* < t <= j*} terms_t / |1 + rho_t|);
  a gradient entry: sum_t A_t |1 - c tau_t| |q_t[s]| |r[t,d]| + sum_k (|g_turnover| + c (1 + |g_k|) A_k) |q_k[s] -
    q_{k-1}[s]|, with A_t the sum of the absolute values of a_t's terms.
"""
import numpy as np

COLS = ("final", "n", "sum", "sumsq", "n_neg", "sum_neg", "sumsq_neg", "n_pos", "drawdown", "turnover", "t_peak",
        "t_trough")
INT_COLS = (1, 4, 7, 10, 11)
REAL_COLS = (0, 2, 3, 5, 6, 8, 9)
U = 2.0 ** -53


def rule(T, S, D, B):
    return 4.0 * (T + S + D + B + 8) * U


def _lengths(lengths, B, T):
    return np.full(B, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)


def _targets(q, W, hard):
    """q (B,S) fp64, W (P,S,D) fp64 -> (target (B,P,D), abs-term sums (B,P,D), rows (B,) or None)."""
    if hard:
        a = q.argmax(1)                      # the lowest index among equal maxima
        return W[:, a].transpose(1, 0, 2), np.abs(W[:, a]).transpose(1, 0, 2), a
    return np.einsum("bs,psd->bpd", q, W), np.einsum("bs,psd->bpd", np.abs(q), np.abs(W)), None


def backtest_ref(returns, probs, lengths, weights, rebalance, tx_cost, lag, hard):
    """-> dict(stats (B,P,12), wealth (B,P,T), tol_stats (B,P,12), tol_wealth (B,P,T), rho, g, tau, terms (B,P,T))."""
    r = np.asarray(returns, np.float32).astype(np.float64)
    q = np.asarray(probs, np.float32).astype(np.float64)
    W = np.asarray(weights, np.float32).astype(np.float64)
    B, T, D = r.shape
    S, P = q.shape[2], W.shape[0]
    L = _lengths(lengths, B, T)
    R = np.asarray(rebalance, np.int64).reshape(P)
    c = np.asarray(tx_cost, np.float32).astype(np.float64).reshape(P)
    V = np.ones((B, P)); peak = np.ones((B, P)); dd = np.zeros((B, P))
    ipk = np.full((B, P), -1.0); ist = np.full((B, P), -1.0); jst = np.full((B, P), -1.0)
    held = np.zeros((B, P, D)); habs = np.zeros((B, P, D))
    st = np.zeros((B, P, 12))
    wealth = np.zeros((B, P, T))
    rho_t = np.zeros((B, P, T)); g_t = np.zeros((B, P, T)); tau_t = np.zeros((B, P, T)); terms_t = np.ones((B, P, T))
    tabs_t = np.zeros((B, P, T))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(T):
            live = (t < L)[:, None]                                       # (B,1)
            tau = np.zeros((B, P)); tabs = np.zeros((B, P))
            if t >= lag:
                reb = ((t - lag) % R == 0)[None, :] & live                 # (B,P)
                target, tabs_d, _ = _targets(q[:, t - lag], W, hard)
                tau = np.where(reb, np.abs(target - held).sum(2), 0.0)
                tabs = np.where(reb, (tabs_d + habs).sum(2), 0.0)
                held = np.where(reb[..., None], target, held)
                habs = np.where(reb[..., None], tabs_d, habs)
            g = (held * r[:, t, None, :]).sum(2)
            gabs = (habs * np.abs(r[:, t, None, :])).sum(2)
            rho = np.where(live, (1.0 - c * tau) * (1.0 + g) - 1.0, 0.0)
            V = np.where(live, V * (1.0 + rho), V)
            up = live & (V > peak)
            peak = np.where(up, V, peak); ipk = np.where(up, t, ipk)
            d = 1.0 - V / peak
            deeper = live & (V < peak) & (d > dd)
            dd = np.where(deeper, d, dd); ist = np.where(deeper, ipk, ist); jst = np.where(deeper, t, jst)
            wealth[:, :, t] = np.where(live, V, 0.0)
            rho_t[:, :, t], g_t[:, :, t], tau_t[:, :, t] = rho, np.where(live, g, 0.0), tau
            terms_t[:, :, t] = np.where(live, (1.0 + c * tabs) * (1.0 + gabs), 0.0)
            tabs_t[:, :, t] = tabs
            neg, pos = live & (rho < 0), live & (rho > 0)
            st[..., 2] += rho; st[..., 3] += rho * rho
            st[..., 4] += neg; st[..., 5] += np.where(neg, rho, 0.0); st[..., 6] += np.where(neg, rho * rho, 0.0)
            st[..., 7] += pos; st[..., 9] += tau
        st[..., 0], st[..., 1], st[..., 8], st[..., 10], st[..., 11] = V, L[:, None], dd, ist, jst
        # ---- bounds
        valid = (np.arange(T)[None, :] < L[:, None])[:, None, :]           # (B,1,T)
        rel = np.where(valid, terms_t / np.abs(1.0 + rho_t), 0.0)
        crel = np.cumsum(rel, axis=2)
        rt = np.where(valid, terms_t + 1.0, 0.0)
        sq = 2.0 * np.abs(rho_t) * rt + rho_t * rho_t
        negm = valid & (rho_t < 0)
        mag = np.zeros((B, P, 12))
        mag[..., 0] = np.abs(V) * (crel[..., -1] if T else 0.0)
        mag[..., 2] = rt.sum(2); mag[..., 3] = sq.sum(2)
        mag[..., 5] = np.where(negm, rt, 0.0).sum(2); mag[..., 6] = np.where(negm, sq, 0.0).sum(2)
        mag[..., 9] = tabs_t.sum(2)
        tt = np.arange(T)[None, None, :]
        inside = (tt > ist[..., None]) & (tt <= jst[..., None])
        mag[..., 8] = 1.0 + (1.0 - dd) * (1.0 + np.where(inside, rel, 0.0).sum(2))
        k = rule(T, S, D, B)
        tol_wealth = k * np.abs(wealth) * crel + np.abs(wealth) * 2.0 ** -24    # ... and the one fp32 rounding
    bad = np.zeros(B, bool)
    for b in range(B):
        bad[b] = not (np.isfinite(r[b, :L[b]]).all() and np.isfinite(q[b, :L[b]]).all())
    st[bad] = np.nan
    wealth[bad] = np.where(np.arange(T)[None, :] < L[bad][:, None], np.nan, 0.0)[:, None, :]
    return dict(stats=st, wealth=wealth, tol_stats=k * mag, tol_wealth=tol_wealth, rho=rho_t, g=g_t, tau=tau_t,
                terms=terms_t)


def reference_order_loop(returns, targets, rebalance_freq, tx_cost, initial_capital=100000.0, lag=0):
    """One window in the reference's order.  returns (T,D), targets (T,D): the target weights the policy would
    take on the distribution of each day.  -> (portfolio_value without its last entry (T,), the dropped last
    entry, the value after each day's return (T,))."""
    returns = np.asarray(returns, np.float64)
    portfolio_value = [float(initial_capital)]
    current_weights = np.zeros(returns.shape[1])
    after = []
    for day in range(len(returns)):
        if day >= lag and (day - lag) % rebalance_freq == 0:
            target_weights = np.asarray(targets[day - lag], np.float64)
            weight_change = np.abs(target_weights - current_weights).sum()
            cost = portfolio_value[-1] * weight_change * tx_cost
            current_weights = target_weights
            portfolio_value[-1] -= cost
        port_return = (current_weights * returns[day]).sum()
        portfolio_value.append(portfolio_value[-1] * (1 + port_return))
        after.append(portfolio_value[-1])
    return np.array(portfolio_value[:-1]), portfolio_value[-1], np.array(after)


def step_targets(probs_b, W_p, hard):
    """The per-step target weights (T,D) of one window and one policy."""
    q = np.asarray(probs_b, np.float32).astype(np.float64)
    W = np.asarray(W_p, np.float32).astype(np.float64)
    return W[q.argmax(1)] if hard else q @ W


def backtest_grad_ref(returns, probs, lengths, weights, rebalance, tx_cost, lag, hard, grad_stats, fwd=None):
    """-> (grad_weights (P,S,D), tol (P,S,D)) by the contract's formulas, date by date."""
    r = np.asarray(returns, np.float32).astype(np.float64)
    q = np.asarray(probs, np.float32).astype(np.float64)
    W = np.asarray(weights, np.float32).astype(np.float64)
    G = np.asarray(grad_stats, np.float64)
    B, T, D = r.shape
    S, P = q.shape[2], W.shape[0]
    L = _lengths(lengths, B, T)
    R = np.asarray(rebalance, np.int64).reshape(P)
    c = np.asarray(tx_cost, np.float32).astype(np.float64).reshape(P)
    f = fwd if fwd is not None else backtest_ref(returns, probs, lengths, weights, rebalance, tx_cost, lag, hard)
    st, rho_all, g_all, tau_all = f["stats"], f["rho"], f["g"], f["tau"]
    dW = np.zeros((P, S, D)); mag = np.zeros((P, S, D))
    for b in range(B):
        n = int(L[b])
        for p in range(P):
            gs = G[b, p]
            rho, g, tau = rho_all[b, p, :n], g_all[b, p, :n], tau_all[b, p, :n]
            VL, dd, i_s, j_s = st[b, p, 0], st[b, p, 8], st[b, p, 10], st[b, p, 11]
            tt = np.arange(n)
            with np.errstate(invalid="ignore", divide="ignore"):
                parts = [np.full(n, gs[2]), 2 * rho * gs[3], np.where(rho < 0, gs[5] + 2 * rho * gs[6], 0.0),
                         gs[0] * VL / (1 + rho),
                         -gs[8] * ((tt > i_s) & (tt <= j_s)) * (1.0 - dd) / (1 + rho)]
            a = sum(parts)
            A = sum(np.abs(x) for x in parts)
            dates = [t for t in range(lag, n) if (t - lag) % R[p] == 0]
            if not dates:
                continue
            rows = [q[b, t - lag] for t in dates]
            if hard:
                rows = [np.eye(S)[np.argmax(x)] for x in rows]
            hs = [x @ W[p] for x in rows]
            u = [gs[9] - c[p] * (1 + g[t]) * a[t] for t in dates]
            uabs = [abs(gs[9]) + c[p] * (1 + abs(g[t])) * A[t] for t in dates]
            sgn = [np.sign(hs[k] - (hs[k - 1] if k else 0.0)) for k in range(len(dates))]
            for k, t in enumerate(dates):
                end = dates[k + 1] if k + 1 < len(dates) else n
                keep = 1 - c[p] * tau[t:end]
                abar = ((a[t:end] * keep)[:, None] * r[b, t:end]).sum(0) + u[k] * sgn[k]
                aabs = ((A[t:end] * np.abs(keep))[:, None] * np.abs(r[b, t:end])).sum(0) + uabs[k] * np.abs(sgn[k])
                if k + 1 < len(dates):
                    abar = abar - u[k + 1] * sgn[k + 1]
                    aabs = aabs + uabs[k + 1] * np.abs(sgn[k + 1])
                dW[p] += np.outer(rows[k], abar)
                mag[p] += np.outer(np.abs(rows[k]), aabs)
    return dW, rule(T, S, D, B) * mag


def backtest_torch(returns, probs, lengths, weights, rebalance, tx_cost, lag, hard):
    """The recursion in torch fp64 on the tensors' device, differentiable in weights (P,S,D) -> stats (B,P,12).
    A Python loop over the steps."""
    import torch
    r, q, W = returns.double(), probs.double(), weights.double()
    B, T, D = r.shape
    P = W.shape[0]
    dev = r.device
    L = torch.full((B,), T, device=dev) if lengths is None else lengths.clamp(0, T)
    R = torch.as_tensor(rebalance, device=dev).reshape(P)
    c = torch.as_tensor(tx_cost, device=dev).float().double().reshape(P)
    one = torch.ones((B, P), dtype=torch.float64, device=dev)
    V, peak, dd = one, one.clone(), 0 * one
    ipk, ist, jst = -one, -one, -one
    held = torch.zeros((B, P, D), dtype=torch.float64, device=dev)
    s_sum = s_sq = s_nneg = s_neg = s_sqneg = s_npos = s_turn = 0 * one
    for t in range(T):
        live = (t < L)[:, None]
        tau = 0 * one
        if t >= lag:
            reb = ((t - lag) % R == 0)[None, :] & live
            if hard:
                target = W[:, q[:, t - lag].argmax(1)].transpose(0, 1)
            else:
                target = torch.einsum("bs,psd->bpd", q[:, t - lag], W)
            tau = torch.where(reb, (target - held).abs().sum(2), 0 * one)
            held = torch.where(reb[..., None], target, held)
        g = (held * r[:, t, None, :]).sum(2)
        rho = torch.where(live, (1 - c * tau) * (1 + g) - 1, 0 * one)
        V = V * (1 + rho)
        up = live & (V > peak)
        peak = torch.where(up, V, peak); ipk = torch.where(up, t * one, ipk)
        d = 1 - V / peak
        deeper = live & (V < peak) & (d > dd)
        dd = torch.where(deeper, d, dd); ist = torch.where(deeper, ipk, ist); jst = torch.where(deeper, t * one, jst)
        neg = live & (rho < 0)
        s_sum = s_sum + rho; s_sq = s_sq + rho * rho
        s_nneg = s_nneg + neg; s_neg = s_neg + torch.where(neg, rho, 0 * one)
        s_sqneg = s_sqneg + torch.where(neg, rho * rho, 0 * one)
        s_npos = s_npos + (live & (rho > 0)); s_turn = s_turn + tau
    n = (L.double()[:, None] * one)
    return torch.stack([V, n, s_sum, s_sq, s_nneg, s_neg, s_sqneg, s_npos, dd, s_turn, ist.detach(), jst.detach()], -1)


def make_case(seed, B, T, S, D, P, lengths=None):
    """Returns ~ N(1e-3, 1e-2); probs = softmax rows with persistence; weights: long-only rows summing to 1, every
    third policy with signed rows; rebalance and tx_cost mixed per policy (tx_cost 0 among them); ragged lengths
    unless given."""
    rng = np.random.default_rng(seed)
    returns = (1e-3 + 1e-2 * rng.standard_normal((B, T, D))).astype(np.float32)
    logit = np.zeros((B, T, S))
    z = rng.standard_normal((B, S))
    for t in range(T):
        z = 0.9 * z + 0.6 * rng.standard_normal((B, S))
        logit[:, t] = 2.0 * z
    e = np.exp(logit - logit.max(2, keepdims=True))
    probs = (e / e.sum(2, keepdims=True)).astype(np.float32)
    w = rng.random((P, S, D)) + 0.1
    w = w / w.sum(2, keepdims=True)
    w[2::3] = 0.3 * rng.standard_normal((len(w[2::3]), S, D))
    reb = np.array([[1, 5, 7, 64, 1000][i % 5] for i in range(P)], np.int32)
    txc = np.array([[1e-3, 0.0, 5e-3, 2e-4][i % 4] for i in range(P)], np.float32)
    if lengths is None:
        lengths = rng.integers(max(T // 2, 1) if T else 0, T + 1, size=B)
        if B:
            lengths[0] = T
    return dict(returns=returns, probs=probs, lengths=np.asarray(lengths, np.int64), weights=w.astype(np.float32),
                rebalance=reb, tx_cost=txc)


def objective(metrics, stats):
    """-sharpe + 0.1 drawdown + 0.01 turnover - log final + sortino, summed over windows x policies."""
    import torch
    return (-metrics["sharpe"] + 0.1 * stats[..., 8] + 0.01 * stats[..., 9] - torch.log(stats[..., 0])
            + metrics["sortino"]).sum()
