"""Historical back-test of regime-conditional portfolios (vqhmm_backtest_f32 / vqhmm_backtest_bwd_f32; contract:
include/vqhmm.h, "Historical back-test"): B windows x P policies in one launch, the statistics a performance
report needs, and their gradient with respect to the weight tables."""
import torch

from . import _ext

COLUMNS = ("final", "n", "sum", "sumsq", "n_neg", "sum_neg", "sumsq_neg", "n_pos", "drawdown", "turnover", "t_peak",
           "t_trough")


def _launch_fwd(returns, probs, lengths, weights, rebalance, tx_cost, lag, hard, want_wealth):
    B, T, D = returns.shape
    S, P = probs.shape[2], weights.shape[0]
    dev = returns.device
    stats = torch.empty((B, P, 12), dtype=torch.float64, device=dev)
    wealth = torch.empty((B, P, T), dtype=torch.float32, device=dev) if want_wealth else None
    _ext.check(_ext.load().vqhmm_backtest_f32(
        _ext.ptr(returns), _ext.ptr(probs), _ext.ptr(lengths), _ext.ptr(weights), _ext.ptr(rebalance),
        _ext.ptr(tx_cost), lag, hard, B, T, S, D, P, _ext.ptr(stats), _ext.ptr(wealth), _ext.stream_ptr(dev)),
        "backtest")
    return stats, wealth


class _Backtest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, returns, probs, lengths, rebalance, tx_cost, lag, hard, want_wealth):
        w32 = weights.detach().to(torch.float32).contiguous()
        stats, wealth = _launch_fwd(returns, probs, lengths, w32, rebalance, tx_cost, lag, hard, want_wealth)
        ctx.save_for_backward(w32, returns, probs, lengths, rebalance, tx_cost)
        ctx.cfg = (lag, hard, weights.dtype)
        if wealth is None:
            wealth = torch.empty(0, device=returns.device)
        ctx.mark_non_differentiable(wealth)
        return stats, wealth

    @staticmethod
    def backward(ctx, g_stats, _g_wealth):
        w32, returns, probs, lengths, rebalance, tx_cost = ctx.saved_tensors
        lag, hard, dtype = ctx.cfg
        B, T, D = returns.shape
        S, P = probs.shape[2], w32.shape[0]
        dev = returns.device
        lib = _ext.load()
        g_stats = g_stats.to(torch.float64).contiguous()
        grad = torch.empty((P, S, D), dtype=torch.float64, device=dev)
        nb = lib.vqhmm_backtest_bwd_workspace_size(B, T, S, D, P)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        _ext.check(lib.vqhmm_backtest_bwd_f32(
            _ext.ptr(returns), _ext.ptr(probs), _ext.ptr(lengths), _ext.ptr(w32), _ext.ptr(rebalance),
            _ext.ptr(tx_cost), lag, hard, B, T, S, D, P, _ext.ptr(g_stats), _ext.ptr(grad), _ext.ptr(ws),
            _ext.stream_ptr(dev)), "backtest backward")
        return grad.to(dtype), None, None, None, None, None, None, None, None


class Backtest:
    """What `backtest` returns: stats (B,P,12) fp64 (columns: COLUMNS), a (B,P) view per column under its name
    (final, n, sum, sumsq, n_neg, sum_neg, sumsq_neg, n_pos, drawdown, turnover, t_peak, t_trough), and wealth
    (B,P,T) fp32 or None."""

    def __init__(self, stats, wealth=None):
        self.stats, self.wealth = stats, wealth

    def __getattr__(self, name):
        if name in COLUMNS:
            return self.stats[..., COLUMNS.index(name)]
        raise AttributeError(name)

    def __repr__(self):
        B, P = self.stats.shape[:2]
        return f"Backtest(windows={B}, policies={P}, wealth={'yes' if self.wealth is not None else 'no'})"

    def metrics(self, periods_per_year=252):
        """The performance report of the reference's calculate_metrics as (B,P) fp64 tensors, from `stats` with torch
        ops only (differentiable wherever the columns are): total_return = final - 1, cagr = final^(ppy / n) - 1,
        annual_vol = population std of the step returns x sqrt(ppy), sharpe = mean x ppy / (annual_vol + 1e-8),
        sortino = mean x ppy / (population std of the negative step returns x sqrt(ppy)), that denominator read as
        1e-8 when no step return is negative, max_drawdown, win_rate = n_pos / n; and turnover, downside_dev =
        sqrt(sumsq_neg / n) (the denominator of a Sortino loss on all steps), calmar = mean / drawdown.  cagr
        counts the n steps; the reference counts the points of its wealth path.

        max_drawdown is positive here (the reference prints it negative).  Costs are booked to the step that
        pays them: the step return rho_t includes the cost of a rebalance at t.  The reference differences the
        wealth path it recorded before each day's cost, which books a cost one day later and drops the first
        one; final and total_return are not affected, the per-step moments differ by that shift.  Windows of
        length 0 give NaN ratios; calmar is infinite where the drawdown is 0."""
        s = self
        ppy = float(periods_per_year)
        n = s.n
        mean = s.sum / n
        var = (s.sumsq / n - mean * mean).clamp_min(0.0)
        vol = var.sqrt() * ppy ** 0.5
        nn = s.n_neg
        mneg = s.sum_neg / nn.clamp_min(1.0)
        vneg = (s.sumsq_neg / nn.clamp_min(1.0) - mneg * mneg).clamp_min(0.0)
        vneg = torch.where(nn > 0, vneg, torch.ones_like(vneg))    # no sqrt(0) in the branch that is not taken
        down = torch.where(nn > 0, vneg.sqrt() * ppy ** 0.5, torch.full_like(vneg, 1e-8))
        return {
            "total_return": s.final - 1.0,
            "cagr": s.final ** (ppy / n) - 1.0,
            "annual_vol": vol,
            "sharpe": mean * ppy / (vol + 1e-8),
            "sortino": mean * ppy / down,
            "max_drawdown": s.drawdown,
            "win_rate": s.n_pos / n,
            "turnover": s.turnover,
            "downside_dev": (s.sumsq_neg / n).sqrt(),
            "calmar": mean / s.drawdown,
        }


def _per_policy(what, v, P, dtype, dev, lo):
    t = torch.as_tensor(v)
    if not t.is_cuda and bool((t < lo).any()):    # host values are checked; device values are the caller's
        raise ValueError(f"backtest: {what} must be >= {lo}")
    t = t.to(device=dev)
    if t.dim() == 0:
        t = t.expand(P)
    if t.shape != (P,):
        raise ValueError(f"backtest: {what} must be a scalar or have shape ({P},)")
    return t.to(dtype).contiguous()


def backtest(returns, probs, weights, lengths=None, rebalance=5, tx_cost=1e-3, lag=1, mode="soft",
             return_wealth=False):
    """Run P regime-conditional policies through B historical windows (one launch) -> Backtest.

    returns (B,T,D) fp32: the assets' step returns.  probs (B,T,S) fp32: a regime distribution per step
    (GaussianHMM.filter's filt, posterior's gamma, an encoder's q), used as given.  weights (S,D) or (P,S,D): the
    holdings per regime.  rebalance, tx_cost: scalars or (P,): a sweep over frequencies and costs is one call.
    On step t >= lag with (t - lag) % rebalance == 0 the portfolio moves to sum_s probs[b, t-lag, s] weights[s]
    (mode="soft") or to the row of the most probable regime (mode="hard"), paying tx_cost per unit of turnover;
    it holds those weights until the next date.

    lag = 1 (the default) trades step t on the distribution of step t - 1, which an investor has when the step
    begins.  lag = 0 reproduces the reference loop, which trades day t on a label that has already seen day
    t's return: a look-ahead that flatters every regime-timing policy.

    When weights requires grad, stats carries the gradient of any function of it (the columns n, n_neg, n_pos,
    t_peak, t_trough are constants), computed by vqhmm_backtest_bwd_f32 and cast to weights.dtype."""
    _ext.require_device(returns, probs, weights)
    if returns.dim() != 3 or probs.dim() != 3 or returns.shape[:2] != probs.shape[:2]:
        raise ValueError("backtest: returns must be (B, T, D) and probs (B, T, S)")
    if returns.dtype != torch.float32 or probs.dtype != torch.float32:
        raise ValueError("backtest: returns and probs must be float32")
    if mode not in ("soft", "hard"):
        raise ValueError("backtest: mode must be 'soft' or 'hard'")
    B, T, D = returns.shape
    S = probs.shape[2]
    dev = returns.device
    w = weights if weights.dim() == 3 else weights.unsqueeze(0)
    if w.dim() != 3 or w.shape[1:] != (S, D):
        raise ValueError(f"backtest: weights must have shape ({S}, {D}) or (P, {S}, {D})")
    if not (1 <= S <= 32 and 1 <= D <= 64):
        raise ValueError("backtest: needs 1 <= S <= 32 and 1 <= D <= 64")
    P = w.shape[0]
    lag = int(lag)
    if lag < 0:
        raise ValueError("backtest: lag must be >= 0")
    reb = _per_policy("rebalance", rebalance, P, torch.int32, dev, 1)
    txc = _per_policy("tx_cost", tx_cost, P, torch.float32, dev, 0)
    if lengths is not None:
        if lengths.shape != (B,) or lengths.dtype != torch.int64:
            raise ValueError(f"backtest: lengths must be a ({B},) int64 tensor")
        _ext.require_device(lengths)
        lengths = lengths.contiguous()
    returns, probs = returns.detach().contiguous(), probs.detach().contiguous()
    hard = int(mode == "hard")
    if w.requires_grad and torch.is_grad_enabled():
        stats, wealth = _Backtest.apply(w, returns, probs, lengths, reb, txc, lag, hard, bool(return_wealth))
        wealth = wealth if return_wealth else None
    else:
        with torch.no_grad():
            stats, wealth = _launch_fwd(returns, probs, lengths, w.detach().to(torch.float32).contiguous(), reb, txc,
                                        lag, hard, bool(return_wealth))
    return Backtest(stats, wealth)
