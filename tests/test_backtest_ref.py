"""CPU checks of the historical back-test's reference (tests/backtest_ref.py), of Backtest.metrics and of the host
side of vqhmm_backtest_f32 / vqhmm_backtest_bwd_f32.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import backtest_ref as BR


def _case(seed=0, B=3, T=40, S=3, D=4, P=6, **kw):
    return BR.make_case(seed, B, T, S, D, P, **kw)


@pytest.mark.parametrize("hard", [0, 1])
@pytest.mark.parametrize("lag", [0, 1, 3])
def test_vectorised_equals_scalar_loop(lag, hard):
    """Final wealth and the wealth path of the vectorised recursion against the day-by-day loop, 1e-12 relative; at
    lag = 0 the loop is the reference's order, and its portfolio_value list (each entry paying the next day's cost
    before that day's return, the last entry dropped) is wealth[t] / (1 + g_t)."""
    c = _case(seed=lag + 10 * hard)
    f = BR.backtest_ref(lag=lag, hard=hard, **c)
    capital = 100000.0
    for b in range(3):
        n = int(c["lengths"][b])
        for p in range(6):
            tg = BR.step_targets(c["probs"][b, :n], c["weights"][p], hard)
            path, last, after = BR.reference_order_loop(c["returns"][b, :n].astype(np.float64), tg,
                                                        int(c["rebalance"][p]), float(c["tx_cost"][p]), capital, lag)
            assert abs(last / capital - f["stats"][b, p, 0]) <= 1e-12 * abs(f["stats"][b, p, 0])
            np.testing.assert_allclose(after / capital, f["wealth"][b, p, :n], rtol=1e-12, atol=0)
            assert len(path) == n and path[0] <= capital
            np.testing.assert_allclose(path * (1 + f["g"][b, p, :n]) / capital, f["wealth"][b, p, :n], rtol=1e-12)
            assert np.all(f["wealth"][b, p, n:] == 0)


def test_equal_weight_buy_and_hold():
    """weights = 1 / D in every row, one purchase, no cost: the wealth path is cumprod(1 + mean_d r).  D = 4, so 1 / D
    is exact in fp32; mode hard, so the holdings are a row of the table and not a sum of probs that is 1 only up to
    fp32 rounding (soft agrees to that rounding)."""
    c = _case(seed=3, P=1)
    D = c["returns"].shape[2]
    assert D == 4
    w = np.full((1, 3, D), 1.0 / D, np.float32)
    expect = np.cumprod(1 + c["returns"].astype(np.float64).mean(2), axis=1)
    f = BR.backtest_ref(c["returns"], c["probs"], None, w, [1000], [0.0], lag=0, hard=1)
    np.testing.assert_allclose(f["wealth"][:, 0], expect, rtol=1e-12)
    np.testing.assert_allclose(f["stats"][:, 0, 0], expect[:, -1], rtol=1e-12)
    assert np.all(f["stats"][:, 0, 9] == 1.0)                     # one purchase of the whole book
    soft = BR.backtest_ref(c["returns"], c["probs"], None, w, [1000], [0.0], lag=0, hard=0)
    np.testing.assert_allclose(soft["wealth"][:, 0], expect, rtol=1e-5)


@pytest.mark.parametrize("hard", [0, 1])
def test_analytic_gradient_equals_autograd(hard):
    import vqhmm
    c = _case(seed=5 + hard, B=3, T=48, S=3, D=4, P=5)
    c["lengths"] = np.array([48, 30, 17], np.int64)
    lag = 1
    W = torch.tensor(c["weights"], dtype=torch.float64, requires_grad=True)
    st = BR.backtest_torch(torch.tensor(c["returns"]), torch.tensor(c["probs"]), torch.tensor(c["lengths"]), W,
                           c["rebalance"], c["tx_cost"], lag, hard)
    st.retain_grad()
    f = BR.backtest_ref(lag=lag, hard=hard, **c)
    np.testing.assert_allclose(st.detach().numpy(), f["stats"], rtol=1e-11, atol=1e-13)
    obj = BR.objective(vqhmm.Backtest(st).metrics(), st)
    obj.backward()
    g, _ = BR.backtest_grad_ref(lag=lag, hard=hard, grad_stats=st.grad.numpy(), fwd=f, **c)
    ref = W.grad.numpy()
    assert np.abs(ref).max() > 0
    err = np.abs(g - ref).max() / np.abs(ref).max()
    assert err <= 1e-9, err


def test_metrics_match_calculate_metrics_restatement():
    """metrics() against a restatement of the reference's calculate_metrics on the wealth path [1, V_0, ..., V_{L-1}],
    with one rebalance at step 0 and no cost, so both bookkeepings of the costs coincide."""
    import vqhmm
    c = _case(seed=9, B=2, T=60, P=2)
    f = BR.backtest_ref(c["returns"], c["probs"], None, c["weights"][:2], [1000, 1000], [0.0, 0.0], lag=0, hard=0)
    m = vqhmm.Backtest(torch.tensor(f["stats"])).metrics()
    for b in range(2):
        for p in range(2):
            pv = np.concatenate([[1.0], f["wealth"][b, p]])
            rets = np.diff(pv) / pv[:-1]
            total_return = pv[-1] / pv[0] - 1
            cagr = (1 + total_return) ** (1 / (len(rets) / 252)) - 1
            annual_vol = rets.std() * np.sqrt(252)
            sharpe = rets.mean() * 252 / (annual_vol + 1e-8)
            cummax = np.maximum.accumulate(pv)
            max_drawdown = ((pv - cummax) / cummax).min()
            down = rets[rets < 0]
            downside_std = down.std() * np.sqrt(252) if len(down) > 0 else 1e-8
            sortino = rets.mean() * 252 / downside_std
            win_rate = (rets > 0).sum() / len(rets)
            want = dict(total_return=total_return, cagr=cagr, annual_vol=annual_vol, sharpe=sharpe, sortino=sortino,
                        max_drawdown=-max_drawdown, win_rate=win_rate,
                        downside_dev=np.sqrt((np.minimum(rets, 0) ** 2).mean()), calmar=rets.mean() / -max_drawdown,
                        turnover=f["stats"][b, p, 9])
            for k, v in want.items():
                assert abs(float(m[k][b, p]) - v) <= 1e-9 * max(abs(v), 1e-3), (k, float(m[k][b, p]), v)


def test_entries_and_host_return_codes():
    """The entries exist with the ABI at 8; the header's order of host codes: a negative size -> EINVAL, the domain
    -> EUNSUPPORTED, an empty problem -> OK without a launch, a null required pointer -> EINVAL.  The values of
    rebalance are device data and are not looked at.  None of these reaches a launch."""
    from vqhmm import _ext
    lib = _ext.load()
    assert lib.vqhmm_abi_version() == 8
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(ret=p, probs=p, lengths=None, W=p, reb=p, tx=p, lag=1, hard=0, B=2, T=5, S=3, D=4, P=2, stats=p,
            wealth=None):
        return lib.vqhmm_backtest_f32(ret, probs, lengths, W, reb, tx, lag, hard, B, T, S, D, P, stats, wealth, None)

    def bwd(ret=p, probs=p, lengths=None, W=p, reb=p, tx=p, lag=1, hard=0, B=2, T=5, S=3, D=4, P=2, gs=p, gw=p,
            ws=p):
        return lib.vqhmm_backtest_bwd_f32(ret, probs, lengths, W, reb, tx, lag, hard, B, T, S, D, P, gs, gw, ws,
                                          None)

    EINVAL, EUNS, OK = -1, -4, 0
    for call in (fwd, bwd):
        for neg in ("B", "T", "S", "D", "P", "lag"):
            assert call(**{neg: -1}) == EINVAL
        assert call(B=-1, S=99) == EINVAL
        for dom in (dict(S=0), dict(S=33), dict(D=0), dict(D=65), dict(T=(1 << 28) + 1), dict(B=1 << 20, P=1 << 12)):
            assert call(**dom) == EUNS
        assert call(S=33, B=0) == EUNS
        assert call(P=0, W=None, reb=None, tx=None) == OK
        for null in ("W", "reb", "tx", "ret", "probs"):
            assert call(**{null: None}) == EINVAL
    assert fwd(B=0, stats=None, W=None) == OK
    assert fwd(stats=None) == EINVAL
    assert bwd(gw=None) == EINVAL and bwd(gs=None) == EINVAL and bwd(ws=None) == EINVAL
    size = lib.vqhmm_backtest_bwd_workspace_size
    assert size(17, 100, 3, 12, 5) == 3 * 5 * 3 * 12 * 8      # ceil(17 / 8) tiles of fp64 (P,S,D) partials
    assert size(0, 100, 3, 12, 5) == 0 and size(4, 100, 33, 12, 5) == 0 and size(4, 100, 3, 65, 5) == 0
    assert size(-1, 100, 3, 12, 5) == 0
