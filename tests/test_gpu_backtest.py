"""vqhmm_backtest_f32 / vqhmm_backtest_bwd_f32 on the GPU against tests/backtest_ref.py: the statistics and the
wealth path within the derived fp64 bounds (integer columns exactly), the bit-for-bit independence of a window
and a policy from the rest of the call, NaN windows, graph capture, the gradient, and the Python surface."""
import functools

import numpy as np
import pytest
import torch

import backtest_ref as BR
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu

# (B, T, S, D, P); the last with lengths (70, 0, 1, 37)
CASES = [(3, 1, 1, 1, 1), (2, 63, 3, 5, 5), (2, 64, 3, 12, 4), (3, 65, 8, 16, 3), (2, 130, 2, 3, 7),
         (1, 200, 32, 64, 2), (4, 70, 3, 12, 9)]
RAGGED = (70, 0, 1, 37)
BWD_CASES = [(2, 64, 3, 12, 4), (3, 130, 8, 16, 3), (1, 200, 32, 64, 2), (4, 70, 3, 12, 9)]


@functools.lru_cache(maxsize=None)
def case(shape):
    B, T, S, D, P = shape
    c = BR.make_case(sum(shape), B, T, S, D, P, lengths=RAGGED if shape == (4, 70, 3, 12, 9) else None)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ref(shape, lag, hard):
    return BR.backtest_ref(lag=lag, hard=hard, **case(shape))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()    # a copy: the cached cases are read-only


def run_fwd(c, lag, hard, want_wealth=True):
    """Through ctypes on guarded exact-size buffers (gpu_buffers.guarded) pre-filled with 7 -> (stats, wealth or
    None) as numpy."""
    from vqhmm import _ext
    lib = _ext.load()
    B, T, D = c["returns"].shape
    S, P = c["probs"].shape[2], c["weights"].shape[0]
    d = {k: dev(c[k]) for k in ("returns", "probs", "weights", "rebalance", "tx_cost")}
    lengths = dev(c["lengths"]) if c.get("lengths") is not None else None
    stats = guarded((B, P, 12), torch.float64, fill=7.0)
    wealth = guarded((B, P, T), torch.float32, fill=7.0) if want_wealth else None
    rc = lib.vqhmm_backtest_f32(_ext.ptr(d["returns"]), _ext.ptr(d["probs"]), _ext.ptr(lengths), _ext.ptr(d["weights"]),
                                _ext.ptr(d["rebalance"]), _ext.ptr(d["tx_cost"]), lag, hard, B, T, S, D, P,
                                stats.ptr, wealth.ptr if want_wealth else None, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(stats, wealth)
    return stats.t.cpu().numpy(), (wealth.t.cpu().numpy() if want_wealth else None)


def run_bwd(c, lag, hard, gstats):
    from vqhmm import _ext
    lib = _ext.load()
    B, T, D = c["returns"].shape
    S, P = c["probs"].shape[2], c["weights"].shape[0]
    d = {k: dev(c[k]) for k in ("returns", "probs", "weights", "rebalance", "tx_cost")}
    lengths = dev(c["lengths"]) if c.get("lengths") is not None else None
    g = dev(np.asarray(gstats, np.float64))
    grad = guarded((P, S, D), torch.float64, fill=7.0)
    nb = lib.vqhmm_backtest_bwd_workspace_size(B, T, S, D, P)
    ws = guarded(nb, torch.uint8)  # exactly the queried size, poisoned
    rc = lib.vqhmm_backtest_bwd_f32(_ext.ptr(d["returns"]), _ext.ptr(d["probs"]), _ext.ptr(lengths),
                                    _ext.ptr(d["weights"]), _ext.ptr(d["rebalance"]), _ext.ptr(d["tx_cost"]), lag, hard,
                                    B, T, S, D, P, _ext.ptr(g), grad.ptr, ws.ptr, _ext.stream_ptr())
    assert rc == 0, rc
    check_all(grad, ws)
    return grad.t.cpu().numpy()


def check_fwd(got_stats, got_wealth, f, what):
    """Integer columns exactly, the rest and the wealth path within the derived bound -> the largest err / bound."""
    st, tol = f["stats"], f["tol_stats"]
    for col in BR.INT_COLS:
        assert np.array_equal(got_stats[..., col], st[..., col]), (what, BR.COLS[col], got_stats[..., col], st[..., col])
    worst = 0.0
    for col in BR.REAL_COLS:
        err = np.abs(got_stats[..., col] - st[..., col])
        assert np.all(err <= tol[..., col]), (what, BR.COLS[col], err.max(), tol[..., col].min())
        worst = max(worst, float((err / np.maximum(tol[..., col], 1e-300)).max()))
    if got_wealth is not None:
        err = np.abs(got_wealth.astype(np.float64) - f["wealth"])
        assert np.all(err <= f["tol_wealth"]), (what, err.max())
        L = st[..., 1].astype(np.int64)
        for b, p in np.ndindex(L.shape):
            if L[b, p] > 0:   # wealth[L-1] has the bits of (float) final, zeros behind it
                assert got_wealth[b, p, L[b, p] - 1] == np.float32(got_stats[b, p, 0]), (what, b, p)
            assert np.all(got_wealth[b, p, L[b, p]:] == 0), (what, b, p)
    return worst


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_forward(shape):
    """lag in {0, 1, 3, >= L}, soft and hard, rebalance in {1, 5, 7, 64, 1000} and tx_cost = 0 mixed over the policies
    of one call (make_case)."""
    c = case(shape)
    worst = 0.0
    for lag in (0, 1, 3, shape[1] + 2):
        for hard in (0, 1):
            stats, wealth = run_fwd(c, lag, hard)
            worst = max(worst, check_fwd(stats, wealth, ref(shape, lag, hard), (shape, lag, hard)))
            if lag >= shape[1]:   # never trades: flat, rho = 0 exactly
                L = np.clip(c["lengths"], 0, shape[1])[:, None] * np.ones((1, shape[4]))
                want = np.stack([1 + 0 * L, L, 0 * L, 0 * L, 0 * L, 0 * L, 0 * L, 0 * L, 0 * L, 0 * L, -1 + 0 * L,
                                 -1 + 0 * L], -1)
                assert np.array_equal(stats, want)
    print(f"backtest forward {shape}: largest err / bound = {worst:.3f}")


def test_mixed_rebalance_periods_in_one_call():
    """All of R in {1, 5, 7, 64, 1000} in one call at T = 130 (two chunk boundaries, 64 | T - 2)."""
    shape = (2, 130, 2, 3, 7)
    c = dict(case(shape))
    assert set(c["rebalance"].tolist()) == {1, 5, 7, 64, 1000}
    stats, wealth = run_fwd(c, 1, 0)
    check_fwd(stats, wealth, ref(shape, 1, 0), "mixed")
    assert len(set(stats[0, :5, 9].tolist())) == 5    # five different turnovers


def test_hard_ties_and_unchanged_regimes():
    """Exact ties take the lowest index; while the most probable regime does not change, a daily rebalance pays
    tau = 0 exactly, so the turnover is that of the few changes only."""
    B, T, S, D, P = 1, 70, 3, 5, 3
    c = dict(BR.make_case(1, B, T, S, D, P, lengths=(T,)))
    probs = np.zeros((B, T, S), np.float32)
    probs[0, :20] = (0.5, 0.5, 0.0)        # tie -> 0
    probs[0, 20:40] = (0.2, 0.6, 0.2)      # 1
    probs[0, 40:] = (0.3, 0.35, 0.35)      # tie -> 1: unchanged
    c["probs"] = probs
    c["rebalance"] = np.array([1, 1, 7], np.int32)
    c["tx_cost"] = np.array([1e-3, 0.0, 1e-3], np.float32)
    f = BR.backtest_ref(lag=1, hard=1, **c)
    stats, wealth = run_fwd(c, 1, 1)
    check_fwd(stats, wealth, f, "ties")
    W = c["weights"].astype(np.float64)
    want = np.abs(W[0, 0]).sum() + np.abs(W[0, 1] - W[0, 0]).sum()
    assert abs(stats[0, 0, 9] - want) <= 4e-15 * want and abs(f["stats"][0, 0, 9] - want) <= 4e-15 * want
    assert np.count_nonzero(f["tau"][0, 0]) == 2


def pad_T(c, extra, fill=np.nan):
    out = dict(c)
    for k in ("returns", "probs"):
        a = c[k]
        out[k] = np.concatenate([a, np.full((a.shape[0], extra, a.shape[2]), fill, np.float32)], 1)
    return out


@pytest.mark.parametrize("hard", [0, 1])
def test_forward_independence(hard):
    """stats[b, p] and wealth[b, p] bit for bit from a call on a slice of the windows, a slice of the policies, a
    call without wealth, and calls with more T behind the lengths (NaN there: it is not read)."""
    shape = (4, 70, 3, 12, 9)
    c = case(shape)
    stats, wealth = run_fwd(c, 1, hard)
    for lo, hi in ((1, 3), (3, 4), (0, 1)):
        sub = dict(c, **{k: c[k][lo:hi] for k in ("returns", "probs", "lengths")})
        s2, w2 = run_fwd(sub, 1, hard)
        assert np.array_equal(s2, stats[lo:hi]) and np.array_equal(w2, wealth[lo:hi])
    for lo, hi in ((2, 5), (8, 9), (0, 1), (3, 8)):
        sub = dict(c, **{k: c[k][lo:hi] for k in ("weights", "rebalance", "tx_cost")})
        s2, w2 = run_fwd(sub, 1, hard)
        assert np.array_equal(s2, stats[:, lo:hi]) and np.array_equal(w2, wealth[:, lo:hi])
    s2, _ = run_fwd(c, 1, hard, want_wealth=False)
    assert np.array_equal(s2, stats)
    for extra in (1, 58, 64):
        s2, w2 = run_fwd(pad_T(c, extra), 1, hard)
        assert np.array_equal(s2, stats)
        assert np.array_equal(w2[:, :, :70], wealth) and np.all(w2[:, :, 70:] == 0)
    # lengths = NULL is lengths = T
    full = dict(c, lengths=np.full(4, 70, np.int64))
    s_full, w_full = run_fwd(full, 1, hard)
    s_null, w_null = run_fwd(dict(full, lengths=None), 1, hard)
    assert np.array_equal(s_full, s_null) and np.array_equal(w_full, w_null)


def test_nan_windows():
    """A non-finite returns or probs value inside a window's length: all twelve columns NaN for every policy, the
    wealth NaN inside the length; outside the length it is not seen; the other windows keep their bits."""
    shape = (4, 70, 3, 12, 9)
    c = case(shape)
    stats, wealth = run_fwd(c, 1, 0)
    bad = dict(c, returns=c["returns"].copy(), probs=c["probs"].copy())
    bad["returns"][0, 69, 11] = np.nan        # the last value inside length 70
    bad["returns"][2, 1, 0] = np.nan          # length 1: outside
    bad["probs"][2, 5, 2] = np.nan
    bad["returns"][1, 0, 0] = np.nan          # length 0: outside
    bad["probs"][3, 37, 0] = np.nan           # t = 37 is the first row outside length 37
    bad["probs"][3, 12, 1] = np.inf           # inside length 37, not a decision row of every policy
    s2, w2 = run_fwd(bad, 1, 0)
    assert np.isnan(s2[0]).all() and np.isnan(w2[0]).all()
    assert np.isnan(s2[3][..., :]).all() and np.isnan(w2[3, :, :37]).all() and np.all(w2[3, :, 37:] == 0)
    assert np.array_equal(s2[1:3], stats[1:3]) and np.array_equal(w2[1:3], wealth[1:3])
    f = BR.backtest_ref(lag=1, hard=0, **bad)
    assert np.array_equal(np.isnan(f["stats"]), np.isnan(s2))
    only3 = dict(c, probs=bad["probs"])
    s3, _ = run_fwd(only3, 1, 0)
    assert np.array_equal(s3[:3], stats[:3]) and np.isnan(s3[3]).all()


def test_graph_capture():
    """One launch, no workspace, no host sync: captured into a graph, the call replays to the same bits."""
    from vqhmm import _ext
    lib = _ext.load()
    shape = (2, 64, 3, 12, 4)
    c = case(shape)
    B, T, S, D, P = shape
    stats, wealth = run_fwd(c, 1, 0)
    d = [dev(c[k]) for k in ("returns", "probs", "lengths", "weights", "rebalance", "tx_cost")]
    st = torch.zeros((B, P, 12), dtype=torch.float64, device="cuda")
    we = torch.zeros((B, P, T), device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.vqhmm_backtest_f32(*(_ext.ptr(t) for t in d), 1, 0, B, T, S, D, P, _ext.ptr(st), _ext.ptr(we),
                                    _ext.stream_ptr())
    assert rc == 0, rc
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), stats) and np.array_equal(we.cpu().numpy(), wealth)


def check_grad(got, want, tol, what):
    err = np.abs(got - want)
    assert np.all(err <= tol), (what, float(err.max()), float((err / np.maximum(tol, 1e-300)).max()))
    return float((err / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("hard", [0, 1])
@pytest.mark.parametrize("shape", BWD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_backward_random_grad_stats(shape, hard):
    """grad_weights for a random grad_stats within the derived bound; two calls and a policy slice bit for bit."""
    c = case(shape)
    B, T, S, D, P = shape
    gs = np.random.default_rng(7).standard_normal((B, P, 12))
    got = run_bwd(c, 1, hard, gs)
    want, tol = BR.backtest_grad_ref(lag=1, hard=hard, grad_stats=gs, fwd=ref(shape, 1, hard), **c)
    worst = check_grad(got, want, tol, (shape, hard))
    print(f"backtest backward {shape} hard={hard}: largest err / bound = {worst:.3f}")
    assert np.array_equal(run_bwd(c, 1, hard, gs), got)
    lo, hi = (1, 3) if P > 2 else (1, 2)
    sub = dict(c, **{k: c[k][lo:hi] for k in ("weights", "rebalance", "tx_cost")})
    assert np.array_equal(run_bwd(sub, 1, hard, gs[:, lo:hi]), got[lo:hi])


@pytest.mark.parametrize("hard", [0, 1])
@pytest.mark.parametrize("shape", BWD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_backward_objective_through_metrics(shape, hard):
    """-sharpe + 0.1 drawdown + 0.01 turnover - log final + sortino through vqhmm.backtest(...).metrics() with
    weights.requires_grad: weights.grad against the reference's gradient for the grad_stats autograd handed to
    the kernel (windows shorter than 2 steps have no Sharpe ratio and are left out of the objective)."""
    import vqhmm
    c = case(shape)
    L = np.clip(c["lengths"], 0, shape[1])
    W = dev(c["weights"]).double().requires_grad_(True)
    bt = vqhmm.backtest(dev(c["returns"]), dev(c["probs"]), W, lengths=dev(c["lengths"]), rebalance=dev(c["rebalance"]),
                        tx_cost=dev(c["tx_cost"]), lag=1, mode="hard" if hard else "soft")
    assert bt.stats.requires_grad and bt.wealth is None
    bt.stats.retain_grad()
    keep = torch.from_numpy(np.flatnonzero(L >= 2)).cuda()
    sub = vqhmm.Backtest(bt.stats[keep])
    obj = BR.objective(sub.metrics(), sub.stats)
    assert torch.isfinite(obj)
    obj.backward()
    gs = bt.stats.grad.cpu().numpy()
    assert W.grad.dtype == torch.float64 and np.all(gs[L < 2] == 0)
    want, tol = BR.backtest_grad_ref(lag=1, hard=hard, grad_stats=gs, fwd=ref(shape, 1, hard), **c)
    assert np.abs(want).max() > 0
    check_grad(W.grad.cpu().numpy(), want, tol, (shape, hard))
    # the column views and the plain call
    plain = vqhmm.backtest(dev(c["returns"]), dev(c["probs"]), W.detach().float(), lengths=dev(c["lengths"]),
                           rebalance=dev(c["rebalance"]), tx_cost=dev(c["tx_cost"]), lag=1,
                           mode="hard" if hard else "soft", return_wealth=True)
    assert torch.equal(plain.stats, bt.stats.detach()) and not plain.stats.requires_grad
    assert torch.equal(plain.final, plain.stats[..., 0]) and torch.equal(plain.t_trough, plain.stats[..., 11])
    assert plain.wealth.shape == (shape[0], shape[4], shape[1])


def test_backward_zero_drawdown_window():
    """Positive returns, long-only weights, no cost: wealth never falls below its peak, drawdown = 0, (t_peak,
    t_trough) = (-1, -1), and grad_stats' drawdown column moves nothing."""
    B, T, S, D, P = 2, 70, 3, 4, 3
    c = dict(BR.make_case(11, B, T, S, D, P, lengths=(70, 41)))
    c["returns"] = np.abs(c["returns"]) + np.float32(1e-4)
    c["weights"] = np.abs(c["weights"])
    c["tx_cost"] = np.zeros(P, np.float32)
    f = BR.backtest_ref(lag=1, hard=0, **c)
    stats, _ = run_fwd(c, 1, 0, want_wealth=False)
    assert np.all(stats[..., 8] == 0) and np.all(stats[..., 10:] == -1)
    check_fwd(stats, None, f, "zero drawdown")
    gs = np.random.default_rng(3).standard_normal((B, P, 12))
    got = run_bwd(c, 1, 0, gs)
    want, tol = BR.backtest_grad_ref(lag=1, hard=0, grad_stats=gs, fwd=f, **c)
    check_grad(got, want, tol, "zero drawdown")
    gs2 = gs.copy()
    gs2[..., 8] += 5.0
    assert np.array_equal(run_bwd(c, 1, 0, gs2), got)


def hmm_model(cov, S, D, seed):
    import vqhmm
    gen = torch.Generator().manual_seed(seed)
    m = vqhmm.GaussianHMM(S, D, cov, generator=gen)
    with torch.no_grad():
        m.mean.mul_(1e-2)
        if cov == "full":
            m.scale_tril.copy_(1e-2 * (0.3 * torch.randn(S, D, D, generator=gen).tril() + torch.eye(D)))
        else:
            m.log_var.copy_(2 * torch.log(1e-2 * (0.5 + torch.rand(S, D, generator=gen))))
    return m.cuda()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("cov", ["diag", "full"])
def test_module_backtest(cov, causal):
    """GaussianHMM.backtest is vqhmm.backtest on filter's / posterior's output, bit for bit."""
    import vqhmm
    shape = (4, 70, 3, 12, 9)
    c = case(shape)
    m = hmm_model(cov, 3, 12, 2)
    x, lengths, W = dev(c["returns"]), dev(c["lengths"]), dev(c["weights"])
    kw = dict(rebalance=dev(c["rebalance"]), tx_cost=dev(c["tx_cost"]), lag=1, mode="soft", return_wealth=True)
    got = m.backtest(x, x, W, lengths=lengths, causal=causal, **kw)
    probs = m.filter(x, lengths)[0] if causal else m.posterior(x, lengths)
    want = vqhmm.backtest(x, probs, W, lengths=lengths, **kw)
    assert torch.equal(got.stats, want.stats) and torch.equal(got.wealth, want.wealth)
    assert got.stats.shape == (4, 9, 12) and torch.isfinite(got.stats).all()
    single = m.backtest(x, x, W[0], lengths=lengths, causal=causal, rebalance=5, tx_cost=1e-3)
    assert single.stats.shape == (4, 1, 12) and single.wealth is None


def test_adam_lowers_the_objective():
    """Twenty Adam steps on weights (S,D) from equal weight lower the net-of-cost objective."""
    import vqhmm
    shape = (2, 130, 2, 3, 7)
    c = case(shape)
    B, T, S, D, P = shape
    r, q = dev(c["returns"]), dev(c["probs"])
    W = torch.full((S, D), 1.0 / D, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([W], lr=0.02)
    hist = []
    for _ in range(21):
        opt.zero_grad()
        bt = vqhmm.backtest(r, q, W, rebalance=5, tx_cost=1e-3, lag=1)
        obj = BR.objective(bt.metrics(), bt.stats)
        hist.append(float(obj.detach()))
        obj.backward()
        assert W.grad is not None and W.grad.dtype == torch.float32 and torch.isfinite(W.grad).all()
        opt.step()
    print(f"objective: {hist[0]:.6f} -> {hist[-1]:.6f}")
    assert hist[-1] < hist[0]
