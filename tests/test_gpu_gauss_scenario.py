"""GPU checks of vqhmm_gauss_scenario_f32 (hmm_gauss_scenario.hip), GaussianHMM.simulate and scenario_summary
against tests/gauss_scenario_ref.py.

Exact cases: on every path the reference keeps (no regime uniform within 1e-4 of a cdf boundary; at most 25 % of a
case may be left out) the states are equal element for element and |x - x_ref| <= 1e-5 sum_j |L_ij| + 1e-6 (|mean_i|
+ sum_j |L_ij eps_j|) (the reference module derives both terms).  The kernel's wealth, final and drawdown equal the
fp64 recursion applied to the kernel's own x and states to rel 1e-6 on every path, final is bitwise wealth[..., H-1],
and against the independent reference they stay inside the propagated x bound (gauss_scenario_ref.wealth_bound).
Then independence of the batch split and of the requested outputs (bit for bit), the hard cases, the distribution
of a larger batch (5 sigma) and the module surface.
"""
import functools

import numpy as np
import pytest
import torch

import gauss_scenario_ref as R
from gauss_scenario_ref import EXACT_CASES, case_inputs
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu
SEED = 1234
ALL = ("states", "x", "wealth", "final", "drawdown")
# N = 1, and H = 1, 70 (three flushes of the 32-step tile, the last partial) and 130
EXTRA_CASES = [("full", 3, 1, 20, 3, 5), ("diag", 2, 70, 1, 3, 4), ("full", 1, 64, 70, 3, 5), ("diag", 1, 64, 130, 2, 3)]


def dev(a, dtype=np.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype)).cuda()


def run(c, B, N, H, want=ALL, seed=SEED, b0=0, n0=0, reb=5, tx=1e-3, port=True, start=None, log_A=None, rc=0):
    """The entry through ctypes on guarded exact-size buffers (gpu_buffers.guarded) -> dict of numpy arrays; every
    requested output starts as 7 (the call must write every element)."""
    from vqhmm import _ext
    lib = _ext.load()
    S, D = c["mean"].shape
    d_in = [dev(c["start"] if start is None else start), dev(c["log_A"] if log_A is None else log_A), dev(c["mean"]),
            dev(c["scale"])]
    d_port = dev(c["port"]) if port else None
    shapes = {"states": (B, N, H), "x": (B, N, H, D), "wealth": (B, N, H), "final": (B, N), "drawdown": (B, N)}
    outs = {k: (guarded(shapes[k], torch.int32 if k == "states" else torch.float32, fill=7) if k in want else None)
            for k in ALL}
    got = lib.vqhmm_gauss_scenario_f32(*(_ext.ptr(t) for t in d_in), int(c["full"]), _ext.ptr(d_port), reb, tx, seed,
                                       b0, n0, B, N, H, S, D, *(None if outs[k] is None else outs[k].ptr for k in ALL),
                                       _ext.stream_ptr())
    assert got == rc, got
    check_all(*outs.values())
    return {k: v.t.cpu().numpy() for k, v in outs.items() if v is not None}


@functools.lru_cache(maxsize=None)
def reference(kind, B, N, H, S, D, reb=5, tx=1e-3):
    c = case_inputs(kind, B, N, H, S, D)
    ref = R.scenario_ref(c["start"], c["log_A"], c["mean"], c["scale"], c["full"], c["port"], reb, tx, SEED, 0, 0, B,
                         N, H)
    for v in ref.values():
        v.setflags(write=False)
    return c, ref


def check_own_recursion(c, g, reb, tx):
    """wealth / final / drawdown = the fp64 recursion on the kernel's own x and states, rel 1e-6, every path."""
    B, N, H, D = g["x"].shape
    wl, fin, dd, _ = R.wealth_ref(g["x"].reshape(B * N, H, D), g["states"].reshape(B * N, H), c["port"], reb, tx)
    np.testing.assert_allclose(g["wealth"].reshape(B * N, H), wl, rtol=1e-6, atol=0)
    np.testing.assert_allclose(g["final"].reshape(-1), fin, rtol=1e-6, atol=0)
    np.testing.assert_allclose(g["drawdown"].reshape(-1), dd, rtol=1e-6, atol=0)
    assert np.array_equal(g["final"].view(np.uint32), g["wealth"][..., H - 1].view(np.uint32))


def check_against_reference(ref, g):
    keep = ref["keep"]
    assert 1.0 - keep.mean() <= R.MAX_LEFT_OUT, keep.mean()
    assert np.array_equal(g["states"][keep], ref["states"][keep])
    err = np.abs(g["x"].astype(np.float64) - ref["x"])[keep]
    print("paths kept %d / %d, max |x - x_ref| / bound = %.3f (abs %.3e)"
          % (keep.sum(), keep.size, (err / ref["xtol"][keep]).max(), err.max()))
    assert (err <= ref["xtol"][keep]).all()
    if "wealth" in g:
        werr = np.abs(g["wealth"].astype(np.float64) - ref["wealth"])[keep]
        print("max |wealth - ref| / bound = %.3f" % (werr / ref["wealth_tol"][keep]).max())
        assert (werr <= ref["wealth_tol"][keep]).all()
        assert (np.abs(g["final"] - ref["final"])[keep] <= ref["wealth_tol"][..., -1][keep]).all()
        assert (np.abs(g["drawdown"] - ref["drawdown"])[keep] <= ref["drawdown_tol"][keep]).all()


@pytest.mark.parametrize("kind,B,N,H,S,D", EXACT_CASES + EXTRA_CASES)
def test_exact(kind, B, N, H, S, D):
    c, ref = reference(kind, B, N, H, S, D)
    g = run(c, B, N, H)
    check_against_reference(ref, g)
    check_own_recursion(c, g, 5, 1e-3)
    assert (g["states"] >= 0).all() and np.isfinite(g["x"]).all()


@pytest.mark.parametrize("reb", [1, 5, 40])
@pytest.mark.parametrize("tx", [0.0, 1e-3])
def test_wealth_settings(reb, tx):
    """rebalance 1, 5 and > H, tx_cost 0 and 1e-3, on the (4, 70, 33, 3, 12) full case."""
    kind, B, N, H, S, D = EXACT_CASES[5]
    c, ref = reference(kind, B, N, H, S, D, reb, tx)
    g = run(c, B, N, H, reb=reb, tx=tx)
    check_own_recursion(c, g, reb, tx)
    check_against_reference(ref, g)
    if tx == 0.0 and reb > H:   # the holdings of step 0's regime, never changed, no cost
        st, x = g["states"].reshape(-1, H), g["x"].reshape(-1, H, D).astype(np.float64)
        w1 = 1.0 + (c["port"][st[:, 0]].astype(np.float64) * x[:, 0]).sum(1)
        np.testing.assert_allclose(g["wealth"].reshape(-1, H)[:, 0], w1, rtol=1e-6)


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def test_independent_of_the_batch_split():
    kind, B, N, H, S, D = EXACT_CASES[5]
    c = case_inputs(kind, B, N, H, S, D)
    whole = run(c, B, N, H)
    a, b = run(c, B, 30, H), run(c, B, 40, H, n0=30)
    assert same_bits(whole, {k: np.concatenate([a[k], b[k]], 1) for k in ALL})
    a, b = run(c, 1, N, H), run(c, 3, N, H, b0=1, start=c["start"][1:])
    assert same_bits(whole, {k: np.concatenate([a[k], b[k]], 0) for k in ALL})
    assert same_bits(whole, run(c, B, N, H))   # two calls
    other = run(c, B, N, H, seed=SEED + 1)
    assert not np.array_equal(other["x"], whole["x"]) and not np.array_equal(other["states"], whole["states"])
    high = run(c, B, N, H, seed=SEED + (1 << 32))   # the high word of the seed is the key's second word
    assert not np.array_equal(high["x"], whole["x"])


@pytest.mark.parametrize("kind,B,N,H,S,D", [EXACT_CASES[5], EXACT_CASES[2]])
def test_independent_of_the_requested_outputs(kind, B, N, H, S, D):
    c = case_inputs(kind, B, N, H, S, D)
    whole = run(c, B, N, H)
    for want in (("final",), ("drawdown",), ("final", "drawdown"), ("wealth",), ("states", "wealth"),
                 ("x", "final")):
        part = run(c, B, N, H, want=want)
        assert sorted(part) == sorted(want)
        assert same_bits(part, {k: whole[k] for k in want}), want
    for want in (("states",), ("x",), ("states", "x")):   # no portfolio at all
        part = run(c, B, N, H, want=want, port=False)
        assert same_bits(part, {k: whole[k] for k in want}), want


def test_structural_zeros_and_failed_paths():
    S, D, B, N, H = 4, 3, 6, 64, 40
    log_A, mean, scale = R.make_case(5, S, D, True, zero_frac=0.3)
    log_A[3] = -np.inf                  # an all -inf row: a path fails at the step after it enters regime 3
    log_A[:3, 3] = np.log(np.float32(0.05))
    start = np.array([[1, 1, 1, 0], [0, 2, 0, 0], [0, 0, 0, 0], [1, -1, 1, 0], [1, np.inf, 0, 0], [0, 0, 0, 3]],
                     np.float32)
    c = dict(start=start, log_A=log_A, mean=mean, scale=scale, full=True, port=R.make_port(6, S, D))
    g = run(c, B, N, H)
    st = g["states"]
    A = np.exp(log_A)
    # zeros of start and -inf entries of log_A are never drawn
    assert (st[0, :, 0] != 3).all() and (st[1, :, 0] == 1).all() and (st[5, :, 0] == 3).all()
    prev, nxt = st[:, :, :-1], st[:, :, 1:]
    live = nxt >= 0
    assert (A[prev[live], nxt[live]] > 0).all()
    # a bad start row fails its own paths only, from step 0
    for b in (2, 3, 4):
        assert (st[b] == -1).all() and np.isnan(g["x"][b]).all() and np.isnan(g["wealth"][b]).all()
        assert np.isnan(g["final"][b]).all() and np.isnan(g["drawdown"][b]).all()
    assert (st[:2, :, 0] >= 0).all() and np.isfinite(g["x"][:2, :, 0]).all()
    # the all -inf row fails the path from the step after it is entered, and only then
    flat = st.reshape(-1, H)
    xs, wl = g["x"].reshape(-1, H, D), g["wealth"].reshape(-1, H)
    entered = 0
    for p in range(flat.shape[0]):
        if flat[p, 0] < 0:
            continue
        hit = np.nonzero(flat[p] == 3)[0]
        if hit.size == 0:
            assert (flat[p] >= 0).all() and np.isfinite(g["final"].reshape(-1)[p])
            continue
        t = hit[0]
        entered += 1
        assert (flat[p, :t + 1] >= 0).all() and (flat[p, t + 1:] == -1).all()
        assert np.isfinite(xs[p, :t + 1]).all() and np.isnan(xs[p, t + 1:]).all()
        assert np.isfinite(wl[p, :t + 1]).all() and np.isnan(wl[p, t + 1:]).all()
        assert np.isnan(g["final"].reshape(-1)[p]) == (t < H - 1)
    assert entered > 64    # start row 5 alone gives 64
    # and the live part agrees with the reference
    ref = R.scenario_ref(start, log_A, mean, scale, True, c["port"], 5, 1e-3, SEED, 0, 0, B, N, H)
    keep = ref["keep"]
    assert keep.mean() >= 0.75 and np.array_equal(st[keep], ref["states"][keep])


def full_model(S, D, seed):
    import vqhmm
    gen = torch.Generator().manual_seed(seed)
    m = vqhmm.GaussianHMM(S, D, "full", generator=gen)
    with torch.no_grad():
        L = 0.3 * torch.randn(S, D, D, generator=gen).tril() + torch.eye(D)
        m.scale_tril.copy_(L)
    return m.cuda()


def test_distribution():
    """B = 2 starts x N = 4096 paths, H = 6, S = 3, D = 4, full, through GaussianHMM.simulate from a filtered state:
    regime frequencies against probs A^t and the path mean of x_t against (probs A^t) mean within 5 sigma of their
    exact standard deviations; the step-0 covariance against predict_next's within 5 empirical standard errors of
    each product."""
    S, D, B, N, H = 3, 4, 2, 4096, 6
    m = full_model(S, D, 3)
    state = torch.tensor([[0.7, 0.2, 0.1], [0.05, 0.05, 0.9]], device="cuda")
    probs, pmean, pcov = (t.double().cpu().numpy() for t in m.predict_next(state))
    res = m.simulate(H, N, state=state, seed=77, return_x=True, return_states=True)
    st, x = res.states.cpu().numpy(), res.x.double().cpu().numpy()
    A = np.exp(m.log_A.double().cpu().numpy())
    A /= A.sum(1, keepdims=True)
    mu = m.mean.double().cpu().numpy()
    Lm = np.tril(m.scale_tril.double().cpu().numpy())
    sig = Lm @ Lm.transpose(0, 2, 1)
    for b in range(B):
        p = probs[b] / probs[b].sum()
        for t in range(H):
            freq = np.bincount(st[b, :, t], minlength=S) / N
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N)).all(), (b, t, freq, p)
            mt = p @ mu
            var = p @ (sig[:, np.arange(D), np.arange(D)] + mu ** 2) - mt ** 2
            assert (np.abs(x[b, :, t].mean(0) - mt) <= 5 * np.sqrt(var / N)).all(), (b, t)
            p = p @ A
        xc = x[b, :, 0] - pmean[b]
        prod = xc[:, :, None] * xc[:, None, :]
        se = prod.std(0) / np.sqrt(N)
        assert (np.abs(prod.mean(0) - pcov[b]) <= 5 * se).all(), b


@pytest.mark.parametrize("cov", ["diag", "full"])
def test_module_simulate(cov):
    import vqhmm
    S, D, H, N = 3, 5, 24, 96
    gen = torch.Generator().manual_seed(4)
    m = vqhmm.GaussianHMM(S, D, cov, generator=gen)
    with torch.no_grad():
        m.mean.mul_(1e-3)
        if cov == "full":
            m.scale_tril.copy_(1e-2 * (0.3 * torch.randn(S, D, D, generator=gen).tril() + torch.eye(D)))
        else:
            m.log_var.copy_(2 * torch.log(1e-2 * (0.5 + torch.rand(S, D, generator=gen))))
    m = m.cuda()
    port = torch.tensor(R.make_port(1, S, D))
    scale = (m.scale_tril if cov == "full" else torch.exp(0.5 * m.log_var.double()).float()).cpu().numpy()

    def ref_of(start, B, b0=0, n0=0, n=N):
        return R.scenario_ref(start, m.log_A.cpu().numpy(), m.mean.cpu().numpy(), scale, cov == "full", port.numpy(),
                              5, 1e-3, 9, b0, n0, B, n, H)

    # from log_pi
    res = m.simulate(H, N, seed=9, weights=port, rebalance=5, tx_cost=1e-3, return_x=True, return_states=True,
                     return_wealth=True)
    assert res.final.shape == (1, N) and res.x.shape == (1, N, H, D) and res.states.dtype == torch.int32
    g = {k: getattr(res, k).cpu().numpy() for k in ALL}
    check_against_reference(ref_of(torch.exp(m.log_pi.double()).float().cpu().numpy()[None], 1), g)
    # from a filtered state: step 0 is drawn from predict_next's probs
    x_obs = torch.randn(3, 7, D, generator=gen).mul(1e-2).cuda()
    state, _ = m.update(x_obs)
    res = m.simulate(H, N, state=state, seed=9, weights=port, rebalance=5, tx_cost=1e-3, return_x=True,
                     return_states=True, return_wealth=True)
    g = {k: getattr(res, k).cpu().numpy() for k in ALL}
    check_against_reference(ref_of(m.predict_next(state)[0].cpu().numpy(), 3), g)
    # only what is asked for is computed; a slice of starts and paths is the full call's rows
    lean = m.simulate(H, 40, state=state[1:], seed=9, weights=port, rebalance=5, tx_cost=1e-3, start_offset=1,
                      path_offset=16)
    assert lean.x is None and lean.states is None and lean.wealth is None
    assert torch.equal(lean.final, res.final[1:, 16:56]) and torch.equal(lean.drawdown, res.drawdown[1:, 16:56])
    only_x = m.simulate(H, N, state=state, seed=9, return_x=True)
    assert only_x.final is None and only_x.drawdown is None and torch.equal(only_x.x, res.x)
    with pytest.raises(ValueError, match="nothing to compute"):
        m.simulate(H, N)
    with pytest.raises(ValueError, match="weights"):
        m.simulate(H, N, return_wealth=True)
    with pytest.raises(ValueError, match="weights must have shape"):
        m.simulate(H, N, weights=port[:, :2])
    with pytest.raises(RuntimeError, match="HIP"):
        vqhmm.GaussianHMM(S, D, cov).simulate(H, N, weights=port)


def test_scenario_summary():
    import vqhmm
    m = full_model(3, 4, 8)
    with torch.no_grad():
        m.mean.mul_(1e-3)
        m.scale_tril.mul_(1e-2)
    port = torch.tensor(R.make_port(2, 3, 4))
    state = torch.tensor([[1.0, 0, 0], [0, 1, 0], [0.2, 0.3, 0.5]], device="cuda")
    final = m.simulate(60, 1000, state=state, seed=5, weights=port, rebalance=5, tx_cost=1e-3).final
    s = vqhmm.scenario_summary(final)
    f = final.double()
    q = torch.quantile(f, torch.tensor([0.05, 0.5, 0.95], dtype=torch.float64, device="cuda"), dim=1)
    for k, want in (("mean", f.mean(1)), ("std", f.std(1)), ("q05", q[0]), ("q50", q[1]), ("q95", q[2]),
                    ("prob_gain", (f > 1).double().mean(1))):
        assert s[k].shape == (3,) and torch.equal(s[k], want), k
    assert (s["q05"] < s["q50"]).all() and (s["q50"] < s["q95"]).all() and (s["std"] > 0).all()
    # against numpy on the host
    fn = f.cpu().numpy()
    np.testing.assert_allclose(s["q50"].cpu().numpy(), np.quantile(fn, 0.5, axis=1), rtol=1e-12)
    np.testing.assert_allclose(s["mean"].cpu().numpy(), fn.mean(1), rtol=1e-12)
    with pytest.raises(ValueError):
        vqhmm.scenario_summary(final[0])


def test_graph_capture():
    """No host sync, no workspace: the call is captured into a graph and replays to the same bits."""
    kind, B, N, H, S, D = EXACT_CASES[1]
    c = case_inputs(kind, B, N, H, S, D)
    whole = run(c, B, N, H, want=("final", "x"))
    from vqhmm import _ext
    lib = _ext.load()
    d_in = [dev(c[k]) for k in ("start", "log_A", "mean", "scale")]
    d_port = dev(c["port"])
    fin = torch.zeros((B, N), device="cuda")
    x = torch.zeros((B, N, H, D), device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.vqhmm_gauss_scenario_f32(*(_ext.ptr(t) for t in d_in), 1, _ext.ptr(d_port), 5, 1e-3, SEED, 0, 0, B, N,
                                          H, S, D, None, _ext.ptr(x), None, _ext.ptr(fin), None, _ext.stream_ptr())
    assert rc == 0, rc
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(fin.cpu().numpy(), whole["final"]) and np.array_equal(x.cpu().numpy(), whole["x"])
