"""Kernel micro-benchmarks (HIP events on the launch stream).

    python tools/kbench.py vq [--B 2048 --Dv 64 --T 200 --K 32]
    python tools/kbench.py xi --B 512 --T 512 --K 8     (fwdbwd, filter, xi, combined; alternated)
    python tools/kbench.py estep --B 1024 --T 512 --K 8 --V 512 [--old-route]
                                                        (the fused E-step on code indices; --old-route: also
                                                         the same statistics through pairwise_posteriors)
    python tools/kbench.py estep_batched --B 256 --T 200 --K 8 --V 512 --M 8 [--old-route]
                                                        (M models in one vqhmm_code_estep_batched_f32 call; --old-route:
                                                         also M sequential vqhmm_code_estep_f32 calls on the members, in
                                                         five alternating pairs, and a line that checks the two agree
                                                         exactly)
    python tools/kbench.py gauss_estep --B 2048 --T 200 --K 32 --D 16 [--old-route]
                                                        (the fused Gaussian-HMM E-step on x (B,T,D); --old-route: also
                                                         torch emissions + expanded log_A + pairwise_posteriors + torch
                                                         moment sums, in five alternating pairs, and a check line)
    python tools/kbench.py gauss_full_estep --B 2048 --T 200 --K 32 --D 16 [--old-route]
    python tools/kbench.py gauss_moments --B 2048 --T 200 --K 32 --D 16 [--old-route]
                                                        (the full-covariance E-step / the regime moments under a given
                                                         gamma; --old-route: also the torch route (triangular solve,
                                                         emissions, expanded log_A, pairwise_posteriors, fp64 einsum /
                                                         the fp64 einsum alone), five alternating pairs, a check line)
    python tools/kbench.py gauss_estep_batched --B 512 --T 512 --K 8 --D 5 --M 8 [--full] [--old-route]
                                                        (M Gaussian HMMs in one vqhmm_gauss_estep_batched_f32 /
                                                         vqhmm_gauss_full_estep_batched_f32 call; --old-route: also M
                                                         sequential single-model calls on the members, five alternating
                                                         pairs; every member is first checked bit for bit against them)
    python tools/kbench.py code_fit --B 256 --T 200 --K 8 --V 512 --M 8 [--iters 20]
                                                        (--iters EM iterations of CodeHMMEnsemble.fit against --M
                                                         sequential CodeHMM.fit(n_init=1) runs, five alternating pairs)
    python tools/kbench.py code_viterbi --B 512 --T 512 --K 8 --V 512 [--old-route]
    python tools/kbench.py code_filter --B 2048 --T 200 --K 32 --V 512 [--old-route]
                                                        (CodeHMM's fused decode / causal filter; --old-route: also
                                                         the expanded tables through viterbi / forward_filter)
    python tools/kbench.py sample --B 512 --T 512 --K 8 --N 64
                                                        (the FFBS and simulation kernels, the filter beside them,
                                                         and a plain-torch FFBS loop on the same shapes)
    python tools/kbench.py gauss_viterbi --B 2048 --T 200 --K 32 --D 16 [--full] [--old-route]
    python tools/kbench.py gauss_filter --B 2048 --T 200 --K 32 --D 16 [--full] [--old-route]
                                                        (GaussianHMM's fused decode / causal filter on x; --full:
                                                         full covariances; --old-route: also the emission entry +
                                                         expanded log_A + viterbi / forward_filter; the filter leg
                                                         also times the E-step of the same shape)
    python tools/kbench.py gauss_scenario --B 512 --N 256 --T 64 --K 3 --D 12 [--full] [--old-route]
                                                        (GaussianHMM.simulate: B starts x N paths x T steps, final +
                                                         drawdown only and with x written; --old-route: also
                                                         simulate_paths + torch.randn + gather / matmul + torch wealth,
                                                         five alternating pairs, a check line on the distributions)
    python tools/kbench.py vq_stats --B 2048 --Dv 64 --T 200 --K 32 [--old-route]
    python tools/kbench.py vq_bwd --B 2048 --Dv 64 --T 200 --K 32 [--old-route]
                                                        (the codebook statistics / the quantizer's fused backward;
                                                         --old-route: also bincount + index_add_ / the torch backward
                                                         of vqhmm.quantize, in five alternating pairs)
    python tools/kbench.py backtest --B 512 --T 252 --K 3 --D 12 --P 64 [--hard] [--bwd] [--old-route]
                                                        (vqhmm.backtest: B windows x P weight tables, S = K regimes;
                                                         --bwd: with an objective on metrics() and its backward;
                                                         --old-route: also the torch fp64 restatement (einsum, gather,
                                                         cumprod, cummax; autograd with --bwd), five alternating pairs,
                                                         a check line on stats and gradient within the derived bound)
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vq-vae-hmm-model_amd"))
import vqhmm  # noqa: E402

HBM_PEAK = 8.0e12


def time_fn(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def bench_vq(a):
    g = torch.Generator(device="cuda").manual_seed(1234)
    z = torch.randn(a.B, a.Dv, a.T, device="cuda", generator=g)
    cb = torch.randn(a.K, a.Dv, device="cuda", generator=g)
    idx = torch.empty(a.B, a.T, dtype=torch.int32, device="cuda")
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()

    def fn():
        lib.vqhmm_vq_argmin_f32(P(z), a.B, a.Dv, a.T, P(cb), a.K, P(idx), None, st)

    t = time_fn(fn)
    N = a.B * a.T
    byts = 4 * N * a.Dv + 4 * a.K * a.Dv + 4 * N
    print(json.dumps({"kernel": "vq_argmin", "B": a.B, "Dv": a.Dv, "T": a.T, "K": a.K, "us": t * 1e6,
                      "GBps": byts / t / 1e9, "frac_hbm": byts / t / HBM_PEAK}))


def bench_stream(a):
    """Bandwidth references on the VQ input size: torch read-reduce and copy of z."""
    z = torch.randn(a.B, a.Dv, a.T, device="cuda")
    out = torch.empty_like(z)
    nb = z.numel() * 4
    t_sum = time_fn(lambda: z.sum())
    t_cp = time_fn(lambda: out.copy_(z))
    print(json.dumps({"kernel": "torch_stream", "bytes": nb, "sum_us": t_sum * 1e6, "sum_GBps": nb / t_sum / 1e9,
                      "copy_us": t_cp * 1e6, "copy_GBps": 2 * nb / t_cp / 1e9}))


def hmm_tables(B, T, K, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    log_pi = torch.log_softmax(torch.randn(K, device="cuda", generator=g), -1)
    log_A = torch.log_softmax(torch.randn(B, T, K, K, device="cuda", generator=g), -1)
    em = torch.log_softmax(torch.randn(B, T, K, device="cuda", generator=g), -1)
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    return log_pi, log_A, em, L


def bench_viterbi(a):
    B, T, K = a.B, a.T, a.K
    log_pi, log_A, em, L = hmm_tables(B, T, K)
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    path = torch.empty(B, T, dtype=torch.int32, device="cuda")
    score = torch.empty(B, device="cuda")
    nb = lib.vqhmm_viterbi_workspace_size(B, T, K)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    def fn():
        lib.vqhmm_viterbi_f32(P(log_pi), P(log_A), P(em), P(L), B, T, K, P(path), P(score), P(ws), nb, st)

    t = time_fn(fn, iters=5, warmup=2)
    byts = B * (4 * T * K * K + 4 * T * K + 4 * T) + 4 * K
    print(json.dumps({"kernel": "viterbi", "B": B, "T": T, "K": K, "us": t * 1e6, "GBps": byts / t / 1e9,
                      "frac_hbm": byts / t / HBM_PEAK}))


def bench_fwdbwd(a):
    B, T, K = a.B, a.T, a.K
    log_pi, log_A, em, L = hmm_tables(B, T, K)
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    gamma = torch.empty(B, T, K, device="cuda")
    logZ = torch.empty(B, device="cuda")
    nb = lib.vqhmm_fwdbwd_workspace_size(B, T, K)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    def fn():
        lib.vqhmm_fwdbwd_f32(P(log_pi), P(log_A), P(em), P(L), B, T, K, P(gamma), P(logZ), P(ws), nb, st)

    t = time_fn(fn, iters=20, warmup=3)
    byts = B * (4 * T * K * K + 4 * T * K + 4 * T * K) + 4 * K
    print(json.dumps({"kernel": "fwdbwd", "B": B, "T": T, "K": K, "us": t * 1e6, "GBps": byts / t / 1e9,
                      "frac_hbm": byts / t / HBM_PEAK}))


def _pair_legs(a):
    """The launches behind vqhmm.pairwise_posteriors on one set of tables: name -> callable."""
    B, T, K = a.B, a.T, a.K
    log_pi, log_A, em, L = hmm_tables(B, T, K)
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    gamma = torch.empty(B, T, K, device="cuda")
    filt = torch.empty(B, T, K, device="cuda")
    xi = torch.empty(B, T, K, K, device="cuda")
    logZ = torch.empty(B, device="cuda")
    nb = lib.vqhmm_fwdbwd_workspace_size(B, T, K)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    nbx = lib.vqhmm_fwdbwd_xi_workspace_size(B, T, K)
    wsx = torch.empty(max(nbx, 1), dtype=torch.uint8, device="cuda")
    keep = (log_pi, log_A, em, L, gamma, filt, xi, logZ, ws, wsx)

    def fwdbwd():
        lib.vqhmm_fwdbwd_f32(P(log_pi), P(log_A), P(em), P(L), B, T, K, P(gamma), P(logZ), P(ws), nb, st)

    def filt_fn():
        lib.vqhmm_filter_f32(P(log_pi), P(log_A), P(em), P(L), B, T, K, P(filt), P(logZ), st)

    def combined():
        lib.vqhmm_fwdbwd_xi_f32(P(log_pi), P(log_A), P(em), P(L), B, T, K, P(gamma), P(xi), P(logZ), P(wsx), nbx, st)

    return {"fwdbwd": fwdbwd, "filter": filt_fn, "fwdbwd_xi": combined}, keep


def bench_filter(a):
    B, T, K = a.B, a.T, a.K
    legs, _keep = _pair_legs(a)
    t = time_fn(legs["filter"], iters=20, warmup=3)
    byts = B * T * (4 * K * K + 8 * K)
    print(json.dumps({"kernel": "filter", "B": B, "T": T, "K": K, "us": t * 1e6, "GBps": byts / t / 1e9,
                      "frac_hbm": byts / t / HBM_PEAK}))


def bench_xi(a):
    """fwdbwd, filter and the combined vqhmm_fwdbwd_xi_f32 in one process, alternated after a
    warm-up (median of the rounds); the xi launch is the combined call less its two other
    launches (the three run back to back on one stream).  Algorithmic bytes per position:
    fwdbwd 4K^2 + 8K, filter 4K^2 + 8K, xi 8K^2 + 8K."""
    B, T, K = a.B, a.T, a.K
    legs, _keep = _pair_legs(a)
    for fn in legs.values():
        time_fn(fn, iters=3, warmup=2)
    rounds = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            rounds[k].append(time_fn(fn, iters=10, warmup=1))
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    t["xi"] = t["fwdbwd_xi"] - t["fwdbwd"] - t["filter"]
    n = B * T
    byts = {"fwdbwd": n * (4 * K * K + 8 * K), "filter": n * (4 * K * K + 8 * K), "xi": n * (8 * K * K + 8 * K)}
    byts["fwdbwd_xi"] = sum(byts.values())
    for k in ("fwdbwd", "filter", "xi", "fwdbwd_xi"):
        print(json.dumps({"kernel": k, "B": B, "T": T, "K": K, "us": t[k] * 1e6, "GBps": byts[k] / t[k] / 1e9,
                          "frac_hbm": byts[k] / t[k] / HBM_PEAK, "x_fwdbwd": t[k] / t["fwdbwd"]}))


def bench_estep(a):
    """vqhmm_code_estep_f32 (counts + loglik, no gamma) at S = --K states, V = --V codes.  --old-route: also the
    existing entry points' way to the same statistics (broadcast log_A, the log_B[:, codes] gather,
    pairwise_posteriors, then xi.sum, gamma[:, 0].sum and index_add_), alternated with the new call (median of
    the rounds).  Algorithmic HBM bytes per position: the code (4) and the scaled forward vector written and
    read back (8 S); the old route's: 4 S^2 (log_A) + 4 S (em) written, read by three kernels, + xi."""
    B, T, S, V = a.B, a.T, a.K, a.V
    g = torch.Generator(device="cuda").manual_seed(11)
    hmm = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(3)).cuda()
    codes = torch.randint(0, V, (B, T), device="cuda", generator=g, dtype=torch.int32)
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    cnt = [torch.empty(n, dtype=torch.float64, device="cuda") for n in (S, S * S, S * V)]
    ll = torch.empty(B, device="cuda")
    nb = lib.vqhmm_code_estep_workspace_size(B, T, S, V)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    def new():
        lib.vqhmm_code_estep_f32(P(hmm.log_pi), P(hmm.log_A), P(hmm.log_B), P(codes), P(L), B, T, S, V, P(cnt[0]),
                                 P(cnt[1]), P(cnt[2]), P(ll), None, P(ws), nb, st)

    cl = codes.long()

    def old():
        log_A = hmm.log_A.expand(B, T, S, S)
        em = hmm.log_B[:, cl].permute(1, 2, 0)
        gamma, xi, logZ = vqhmm.pairwise_posteriors(hmm.log_pi, log_A, em, L)
        trans = xi.sum((0, 1), dtype=torch.float64)
        pi = gamma[:, 0].sum(0, dtype=torch.float64)
        emit = torch.zeros(V, S, dtype=torch.float64, device="cuda").index_add_(0, cl.reshape(-1),
                                                                               gamma.reshape(-1, S).double())
        return pi, trans, emit, logZ

    legs = {"code_estep": new}
    if a.old_route:
        legs["old_route"] = old
        pi, trans, emit, _ = old()
        new()
        torch.cuda.synchronize()
        print(json.dumps({"check": "old_route vs code_estep", "trans_maxdiff": (trans.reshape(-1) - cnt[1]).abs().max().item(),
                          "emit_maxdiff": (emit.t().reshape(-1) - cnt[2]).abs().max().item(),
                          "pi_maxdiff": (pi - cnt[0]).abs().max().item()}))
    for fn in legs.values():
        time_fn(fn, iters=3, warmup=2)
    rounds = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            rounds[k].append(time_fn(fn, iters=10, warmup=1))
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    n = B * T
    byts = {"code_estep": n * (4 + 8 * S), "old_route": n * (4 * S * S * (1 + 3 + 2 + 1) + 4 * S * (1 + 3 + 2 + 2))}
    for k in legs:
        rec = {"kernel": k, "B": B, "T": T, "S": S, "V": V, "us": t[k] * 1e6, "min_us": min(rounds[k]) * 1e6,
               "max_us": max(rounds[k]) * 1e6, "GBps": byts[k] / t[k] / 1e9, "frac_hbm": byts[k] / t[k] / HBM_PEAK}
        if k == "old_route":
            rec["x_code_estep"] = t[k] / t["code_estep"]
        print(json.dumps(rec))


def _pairs(legs, rounds_n=5, iters=10):
    """Warm every leg up, then time them alternately rounds_n times -> {leg: [seconds per call]}."""
    for fn in legs.values():
        time_fn(fn, iters=3, warmup=2)
    rounds = {k: [] for k in legs}
    for _ in range(rounds_n):
        for k, fn in legs.items():
            rounds[k].append(time_fn(fn, iters=iters, warmup=1))
    return rounds


def bench_estep_batched(a):
    """vqhmm_code_estep_batched_f32 (counts + loglik, no gamma) on --M members of S = --K states, V = --V codes
    that share one batch of full-length sequences.  --old-route: also --M sequential vqhmm_code_estep_f32 calls
    on the members' slices, in five alternating pairs after a warm-up, every pair's two times reported, and a
    check line with the largest difference between the two routes' outputs, which must be 0."""
    B, T, S, V, M = a.B, a.T, a.K, a.V, a.M
    g = torch.Generator(device="cuda").manual_seed(11)
    ens = vqhmm.CodeHMMEnsemble(num_models=M, num_states=S, num_codes=V, generator=torch.Generator().manual_seed(3)).cuda()
    codes = torch.randint(0, V, (B, T), device="cuda", generator=g, dtype=torch.int32)
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    cnt = [torch.empty((M, n), dtype=torch.float64, device="cuda") for n in (S, S * S, S * V)]
    ll = torch.empty(M, B, device="cuda")
    cnt1 = [torch.empty((M, n), dtype=torch.float64, device="cuda") for n in (S, S * S, S * V)]
    ll1 = torch.empty(M, B, device="cuda")
    nb = lib.vqhmm_code_estep_batched_workspace_size(B, T, S, V, M)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    nb1 = lib.vqhmm_code_estep_workspace_size(B, T, S, V)

    def new():
        lib.vqhmm_code_estep_batched_f32(P(ens.log_pi), P(ens.log_A), P(ens.log_B), P(codes), P(L), None, B, T, S, V, M,
                                         P(cnt[0]), P(cnt[1]), P(cnt[2]), P(ll), None, P(ws), nb, st)

    def old():
        for m in range(M):
            lib.vqhmm_code_estep_f32(P(ens.log_pi[m]), P(ens.log_A[m]), P(ens.log_B[m]), P(codes), P(L), B, T, S, V,
                                     P(cnt1[0][m]), P(cnt1[1][m]), P(cnt1[2][m]), P(ll1[m]), None, P(ws), nb1, st)

    legs = {"estep_batched": new}
    if a.old_route:
        legs["sequential"] = old
        new()
        old()
        torch.cuda.synchronize()
        diffs = [(x - y).abs().max().item() for x, y in zip(cnt + [ll], cnt1 + [ll1])]
        print(json.dumps({"check": "sequential vs estep_batched", "B": B, "T": T, "S": S, "V": V, "M": M,
                          "maxdiff": max(diffs)}))
    rounds = _pairs(legs)
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    for k in legs:
        rec = {"kernel": k, "B": B, "T": T, "S": S, "V": V, "M": M, "us": t[k] * 1e6,
               "pairs_us": [r * 1e6 for r in rounds[k]], "us_per_member": t[k] * 1e6 / M}
        if k == "sequential":
            rec["x_estep_batched"] = t[k] / t["estep_batched"]
            rec["batched_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds["estep_batched"]))
        print(json.dumps(rec))


def bench_gauss_estep(a):
    """vqhmm_gauss_estep_f32 (counts + loglik, no gamma) at S = --K states on x (B,T,--D).  --old-route: also the
    time-varying kernels' way to the same statistics (the emissions in torch, log_A expanded to (B,T,S,S),
    pairwise_posteriors, the moment sums in torch; all of it inside the timed call, the (B,T,S,S) copy of the
    expanded view included, which pairwise_posteriors makes itself), in five alternating pairs after a warm-up,
    every pair's two times reported, and a check line with the largest differences between the two routes' counts relative to the
    tests' bounds' scales.  Algorithmic HBM bytes per position of the fused call: x read twice (8 D) and the
    scaled forward vector written and read back (8 S)."""
    B, T, S, D = a.B, a.T, a.K, a.D
    g = torch.Generator(device="cuda").manual_seed(11)
    hmm = vqhmm.GaussianHMM(S, D, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        hmm.mean.mul_(2.0)
    z = torch.randint(0, S, (B, T), device="cuda", generator=g)
    x = (hmm.mean[z] + torch.randn((B, T, D), device="cuda", generator=g)).contiguous()
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    shift = x.mean((0, 1)).contiguous()
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    names = ("pi_cnt", "trans_cnt", "occ", "m1", "m2")
    cnt = {k: torch.empty(n, dtype=torch.float64, device="cuda") for k, n in zip(names, (S, S * S, S, S * D, S * D))}
    ll = torch.empty(B, device="cuda")
    nb = lib.vqhmm_gauss_estep_workspace_size(B, T, S, D)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    def new():
        lib.vqhmm_gauss_estep_f32(P(hmm.log_pi), P(hmm.log_A), P(hmm.mean), P(hmm.log_var), P(x), P(L), P(shift), None,
                                  B, T, S, D, *(P(cnt[k]) for k in names), P(ll), None, P(ws), nb, st)

    def old():
        iv = torch.exp(-hmm.log_var)
        em = -0.5 * (((x[:, :, None, :] - hmm.mean) ** 2 * iv).sum(-1) + hmm.log_var.sum(-1)) - 0.5 * D * math.log(2 * math.pi)
        gamma, xi, logZ = vqhmm.pairwise_posteriors(hmm.log_pi, hmm.log_A.expand(B, T, S, S), em, L)
        y = (x - shift).double()
        gd = gamma.double()
        return {"pi_cnt": gamma[:, 0].sum(0, dtype=torch.float64), "trans_cnt": xi.sum((0, 1), dtype=torch.float64),
                "occ": gd.sum((0, 1)), "m1": torch.einsum("bts,btd->sd", gd, y),
                "m2": torch.einsum("bts,btd->sd", gd, y * y), "loglik": logZ}

    legs = {"gauss_estep": new}
    if a.old_route:
        legs["old_route"] = old
        ref = old()
        new()
        torch.cuda.synchronize()
        n = B * T
        scale = {"pi_cnt": B, "trans_cnt": n, "occ": n, "m1": (x - shift).abs().sum().item() / D,
                 "m2": ((x - shift) ** 2).sum().item() / D}
        rec = {"check": "old_route vs gauss_estep", "B": B, "T": T, "S": S, "D": D}
        for k in names:
            rec[k + "_maxdiff_per_scale"] = (ref[k].reshape(-1) - cnt[k]).abs().max().item() / scale[k]
        rec["loglik_maxrel"] = ((ref["loglik"] - ll).abs() / ll.abs().clamp_min(1.0)).max().item()
        print(json.dumps(rec))
        del ref
    rounds = _pairs(legs)
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    byts = B * T * (8 * D + 8 * S)
    for k in legs:
        rec = {"kernel": k, "B": B, "T": T, "S": S, "D": D, "us": t[k] * 1e6, "pairs_us": [r * 1e6 for r in rounds[k]]}
        if k == "gauss_estep":
            rec.update({"GBps": byts / t[k] / 1e9, "frac_hbm": byts / t[k] / HBM_PEAK})
        else:
            rec["x_gauss_estep"] = t[k] / t["gauss_estep"]
            rec["fused_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds["gauss_estep"]))
        print(json.dumps(rec))


def _full_case(B, T, S, D):
    """A full-covariance model with random correlated covariances, data around its means, full lengths."""
    g = torch.Generator(device="cuda").manual_seed(11)
    hmm = vqhmm.GaussianHMM(S, D, covariance_type="full", generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        hmm.mean.mul_(2.0)
        Lc = torch.randn((S, D, D), device="cuda", generator=g).tril(-1) * (0.4 / math.sqrt(D))
        hmm.scale_tril.copy_(Lc + torch.diag_embed(torch.rand((S, D), device="cuda", generator=g) + 0.6))
    z = torch.randint(0, S, (B, T), device="cuda", generator=g)
    x = hmm.mean[z] + torch.randn((B, T, D), device="cuda", generator=g)
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    return hmm, x.contiguous(), L, x.mean((0, 1)).contiguous()


def _report(legs, rounds, new, dims, extra=None):
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    for k in legs:
        rec = dict({"kernel": k}, **dims, us=t[k] * 1e6, pairs_us=[r * 1e6 for r in rounds[k]])
        if k == new:
            rec.update(extra(t[k]) if extra else {})
        else:
            rec["x_" + new] = t[k] / t[new]
            rec["fused_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds[new]))
        print(json.dumps(rec))


def bench_gauss_full_estep(a):
    """vqhmm_gauss_full_estep_f32 (counts + loglik, no gamma) at S = --K states on x (B,T,--D).  --old-route: also
    the torch way to the same statistics (W by solve_triangular, the emissions by a batched product into (B,T,S),
    log_A expanded to (B,T,S,S), pairwise_posteriors, the moments by fp64 einsum; all inside the timed call), in
    five alternating pairs after a warm-up, and a check line with the largest differences between the two routes'
    counts relative to the tests' bounds' scales."""
    B, T, S, D = a.B, a.T, a.K, a.D
    hmm, x, L, shift = _full_case(B, T, S, D)
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    names = ("pi_cnt", "trans_cnt", "occ", "m1", "m2")
    cnt = {k: torch.empty(n, dtype=torch.float64, device="cuda")
           for k, n in zip(names, (S, S * S, S, S * D, S * D * D))}
    ll = torch.empty(B, device="cuda")
    nb = lib.vqhmm_gauss_full_estep_workspace_size(B, T, S, D)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    W = hmm.precisions_cholesky

    def new():
        lib.vqhmm_gauss_full_estep_f32(P(hmm.log_pi), P(hmm.log_A), P(hmm.mean), P(W), P(x), P(L), P(shift), None,
                                       B, T, S, D, *(P(cnt[k]) for k in names), P(ll), None, P(ws), nb, st)

    def old():
        eye = torch.eye(D, device="cuda").expand(S, D, D)
        Wt = torch.linalg.solve_triangular(hmm.scale_tril, eye, upper=False)
        em = torch.empty((B, T, S), device="cuda")
        for s in range(S):   # (B T, D) x (D, D) per state: the (B,T,S,D) intermediate never exists
            r = (x - hmm.mean[s]).reshape(-1, D) @ Wt[s].T
            em[:, :, s] = (-0.5 * (r * r).sum(-1) + torch.log(torch.diagonal(Wt[s])).sum()
                           - 0.5 * D * math.log(2 * math.pi)).view(B, T)
        gamma, xi, logZ = vqhmm.pairwise_posteriors(hmm.log_pi, hmm.log_A.expand(B, T, S, S), em, L)
        y = (x - shift).double()
        gd = gamma.double()
        return {"pi_cnt": gamma[:, 0].sum(0, dtype=torch.float64), "trans_cnt": xi.sum((0, 1), dtype=torch.float64),
                "occ": gd.sum((0, 1)), "m1": torch.einsum("bts,btd->sd", gd, y),
                "m2": torch.einsum("bts,bti,btj->sij", gd, y, y), "loglik": logZ}

    legs = {"gauss_full_estep": new}
    if a.old_route:
        legs["old_route"] = old
        ref = old()
        new()
        torch.cuda.synchronize()
        n = B * T
        ya = (x - shift).abs()
        scale = {"pi_cnt": B, "trans_cnt": n, "occ": n, "m1": ya.sum().item() / D, "m2": (ya ** 2).sum().item() / D}
        rec = {"check": "old_route vs gauss_full_estep", "B": B, "T": T, "S": S, "D": D}
        for k in names:
            rec[k + "_maxdiff_per_scale"] = (ref[k].reshape(-1) - cnt[k]).abs().max().item() / scale[k]
        rec["loglik_maxrel"] = ((ref["loglik"] - ll).abs() / ll.abs().clamp_min(1.0)).max().item()
        print(json.dumps(rec))
        del ref
    byts = B * T * (8 * D + 8 * S)
    _report(legs, _pairs(legs), "gauss_full_estep", {"B": B, "T": T, "S": S, "D": D},
            lambda t: {"GBps": byts / t / 1e9, "frac_hbm": byts / t / HBM_PEAK})


def bench_gauss_estep_batched(a):
    """vqhmm_gauss_estep_batched_f32 (--full: vqhmm_gauss_full_estep_batched_f32; counts + loglik, no gamma) on --M
    members of S = --K states that share x (B,T,--D), full lengths and the shift.  Before any timing every member's
    five counts and loglik are compared byte for byte with the single-model call on its slices (a check line;
    a mismatch ends the run).  --old-route: also --M sequential single-model calls, the only other way to the same
    numbers, in five alternating pairs after a warm-up, every pair's two times reported."""
    B, T, S, D, M, full = a.B, a.T, a.K, a.D, a.M, a.full
    gen = torch.Generator().manual_seed(3)
    ens = vqhmm.GaussianHMMEnsemble(num_models=M, num_states=S, dim=D, covariance_type="full" if full else "diag",
                                    generator=gen).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        ens.mean.mul_(2.0)
        if full:
            Lc = torch.randn((M, S, D, D), device="cuda", generator=g).tril(-1) * (0.4 / math.sqrt(D))
            ens.scale_tril.copy_(Lc + torch.diag_embed(torch.rand((M, S, D), device="cuda", generator=g) + 0.6))
    z = torch.randint(0, S, (B, T), device="cuda", generator=g)
    x = (ens.mean[0][z] + torch.randn((B, T, D), device="cuda", generator=g)).contiguous()
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    shift = x.mean((0, 1)).contiguous()
    log_pi, log_A, mean, last = (t.contiguous() for t in ens._params())
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    sizes = (S, S * S, S, S * D, S * D * D if full else S * D)
    cnt = [torch.empty((M, n), dtype=torch.float64, device="cuda") for n in sizes]
    cnt1 = [torch.empty((M, n), dtype=torch.float64, device="cuda") for n in sizes]
    ll, ll1 = torch.empty(M, B, device="cuda"), torch.empty(M, B, device="cuda")
    if full:
        size_m, entry_m = lib.vqhmm_gauss_full_estep_batched_workspace_size, lib.vqhmm_gauss_full_estep_batched_f32
        size_1, entry_1 = lib.vqhmm_gauss_full_estep_workspace_size, lib.vqhmm_gauss_full_estep_f32
    else:
        size_m, entry_m = lib.vqhmm_gauss_estep_batched_workspace_size, lib.vqhmm_gauss_estep_batched_f32
        size_1, entry_1 = lib.vqhmm_gauss_estep_workspace_size, lib.vqhmm_gauss_estep_f32
    nb, nb1 = size_m(B, T, S, D, M), size_1(B, T, S, D)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    def new():
        entry_m(P(log_pi), P(log_A), P(mean), P(last), P(x), P(L), P(shift), None, B, T, S, D, M,
                *(P(c) for c in cnt), P(ll), None, P(ws), nb, st)

    def old():
        for m in range(M):
            entry_1(P(log_pi[m]), P(log_A[m]), P(mean[m]), P(last[m]), P(x), P(L), P(shift), None, B, T, S, D,
                    *(P(c[m]) for c in cnt1), P(ll1[m]), None, P(ws), nb1, st)

    new()
    old()
    torch.cuda.synchronize()
    same = all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(cnt + [ll], cnt1 + [ll1]))
    dims = {"B": B, "T": T, "S": S, "D": D, "M": M, "full": bool(full)}
    print(json.dumps(dict({"check": "sequential vs gauss_estep_batched", "bit_identical": same}, **dims)))
    if not same:
        raise SystemExit("gauss_estep_batched: a member differs from the single-model call")
    legs = {"gauss_estep_batched": new}
    if a.old_route:
        legs["sequential"] = old
    rounds = _pairs(legs)
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    for k in legs:
        rec = dict({"kernel": k}, **dims, us=t[k] * 1e6, pairs_us=[r * 1e6 for r in rounds[k]],
                   us_per_member=t[k] * 1e6 / M)
        if k == "sequential":
            rec["x_gauss_estep_batched"] = t[k] / t["gauss_estep_batched"]
            rec["batched_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds["gauss_estep_batched"]))
        print(json.dumps(rec))


def bench_gauss_moments(a):
    """vqhmm_gauss_moments_f32 (occ, m1, m2 under a given gamma (B,T,--K)) on x (B,T,--D).  --old-route: also the
    fp64 einsum of the same sums, in five alternating pairs, and a check line."""
    B, T, S, D = a.B, a.T, a.K, a.D
    hmm, x, L, shift = _full_case(B, T, S, D)
    gamma = torch.softmax(torch.randn((B, T, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)), -1)
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    names = ("occ", "m1", "m2")
    cnt = {k: torch.empty(n, dtype=torch.float64, device="cuda") for k, n in zip(names, (S, S * D, S * D * D))}
    nb = lib.vqhmm_gauss_moments_workspace_size(B, T, S, D)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

    def new():
        lib.vqhmm_gauss_moments_f32(P(x), P(gamma), P(L), P(shift), None, B, T, S, D, *(P(cnt[k]) for k in names),
                                    P(ws), nb, st)

    def old():
        y = (x - shift).double()
        gd = gamma.double()
        return {"occ": gd.sum((0, 1)), "m1": torch.einsum("bts,btd->sd", gd, y),
                "m2": torch.einsum("bts,bti,btj->sij", gd, y, y)}

    legs = {"gauss_moments": new}
    if a.old_route:
        legs["old_route"] = old
        ref = old()
        new()
        torch.cuda.synchronize()
        ya = (x - shift).abs()
        scale = {"occ": B * T, "m1": ya.sum().item() / D, "m2": (ya ** 2).sum().item() / D}
        rec = {"check": "old_route vs gauss_moments", "B": B, "T": T, "S": S, "D": D}
        for k in names:
            rec[k + "_maxdiff_per_scale"] = (ref[k].reshape(-1) - cnt[k]).abs().max().item() / scale[k]
        print(json.dumps(rec))
        del ref
    byts = B * T * (8 * D + 8 * S)   # x and gamma, each read by the flag launch and by the product
    _report(legs, _pairs(legs), "gauss_moments", {"B": B, "T": T, "S": S, "D": D},
            lambda t: {"GBps": byts / t / 1e9, "frac_hbm": byts / t / HBM_PEAK})


def bench_code_fit(a):
    """--iters EM iterations of CodeHMMEnsemble.fit on --M members against --M sequential CodeHMM.fit(n_init=1)
    runs from the same starts (every timed call starts from a copy of them), five alternating pairs."""
    B, T, S, V, M, n_iter = a.B, a.T, a.K, a.V, a.M, a.iters
    g = torch.Generator(device="cuda").manual_seed(11)
    ens = vqhmm.CodeHMMEnsemble(num_models=M, num_states=S, num_codes=V, generator=torch.Generator().manual_seed(3)).cuda()
    hmms = [ens.member(m) for m in range(M)]
    start = {k: v.clone() for k, v in ens.state_dict().items()}
    codes = torch.randint(0, V, (B, T), device="cuda", generator=g, dtype=torch.int32)
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")

    def new():
        ens.load_state_dict(start)
        return ens.fit(codes, L, n_iter=n_iter, prior_count=1e-3)

    def old():
        for m, h in enumerate(hmms):
            for k in ("log_pi", "log_A", "log_B"):
                getattr(h, k).copy_(start[k][m])
            h.fit(codes, L, n_iter=n_iter, prior_count=1e-3)

    rounds = _pairs({"ensemble_fit": new, "sequential_fit": old}, iters=2)
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    for k in rounds:
        rec = {"kernel": k, "B": B, "T": T, "S": S, "V": V, "M": M, "n_iter": n_iter, "ms": t[k] * 1e3,
               "pairs_ms": [r * 1e3 for r in rounds[k]], "us_per_member_iteration": t[k] * 1e6 / (M * n_iter)}
        if k == "sequential_fit":
            rec["x_ensemble_fit"] = t[k] / t["ensemble_fit"]
            rec["ensemble_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds["ensemble_fit"]))
        print(json.dumps(rec))


def _bench_code_decode(a, leg):
    """One of CodeHMM's fused read-outs at S = --K states, V = --V codes on full-length sequences.  --old-route:
    also the time-varying entry point's way to the same result (log_A broadcast to (B,T,S,S), the log_B[:, codes]
    gather to (B,T,S), then viterbi / forward_filter; building the tables is part of its time), in five
    alternating pairs after a warm-up, every pair's two times reported, and a line that checks the two routes
    agree.  Algorithmic HBM bytes per position: the code read (4) and the path (4) or filt (4 S) written; the
    old route's: 4 S^2 + 4 S written, then read, plus the same output."""
    B, T, S, V = a.B, a.T, a.K, a.V
    g = torch.Generator(device="cuda").manual_seed(11)
    hmm = vqhmm.CodeHMM(S, V, generator=torch.Generator().manual_seed(3)).cuda()
    codes = torch.randint(0, V, (B, T), device="cuda", generator=g, dtype=torch.int32)
    L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    cl = codes.long()
    if leg == "code_viterbi":
        path = torch.empty(B, T, dtype=torch.int32, device="cuda")
        score = torch.empty(B, device="cuda")
        nb = lib.vqhmm_code_viterbi_workspace_size(B, T, S, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

        def new():
            lib.vqhmm_code_viterbi_f32(P(hmm.log_pi), P(hmm.log_A), P(hmm.log_B), P(codes), P(L), B, T, S, V, P(path),
                                       P(score), P(ws), nb, st)

        def old():
            return vqhmm.viterbi(hmm.log_pi, hmm.log_A.expand(B, T, S, S), hmm.log_B[:, cl].permute(1, 2, 0), L)

        out_bytes = 4
    else:
        filt = torch.empty(B, T, S, device="cuda")
        last = torch.empty(B, S, device="cuda")
        ll = torch.empty(B, device="cuda")
        nb = lib.vqhmm_code_filter_workspace_size(B, T, S, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")

        def new():
            lib.vqhmm_code_filter_f32(P(hmm.log_pi), P(hmm.log_A), P(hmm.log_B), P(codes), P(L), None, B, T, S, V,
                                      P(filt), P(last), P(ll), P(ws), nb, st)

        def old():
            return vqhmm.forward_filter(hmm.log_pi, hmm.log_A.expand(B, T, S, S), hmm.log_B[:, cl].permute(1, 2, 0), L)

        out_bytes = 4 * S
    legs = {leg: new}
    if a.old_route:
        legs["old_route"] = old
        ref = old()
        new()
        torch.cuda.synchronize()
        if leg == "code_viterbi":
            chk = {"paths_equal": bool(torch.equal(ref[0], path)),
                   "scores_equal": bool(torch.equal(ref[1].view(torch.int32), score.view(torch.int32)))}
        else:
            chk = {"filt_maxdiff": (ref[0] - filt).abs().max().item(),
                   "loglik_max_rel": ((ref[1] - ll).abs() / ll.abs().clamp(min=1)).max().item()}
        print(json.dumps({"check": "old_route vs " + leg, "B": B, "T": T, "S": S, "V": V, **chk}))
    for fn in legs.values():
        time_fn(fn, iters=3, warmup=2)
    rounds = {k: [] for k in legs}
    for _ in range(5):
        for k, fn in legs.items():
            rounds[k].append(time_fn(fn, iters=10, warmup=1))
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    n = B * T
    byts = {leg: n * (4 + out_bytes), "old_route": n * (2 * (4 * S * S + 4 * S) + 4 + out_bytes)}
    for k in legs:
        rec = {"kernel": k, "B": B, "T": T, "S": S, "V": V, "us": t[k] * 1e6, "pairs_us": [r * 1e6 for r in rounds[k]],
               "GBps": byts[k] / t[k] / 1e9, "frac_hbm": byts[k] / t[k] / HBM_PEAK}
        if k == "old_route":
            rec["x_" + leg] = t[k] / t[leg]
            rec["fused_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds[leg]))
        print(json.dumps(rec))


def bench_code_viterbi(a):
    _bench_code_decode(a, "code_viterbi")


def bench_code_filter(a):
    _bench_code_decode(a, "code_filter")


def _bench_gauss_decode(a, leg):
    """One of GaussianHMM's fused read-outs on x (B,T,--D) at S = --K states, full-length sequences; --full: full
    covariances.  --old-route: also the time-varying kernels' way to the same result (the emission entry into
    (B,T,S), log_A expanded to (B,T,S,S), then viterbi / forward_filter; building the tables is part of its
    time), in five alternating pairs after a warm-up, every pair's two times reported, and a line that checks the
    two routes agree.  The gauss_filter leg also times the E-step of the same shape in the same pairs: the filter
    is its forward half and has to stay below it.  Algorithmic HBM bytes per position: x read (4 D) and the
    backpointers written and read back (2 SP) plus the path (4), or filt (4 S) written."""
    B, T, S, D = a.B, a.T, a.K, a.D
    if a.full:
        hmm, x, L, _ = _full_case(B, T, S, D)
    else:
        g = torch.Generator(device="cuda").manual_seed(11)
        hmm = vqhmm.GaussianHMM(S, D, generator=torch.Generator().manual_seed(3)).cuda()
        with torch.no_grad():
            hmm.mean.mul_(2.0)
        z = torch.randint(0, S, (B, T), device="cuda", generator=g)
        x = (hmm.mean[z] + torch.randn((B, T, D), device="cuda", generator=g)).contiguous()
        L = torch.full((B,), T, dtype=torch.int64, device="cuda")
    log_pi, log_A, mean, par = hmm._params()
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    pre = "vqhmm_gauss_full_" if a.full else "vqhmm_gauss_"
    legs = {}
    if leg == "gauss_viterbi":
        path = torch.empty(B, T, dtype=torch.int32, device="cuda")
        score = torch.empty(B, device="cuda")
        nb = getattr(lib, pre + "viterbi_workspace_size")(B, T, S, D)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
        entry = getattr(lib, pre + "viterbi_f32")

        def new():
            entry(P(log_pi), P(log_A), P(mean), P(par), P(x), P(L), B, T, S, D, P(path), P(score), P(ws), nb, st)

        def old():
            return vqhmm.viterbi(log_pi, log_A.expand(B, T, S, S), hmm.emission_log_prob(x, L), L)

        SP = 1 << max(S - 1, 0).bit_length()
        byts = B * T * (4 * D + 2 * SP + 4)
        legs[leg] = new
    else:
        filt = torch.empty(B, T, S, device="cuda")
        last = torch.empty(B, S, device="cuda")
        ll = torch.empty(B, device="cuda")
        entry = getattr(lib, pre + "filter_f32")

        def new():
            entry(P(log_pi), P(log_A), P(mean), P(par), P(x), P(L), None, B, T, S, D, P(filt), P(last), P(ll), st)

        def old():
            return vqhmm.forward_filter(log_pi, log_A.expand(B, T, S, S), hmm.emission_log_prob(x, L), L)

        def estep():
            return hmm.log_prob(x, L)

        byts = B * T * (4 * D + 4 * S)
        legs[leg] = new
        legs["estep"] = estep
    if a.old_route:
        legs["old_route"] = old
        ref = old()
        new()
        torch.cuda.synchronize()
        if leg == "gauss_viterbi":
            chk = {"paths_equal": bool(torch.equal(ref[0], path)),
                   "scores_equal": bool(torch.equal(ref[1].view(torch.int32), score.view(torch.int32)))}
        else:
            chk = {"filt_maxdiff": (ref[0] - filt).abs().max().item(),
                   "loglik_max_rel": ((ref[1] - ll).abs() / ll.abs().clamp(min=1)).max().item()}
        print(json.dumps({"check": "old_route vs " + leg, "B": B, "T": T, "S": S, "D": D, "full": a.full, **chk}))
        del ref
    rounds = _pairs(legs)
    dims = {"B": B, "T": T, "S": S, "D": D, "full": a.full}
    _report(legs, rounds, leg, dims, lambda t: {"GBps": byts / t / 1e9, "frac_hbm": byts / t / HBM_PEAK})


def bench_gauss_viterbi(a):
    _bench_gauss_decode(a, "gauss_viterbi")


def bench_gauss_filter(a):
    _bench_gauss_decode(a, "gauss_filter")


def _bench_vq_codebook(a, leg):
    """vqhmm_vq_stats_f32 or vqhmm_vq_quantize_bwd_f32 on the argmin's indices of random z.  --old-route: also
    the torch route to the same numbers (vq_stats: bincount + a permuted index_add_ of the residuals in fp64;
    vq_bwd: _Quantize.backward, the gather, the permuted difference and the fp32 index_add_), in five alternating
    pairs after a warm-up, every pair's two times reported, and a line that checks the two routes agree on the
    timed inputs.  Algorithmic HBM bytes per position: z read (4 Dv) and the code (4); the backward also reads
    g_zq and writes dz (8 Dv)."""
    B, Dv, T, K = a.B, a.Dv, a.T, a.K
    g = torch.Generator(device="cuda").manual_seed(1234)
    z = torch.randn(B, Dv, T, device="cuda", generator=g)
    cb = torch.randn(K, Dv, device="cuda", generator=g)
    g_zq = torch.randn(B, Dv, T, device="cuda", generator=g)
    idx = vqhmm.vq_argmin(z, cb)
    il = idx.long()
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    n = float(z.numel())
    beta = 0.25
    if leg == "vq_stats":
        flat = torch.empty(K + K * Dv + 1, dtype=torch.float64, device="cuda")
        nb = lib.vqhmm_vq_stats_workspace_size(B, Dv, T, K)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")

        def new():
            lib.vqhmm_vq_stats_f32(P(z), P(idx), None, B, Dv, T, P(cb), K, P(flat[:K]), P(flat[K:K + K * Dv]),
                                   P(flat[K + K * Dv:]), P(ws), nb, st)

        def old():
            count = torch.bincount(il.reshape(-1), minlength=K).double()
            r = (z - cb[il].permute(0, 2, 1)).permute(0, 2, 1).reshape(-1, Dv).double()
            rsum = torch.zeros(K, Dv, dtype=torch.float64, device="cuda").index_add_(0, il.reshape(-1), r)
            return count, rsum, (r * r).sum()

        out_bytes = 0
    else:
        dz = torch.empty_like(z)
        dcb = torch.empty_like(cb)
        one = torch.ones((), device="cuda")
        dzs = torch.full((1,), 2.0 * beta / n, device="cuda")
        dcs = torch.full((1,), -2.0 / n, device="cuda")
        nb = lib.vqhmm_vq_quantize_bwd_workspace_size(B, Dv, T, K)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")

        def new():
            lib.vqhmm_vq_quantize_bwd_f32(P(z), P(idx), None, B, Dv, T, P(cb), K, P(g_zq), P(dzs), P(dcs), P(dz),
                                          P(dcb), P(ws), nb, st)

        class Ctx:
            saved_tensors = (z, cb, idx)
            needs_input_grad = (True, True, False)

        Ctx.beta, Ctx.n = beta, n
        from vqhmm.hmm import _Quantize

        def old():
            return _Quantize.backward(Ctx, g_zq, None, one, one)

        out_bytes = 8 * Dv
    legs = {leg: new}
    if a.old_route:
        legs["old_route"] = old
        ref = old()
        new()
        torch.cuda.synchronize()
        if leg == "vq_stats":
            chk = {"count_equal": bool(torch.equal(ref[0], flat[:K])),
                   "rsum_maxdiff": (ref[1].reshape(-1) - flat[K:K + K * Dv]).abs().max().item(),
                   "sse_rel": abs((ref[2] - flat[-1]).item()) / max(flat[-1].item(), 1e-300)}
        else:
            chk = {"dz_maxdiff": (ref[0] - dz).abs().max().item(), "dcb_maxdiff": (ref[1] - dcb).abs().max().item(),
                   "dcb_max": dcb.abs().max().item()}
        print(json.dumps({"check": "old_route vs " + leg, "B": B, "Dv": Dv, "T": T, "K": K, **chk}))
    for fn in legs.values():
        time_fn(fn, iters=3, warmup=2)
    rounds = {k: [] for k in legs}
    for _ in range(5):
        for k, fn in legs.items():
            rounds[k].append(time_fn(fn, iters=10, warmup=1))
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    byts = B * T * (4 * Dv + 4 + out_bytes)
    for k in legs:
        rec = {"kernel": k, "B": B, "Dv": Dv, "T": T, "K": K, "us": t[k] * 1e6,
               "pairs_us": [r * 1e6 for r in rounds[k]], "GBps": byts / t[k] / 1e9, "frac_hbm": byts / t[k] / HBM_PEAK}
        if k == "old_route":
            rec["x_" + leg] = t[k] / t[leg]
            rec["fused_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds[leg]))
        print(json.dumps(rec))


def bench_vq_stats(a):
    _bench_vq_codebook(a, "vq_stats")


def bench_vq_bwd(a):
    _bench_vq_codebook(a, "vq_bwd")


def bench_gauss_scenario(a):
    """GaussianHMM.simulate (vqhmm_gauss_scenario_f32) at --B starts x --N paths x --T steps, S = --K states, --D
    assets; --full: full covariances.  Two legs of the new call: final + drawdown only, and the same with x written.
    --old-route: also what could be assembled before it: simulate_paths on log_A expanded to (B,T,S,S), torch.randn
    (B,N,T,D), the gather of the means plus a scale multiply (diag) or S masked matmuls (full, GaussianHMM.sample's
    way) for x, and torch ops (cumprod / cummax in fp64) for the wealth; five alternating pairs after a warm-up.
    Every start has the same regime distribution (simulate_paths takes one log_pi), and the two routes draw
    different random numbers, so the check line compares the two routes' mean and standard deviation of the final
    wealth in units of their standard errors.  valu_frac: an instruction-count estimate of the kernel's arithmetic
    (per Philox block 10 rounds of about 10 integer operations; per four normals about 100; the triangular or
    diagonal fma's; 4 D for the fp64 wealth) over 256 CUs x 64 lanes x 2.4 GHz."""
    B, N, H, S, D = a.B, a.N, a.T, a.K, a.D
    kind = "full" if a.full else "diag"
    gen = torch.Generator().manual_seed(3)
    hmm = vqhmm.GaussianHMM(S, D, covariance_type=kind, generator=gen)
    with torch.no_grad():
        hmm.mean.mul_(1e-3)
        if a.full:
            Lc = torch.randn((S, D, D), generator=gen).tril(-1) * (0.4 / math.sqrt(D))
            hmm.scale_tril.copy_(1e-2 * (Lc + torch.diag_embed(torch.rand((S, D), generator=gen) + 0.6)))
        else:
            hmm.log_var.copy_(2 * torch.log(1e-2 * (0.5 + torch.rand((S, D), generator=gen))))
    hmm = hmm.cuda()
    port = torch.rand((S, D), generator=gen)
    port = (port / port.sum(1, keepdim=True)).cuda()
    reb, tx = 5, 1e-3
    state = torch.exp(hmm.log_pi.detach()).expand(B, S).contiguous()
    start = hmm.predict_next(state)[0]
    log_p0 = torch.log(start[0]).contiguous()
    log_A = hmm.log_A.detach()
    mean = hmm.mean.detach()
    scale = hmm.scale_tril.detach().tril() if a.full else torch.exp(0.5 * hmm.log_var.detach())
    tt = torch.arange(H, device="cuda")
    last_reb = tt - tt % reb                       # the step whose regime's holdings are held at t
    is_reb = (tt % reb == 0)

    def new_final():
        return hmm.simulate(H, N, state=state, seed=1, weights=port, rebalance=reb, tx_cost=tx)

    def new_x():
        return hmm.simulate(H, N, state=state, seed=1, weights=port, rebalance=reb, tx_cost=tx, return_x=True)

    def old():
        z = vqhmm.simulate_paths(log_p0, log_A.expand(B, H, S, S), n_samples=N).long()
        eps = torch.randn((B, N, H, D), device="cuda")
        if a.full:
            x = mean[z]
            for s in range(S):
                x = x + (z == s).unsqueeze(-1) * (eps @ scale[s].T)
        else:
            x = torch.addcmul(mean[z], scale[z], eps)
        hz = z[:, :, last_reb]
        held = port[hz]
        r = (held.double() * x.double()).sum(-1)
        prev = torch.cat([torch.zeros_like(held[:, :, :1]), held[:, :, :-1]], 2)
        turn = (held.double() - prev.double()).abs().sum(-1) * is_reb
        w = torch.cumprod((1.0 - tx * turn) * (1.0 + r), -1)
        peak = torch.cummax(w, -1).values.clamp_min(1.0)
        return w[..., -1].float(), (1.0 - w / peak).amax(-1).clamp_min(0.0).float(), x

    legs = {"gauss_scenario": new_final, "gauss_scenario_x": new_x}
    dims = {"B": B, "N": N, "H": H, "S": S, "D": D, "full": a.full}
    if a.old_route:
        legs["old_route"] = old
        res = new_x()
        fo, do, xo = old()
        torch.cuda.synchronize()
        n = B * N
        fn_, fo_ = res.final.double().flatten(), fo.double().flatten()
        se_mean = math.sqrt((fn_.var().item() + fo_.var().item()) / n)
        chk = {"final_mean": [fn_.mean().item(), fo_.mean().item()], "final_std": [fn_.std().item(), fo_.std().item()],
               "final_mean_diff_in_se": abs(fn_.mean().item() - fo_.mean().item()) / se_mean,
               "drawdown_mean": [res.drawdown.double().mean().item(), do.double().mean().item()],
               "x_mean_maxdiff": (res.x.double().mean((0, 1, 2)) - xo.double().mean((0, 1, 2))).abs().max().item(),
               "x_std_max_rel": ((res.x.double().std((0, 1, 2)) / xo.double().std((0, 1, 2))) - 1).abs().max().item()}
        print(json.dumps(dict({"check": "old_route vs gauss_scenario"}, **dims, **chk)))
        del res, fo, do, xo, fn_, fo_
    rounds = _pairs(legs)
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    nb = (D + 3) // 4
    ops = B * N * H * ((1 + nb) * 100 + nb * 100 + (D * (D + 1) // 2 if a.full else D) + 4 * D)
    for k in legs:
        rec = dict({"kernel": k}, **dims, us=t[k] * 1e6, min_us=min(rounds[k]) * 1e6, max_us=max(rounds[k]) * 1e6,
                   pairs_us=[r * 1e6 for r in rounds[k]])
        if k == "old_route":
            for new in ("gauss_scenario", "gauss_scenario_x"):
                rec["x_" + new] = t[k] / t[new]
                rec[new + "_faster_in_every_pair"] = all(o > f for o, f in zip(rounds[k], rounds[new]))
        else:
            byts = B * N * 8 + (B * N * H * D * 4 if k.endswith("_x") else 0)
            rec.update(GBps=byts / t[k] / 1e9, frac_hbm=byts / t[k] / HBM_PEAK, valu_ops=ops,
                       valu_frac=ops / t[k] / (256 * 64 * 2.4e9))
        print(json.dumps(rec))


def bench_backtest(a):
    """vqhmm.backtest (vqhmm_backtest_f32; with --bwd also an objective on Backtest.metrics() and its backward,
    vqhmm_backtest_bwd_f32) at --B windows x --T steps, S = --K regimes, --D assets, --P weight tables, rebalance 5,
    tx_cost 1e-3, lag 1, full lengths; --hard: mode="hard".  --old-route: also the straightforward torch fp64
    restatement: H = einsum(probs[:, dates - lag], W), a gather of H to the steps, (held r).sum(-1), the dates'
    diff().abs().sum(-1), cumprod, cummax and the sums (a (B,P,T,D) fp64 intermediate), with --bwd torch autograd
    through it; five alternating pairs after a warm-up.  The check line compares the two routes' stats (and with
    --bwd the gradients of the objective) against tol = 4 (T + S + D + B + 8) 2^-53 mag, mag the sum of the
    absolute values of the terms that enter each output (tests/backtest_ref.py's rule, evaluated in torch)."""
    B, T, S, D, P = a.B, a.T, a.K, a.D, a.P
    R, cost, lag = 5, 1e-3, 1
    g = torch.Generator(device="cuda").manual_seed(21)
    r = (1e-3 + 1e-2 * torch.randn((B, T, D), device="cuda", generator=g)).contiguous()
    logit = torch.randn((B, T, S), device="cuda", generator=g).cumsum(1) * 0.5
    probs = torch.softmax(logit - logit.mean(2, keepdim=True), 2).contiguous()
    W0 = torch.rand((P, S, D), device="cuda", generator=g) + 0.1
    W0 = (W0 / W0.sum(2, keepdim=True)).contiguous()
    reb = torch.full((P,), R, dtype=torch.int32, device="cuda")
    txc = torch.full((P,), cost, dtype=torch.float32, device="cuda")
    c64 = float(txc[0].double())
    mode = "hard" if a.hard else "soft"
    tt = torch.arange(T, device="cuda")
    dates = torch.arange(lag, T, R, device="cuda")
    kidx = ((tt - lag).clamp_min(0) // R)
    live = (tt >= lag).double()[:, None]
    r64 = r.double()

    def rows():
        q = probs[:, dates - lag].double()
        if a.hard:
            q = torch.nn.functional.one_hot(q.argmax(2), S).double()
        return q

    def old_stats(W):
        q = rows()                                                   # (B,K,S)
        H = torch.einsum("bks,psd->bpkd", q, W.double())
        held = H[:, :, kidx] * live                                  # (B,P,T,D)
        gr = (held * r64[:, None]).sum(-1)
        tauk = torch.cat([H[:, :, :1], H.diff(dim=2)], 2).abs().sum(-1)
        tau = torch.zeros_like(gr).index_copy(2, dates, tauk)
        rho = (1.0 - c64 * tau) * (1.0 + gr) - 1.0
        V = torch.cumprod(1.0 + rho, -1)
        cm = torch.cummax(V, -1)
        peak = cm.values.clamp_min(1.0)
        dds = 1.0 - V / peak
        dd, jt = dds.max(-1)
        it = torch.where(cm.values.gather(2, jt[..., None])[..., 0] > 1.0, cm.indices.gather(2, jt[..., None])[..., 0],
                         torch.full_like(jt, -1))
        none = dd <= 0
        neg = rho < 0
        rn = torch.where(neg, rho, torch.zeros_like(rho))
        n = torch.full_like(dd, float(T))
        cols = [V[..., -1], n, rho.sum(-1), (rho * rho).sum(-1), neg.sum(-1).double(), rn.sum(-1), (rn * rn).sum(-1),
                (rho > 0).sum(-1).double(), dd, tau.sum(-1), torch.where(none, -torch.ones_like(dd), it.double()),
                torch.where(none, -torch.ones_like(dd), jt.double())]
        return torch.stack(cols, -1), (rho, gr, tau, q)

    def objective(stats):
        m = vqhmm.Backtest(stats).metrics()
        return (-m["sharpe"] + 0.1 * stats[..., 8] + 0.01 * stats[..., 9] - torch.log(stats[..., 0])
                + m["sortino"]).sum()

    def new_fwd():
        return vqhmm.backtest(r, probs, W0, rebalance=reb, tx_cost=txc, lag=lag, mode=mode).stats

    def old_fwd():
        with torch.no_grad():
            return old_stats(W0)[0]

    def new_bwd():
        W = W0.clone().requires_grad_(True)
        objective(vqhmm.backtest(r, probs, W, rebalance=reb, tx_cost=txc, lag=lag, mode=mode).stats).backward()
        return W.grad

    def old_bwd():
        W = W0.clone().requires_grad_(True)
        objective(old_stats(W)[0]).backward()
        return W.grad

    name = "backtest_bwd" if a.bwd else "backtest"
    legs = {name: new_bwd if a.bwd else new_fwd}
    dims = {"B": B, "T": T, "S": S, "D": D, "P": P, "mode": mode}
    if a.old_route:
        legs["old_route"] = old_bwd if a.bwd else old_fwd
        k = 4.0 * (T + S + D + B + 8) * 2.0 ** -53
        with torch.no_grad():
            so, (rho, gr, tau, q) = old_stats(W0)
            sn = new_fwd()
            Wa = W0.double().abs()
            Ha = torch.einsum("bks,psd->bpkd", q.abs(), Wa)
            gabs = (Ha[:, :, kidx] * live * r64[:, None].abs()).sum(-1)
            tabk = (Ha + torch.cat([torch.zeros_like(Ha[:, :, :1]), Ha[:, :, :-1]], 2)).sum(-1)
            tabs = torch.zeros_like(gr).index_copy(2, dates, tabk)
            terms = (1.0 + c64 * tabs) * (1.0 + gabs)
            rel = terms / (1.0 + rho).abs()
            rt = terms + 1.0
            sq = 2.0 * rho.abs() * rt + rho * rho
            neg = rho < 0
            inside = (tt > so[..., 10, None]) & (tt <= so[..., 11, None])
            zero = torch.zeros_like(rt)
            mag = {0: so[..., 0].abs() * rel.sum(-1), 2: rt.sum(-1), 3: sq.sum(-1), 5: torch.where(neg, rt, zero).sum(-1),
                   6: torch.where(neg, sq, zero).sum(-1), 9: tabs.sum(-1),
                   8: 1.0 + (1.0 - so[..., 8]) * (1.0 + torch.where(inside, rel, zero).sum(-1))}
            chk = {"int_columns_equal": bool(all(torch.equal(so[..., c], sn[..., c]) for c in (1, 4, 7, 10, 11)))}
            worst = 0.0
            for c, m in mag.items():
                worst = max(worst, ((so[..., c] - sn[..., c]).abs() / (k * m)).max().item())
            chk["stats_err_over_tol"] = worst
        if a.bwd:
            W = W0.clone().double().requires_grad_(True)
            bt = vqhmm.backtest(r, probs, W, rebalance=reb, tx_cost=txc, lag=lag, mode=mode)
            bt.stats.retain_grad()
            objective(bt.stats).backward()
            gs = bt.stats.grad
            Wo = W0.clone().double().requires_grad_(True)
            objective(old_stats(Wo)[0]).backward()
            with torch.no_grad():
                ins = inside.double()
                A = (gs[..., 2, None].abs() + 2 * rho.abs() * gs[..., 3, None].abs()
                     + neg * (gs[..., 5, None].abs() + 2 * rho.abs() * gs[..., 6, None].abs())
                     + (gs[..., 0, None] * so[..., 0, None]).abs() / (1 + rho).abs()
                     + ins * (gs[..., 8, None].abs() * (1 - so[..., 8, None])) / (1 + rho).abs())
                qs = q[:, kidx] * live[None]                                      # (B,T,S)
                m1 = torch.einsum("bpt,bts,btd->psd", A * (1 - c64 * tau).abs() * live[:, 0], qs.abs(), r64.abs())
                dq = torch.cat([q[:, :1], q.diff(dim=1)], 1).abs()                 # (B,K,S)
                uab = gs[..., 9, None].abs() + c64 * (1 + gr.abs()[:, :, dates]) * A[:, :, dates]
                m2 = torch.einsum("bpk,bks->ps", uab, dq)[..., None]
                err = (W.grad - Wo.grad).abs()
                chk["grad_err_over_tol"] = (err / (k * (m1 + m2))).max().item()
                chk["grad_max_rel"] = (err.max() / Wo.grad.abs().max()).item()
            del bt, gs, A, qs, m1, m2, W, Wo
        chk["agree"] = bool(chk["int_columns_equal"] and chk["stats_err_over_tol"] <= 1.0
                            and chk.get("grad_err_over_tol", 0.0) <= 1.0)
        print(json.dumps(dict({"check": "old_route vs " + name}, **dims, **chk)))
        del so, sn, rho, gr, tau, q, Ha, gabs, tabs, terms, rel, rt, sq, mag
        torch.cuda.empty_cache()
    rounds = _pairs(legs)
    t = {k_: sorted(v)[len(v) // 2] for k_, v in rounds.items()}
    for k_ in legs:
        rec = dict({"kernel": k_}, **dims, us=t[k_] * 1e6, min_us=min(rounds[k_]) * 1e6, max_us=max(rounds[k_]) * 1e6,
                   pairs_us=[x * 1e6 for x in rounds[k_]])
        if k_ == "old_route":
            rec["x_" + name] = t[k_] / t[name]
            rec["fused_not_slower_in_any_pair"] = all(o >= f for o, f in zip(rounds[k_], rounds[name]))
        else:
            byts = 4 * B * T * (D + S) + 96 * B * P
            rec.update(GBps=byts / t[k_] / 1e9, frac_hbm=byts / t[k_] / HBM_PEAK)
        print(json.dumps(rec))


def torch_ffbs(filt, log_A, u):
    """Plain-torch FFBS on full-length sequences, one step per iteration: a gather of the column
    z_t, a cumsum and a searchsorted (several launches per time step)."""
    B, T, K = filt.shape
    N = u.shape[1]
    paths = torch.empty(B, N, T, dtype=torch.int64, device=filt.device)

    def draw(w, ut):  # w (B, N, K), ut (B, N)
        c = torch.cumsum(w, dim=2)
        thr = (ut * c[:, :, -1]).unsqueeze(2)
        return torch.searchsorted(c, thr, right=True).squeeze(2).clamp_(max=K - 1)

    z = draw(filt[:, T - 1].unsqueeze(1).expand(B, N, K), u[:, :, T - 1])
    paths[:, :, T - 1] = z
    for t in range(T - 1, 0, -1):
        col = torch.gather(log_A[:, t].transpose(1, 2), 1, z.unsqueeze(2).expand(B, N, K))  # log_A_t(:, z_t)
        w = filt[:, t - 1].unsqueeze(1) * torch.exp(col - col.max(dim=2, keepdim=True).values)
        z = draw(w, u[:, :, t - 1])
        paths[:, :, t - 1] = z
    return paths


def bench_sample(a):
    """vqhmm_ffbs_sample_f32 and vqhmm_markov_sample_f32 at N = --N samples per sequence, the filter
    (FFBS's forward half) and the plain-torch FFBS loop, alternated after a warm-up (median, min and
    max of the rounds).  Algorithmic bytes of a sampler: 4 B T (K^2 + K) + 8 B N T (the tables and
    filt read once, the uniforms read and the paths written)."""
    B, T, K, N = a.B, a.T, a.K, a.N
    log_pi, log_A, em, L = hmm_tables(B, T, K)
    lib = vqhmm._ext.load()
    P = vqhmm._ext.ptr
    st = vqhmm._ext.stream_ptr()
    filt = torch.empty(B, T, K, device="cuda")
    ll = torch.empty(B, device="cuda")
    u = torch.rand(B, N, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    pf = torch.empty(B, N, T, dtype=torch.int32, device="cuda")
    pm = torch.empty(B, N, T, dtype=torch.int32, device="cuda")

    def filt_fn():
        lib.vqhmm_filter_f32(P(log_pi), P(log_A), P(em), P(L), B, T, K, P(filt), P(ll), st)

    def ffbs():
        lib.vqhmm_ffbs_sample_f32(P(filt), P(log_A), P(L), P(u), B, T, K, N, P(pf), st)

    def markov():
        lib.vqhmm_markov_sample_f32(P(log_pi), P(log_A), P(L), P(u), B, T, K, N, P(pm), st)

    filt_fn()
    ffbs()
    ref = torch_ffbs(filt, log_A, u)
    torch.cuda.synchronize()
    print(json.dumps({"check": "torch loop vs ffbs kernel", "B": B, "T": T, "K": K, "N": N,
                      "rows_differing": int((ref != pf.long()).any(dim=2).sum()), "rows": B * N}))
    legs = {"filter": filt_fn, "ffbs_sample": ffbs, "markov_sample": markov,
            "torch_ffbs_loop": lambda: torch_ffbs(filt, log_A, u)}
    iters = {"filter": 10, "ffbs_sample": 10, "markov_sample": 10, "torch_ffbs_loop": 1}
    for k, fn in legs.items():
        time_fn(fn, iters=2 if k != "torch_ffbs_loop" else 1, warmup=2 if k != "torch_ffbs_loop" else 1)
    rounds = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            rounds[k].append(time_fn(fn, iters=iters[k], warmup=1 if k != "torch_ffbs_loop" else 0))
    t = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    byts = 4 * B * T * (K * K + K) + 8 * B * N * T
    for k in legs:
        rec = {"kernel": k, "B": B, "T": T, "K": K, "N": N, "us": t[k] * 1e6, "min_us": min(rounds[k]) * 1e6,
               "max_us": max(rounds[k]) * 1e6}
        if k.endswith("_sample"):
            rec.update({"GBps": byts / t[k] / 1e9, "frac_hbm": byts / t[k] / HBM_PEAK, "x_filter": t[k] / t["filter"]})
        if k == "torch_ffbs_loop":
            rec["x_ffbs_sample"] = t[k] / t["ffbs_sample"]
        print(json.dumps(rec))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what")
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--Dv", type=int, default=64)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--V", type=int, default=512)
    ap.add_argument("--D", type=int, default=16)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--M", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--old-route", action="store_true")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--P", type=int, default=8)
    ap.add_argument("--hard", action="store_true")
    ap.add_argument("--bwd", action="store_true")
    a = ap.parse_args()
    {"vq": bench_vq, "stream": bench_stream, "viterbi": bench_viterbi, "fwdbwd": bench_fwdbwd,
     "filter": bench_filter, "xi": bench_xi, "estep": bench_estep, "estep_batched": bench_estep_batched,
     "gauss_estep": bench_gauss_estep, "gauss_full_estep": bench_gauss_full_estep,
     "gauss_estep_batched": bench_gauss_estep_batched,
     "gauss_moments": bench_gauss_moments, "code_fit": bench_code_fit, "code_viterbi": bench_code_viterbi,
     "code_filter": bench_code_filter, "gauss_viterbi": bench_gauss_viterbi, "gauss_filter": bench_gauss_filter,
     "sample": bench_sample, "vq_stats": bench_vq_stats, "gauss_scenario": bench_gauss_scenario,
     "vq_bwd": bench_vq_bwd, "backtest": bench_backtest}[a.what](a)
