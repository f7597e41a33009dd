"""fp64 numpy restatement of the batched / weighted E-step and of the mixture of HMMs on code indices (a helper
for the tests, not a test), built on code_hmm_ref.estep_ref called per member and per sequence:

    member m's counts = sum_b w[m,b] * (sequence b's counts under member m)
    mixture EM: r[m,b] = softmax_m(log_mix[m] + loglik[m,b]) (NaN read as -inf, a column without a finite entry
    all zero), counts with weights r, the M-step of code_hmm_ref, log_mix = log(mean over the scorable b of r)

A model is a tuple (log_pi (S), log_A (S,S), log_B (S,V)); the members of a list may differ in S.
"""
import numpy as np

import code_hmm_ref as R
from hmm_pair_ref import lse


def estep_ens_ref(models, codes, lengths=None, weights=None):
    """-> one dict per member: pi_cnt, trans_cnt, emit_cnt (weighted, float64), loglik (B), and abs_w (B): |w| of
    the sequences that count under that member (finite loglik), 0 elsewhere (what the error bounds scale by)."""
    codes = np.asarray(codes)
    B, T = codes.shape
    lengths = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    W = np.broadcast_to(np.ones(B) if weights is None else np.asarray(weights, np.float64), (len(models), B))
    out = []
    for m, model in enumerate(models):
        S, V = np.asarray(model[2]).shape
        w = W[m]
        acc = dict(pi_cnt=np.zeros(S), trans_cnt=np.zeros((S, S)), emit_cnt=np.zeros((S, V)), loglik=np.full(B, np.nan),
                   abs_w=np.zeros(B))
        for b in range(B):
            one = R.estep_ref(*model, codes[b:b + 1], lengths[b:b + 1])
            acc["loglik"][b] = one["loglik"][0]
            if not np.isfinite(one["loglik"][0]):
                continue
            acc["abs_w"][b] = abs(w[b])
            for k in ("pi_cnt", "trans_cnt", "emit_cnt"):
                acc[k] += w[b] * one[k]
        out.append(acc)
    return out


def weighted_bounds(abs_w, codes, lengths, V):
    """(pi, trans, emit (V,)) bounds of include/vqhmm.h's per-position contracts (gamma 1e-5, xi 2e-5) scaled by
    the weights: 1e-5 sum_b |w_b|, 2e-5 sum_b |w_b| max(L_b - 1, 0), 1e-5 sum_b |w_b| n_{b,v} over the sequences
    that count (abs_w is 0 for the others)."""
    codes = np.asarray(codes)
    B, T = codes.shape
    L = np.clip(np.asarray(lengths, np.int64), 0, T)
    n_v = np.zeros(V)
    for b in range(B):
        if abs_w[b] > 0 and L[b] > 0:
            n_v += abs_w[b] * np.bincount(codes[b, :L[b]], minlength=V)[:V]
    return 1e-5 * (abs_w * (L > 0)).sum(), 2e-5 * (abs_w * np.maximum(L - 1, 0)).sum(), 1e-5 * n_v


def responsibilities_ref(log_mix, loglik):
    """loglik (M,B) -> (r (M,B), ok (B,), total): the rule in the module docstring; total = the mixture
    log-likelihood summed over the scorable sequences."""
    with np.errstate(invalid="ignore"):
        z = np.asarray(log_mix, np.float64)[:, None] + np.where(np.isnan(loglik), -np.inf, loglik)
    ok = np.isfinite(z).any(0)
    z = np.where(ok[None, :], z, 0.0)
    tot = lse(z, 0)
    r = np.where(ok[None, :], np.exp(z - tot[None, :]), 0.0)
    return r, ok, float(tot[ok].sum())


def mixture_ref(models, log_mix, codes, lengths=None, n_iter=5, prior_count=0.0):
    """n_iter iterations of the mixture's EM -> (history (n_iter), models, log_mix, r of the last iteration's
    E-step); every iteration's history entry is under the parameters going in."""
    models = [tuple(np.asarray(a, np.float64) for a in m) for m in models]
    log_mix = np.asarray(log_mix, np.float64)
    hist, r = [], None
    for _ in range(n_iter):
        ll = np.stack([e["loglik"] for e in estep_ens_ref(models, codes, lengths)])
        r, ok, tot = responsibilities_ref(log_mix, ll)
        hist.append(tot)
        st = estep_ens_ref(models, codes, lengths, r)
        models = [R.mstep_ref(st[m], *models[m], prior_count=prior_count) for m in range(len(models))]
        with np.errstate(divide="ignore"):
            log_mix = np.log(r[:, ok].sum(1) / max(int(ok.sum()), 1)) if ok.any() else log_mix
    return np.array(hist), models, log_mix, r


# ------------------------------------------------------------------- shared cases
def sample_codes(model, B, T, seed):
    """B sequences of length T from the model by code_hmm_ref.sample_ref on seeded uniforms -> codes (B,T) int32."""
    u = np.random.default_rng(seed).random((B, T, 2), dtype=np.float32)
    return R.sample_ref(*model, u)[1].astype(np.int32)


# the planted two-cluster mixture case: B = 24, T = 12, S = 2, V = 4, M = 2.  Component 0 lives on codes
# {0, 1}, component 1 on codes {2, 3}; sequences 0..11 are drawn from component 0 and 12..23 from component 1.
# tests/test_code_ens_ref.py checks that the fp64 reference assigns all 24 to their component from this start.
MIX_B, MIX_T, MIX_S, MIX_V, MIX_M = 24, 12, 2, 4, 2


def _logs(a):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(a, np.float64)).astype(np.float32)


def planted_mixture_case():
    """-> (codes (24,12) int32, lengths (24,), labels (24,), start models [2], start log_mix (2,))."""
    planted = [(_logs([0.6, 0.4]), _logs([[0.8, 0.2], [0.3, 0.7]]), _logs([[0.70, 0.20, 0.05, 0.05], [0.15, 0.75, 0.05, 0.05]])),
               (_logs([0.5, 0.5]), _logs([[0.6, 0.4], [0.2, 0.8]]), _logs([[0.05, 0.05, 0.70, 0.20], [0.05, 0.05, 0.10, 0.80]]))]
    half = MIX_B // 2
    codes = np.concatenate([sample_codes(planted[0], half, MIX_T, 11), sample_codes(planted[1], half, MIX_T, 12)])
    lengths = np.full(MIX_B, MIX_T, np.int64)
    lengths[[3, 17]] = [7, 9]
    labels = np.repeat([0, 1], half)
    start = [R.random_model(np.random.default_rng(100 + m), MIX_S, MIX_V, 0.5) for m in range(MIX_M)]
    return codes, lengths, labels, start, np.log(np.full(MIX_M, 1.0 / MIX_M))
