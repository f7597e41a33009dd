"""numpy restatements of GaussianHMM's decode and causal filter on a given emission tensor (a helper for the
tests, not a test).  The kernels compute their emissions on chip; the tests feed these functions the tensor the
emission entry wrote, which the kernels reproduce bit for bit.

  viterbi_em_f32  the fp32 max-plus rule of include/vqhmm.h, op for op, so the kernel is compared bit for bit:
                    d_0[j] = log_pi[j] + em[0,j],  d_t[j] = (max_i (d_{t-1}[i] + log_A[i,j])) + em[t,j]
                  i ascending with a strict >, last = first argmax of d_{L-1}
  filter_em_ref   the fp64 log-space causal filter with the carried state `prev` and `last`
  brute_*         enumeration of the S^L paths: the best path weight and the prefix marginals

Conventions of include/vqhmm.h: length 0 -> path all -1, score -inf, loglik NaN, last = prev (or zeros); a
non-finite emission inside the length (what a non-finite x gives) -> path all -1 and score NaN; loglik NaN,
filt rows from the first such position on and last 0, the positions before it filtered as usual; an impossible
sequence (mass 0, or sum(prev) 0 or not finite) -> loglik -inf, the same zero rows.
"""
import itertools

import numpy as np

from code_decode_ref import clamp_lengths
from hmm_pair_ref import lse


def viterbi_em_f32(log_pi, log_A, em, lengths=None):
    """em (B,T,S) -> path (B,T) int32, score (B,) float32."""
    log_pi = np.asarray(log_pi, np.float32)
    log_A = np.asarray(log_A, np.float32)
    em = np.asarray(em, np.float32)
    B, T, S = em.shape
    Ls = clamp_lengths(lengths, B, T)
    path = np.full((B, T), -1, np.int32)
    score = np.full(B, -np.inf, np.float32)
    if T == 0:
        return path, score
    inside = np.arange(T)[None, :] < Ls[:, None]
    bad = (inside[:, :, None] & ~np.isfinite(em)).any((1, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        # all sequences step together (every operation is one fp32 add or compare, as in the rule)
        d = log_pi[None, :] + em[:, 0]
        hist = [d]
        bp = np.zeros((B, T, S), np.int64)
        for t in range(1, T):
            best = d[:, 0, None] + log_A[None, 0, :]
            arg = np.zeros((B, S), np.int64)
            for i in range(1, S):
                v = d[:, i, None] + log_A[None, i, :]
                gt = v > best
                best = np.where(gt, v, best)
                arg = np.where(gt, i, arg)
            d = best + em[:, t]
            assert d.dtype == np.float32
            hist.append(d)
            bp[:, t] = arg
        for b in range(B):
            L = int(Ls[b])
            if L == 0:
                continue
            if bad[b]:
                score[b] = np.nan
                continue
            dl = hist[L - 1][b]
            last = 0
            for j in range(1, S):
                if dl[j] > dl[last]:
                    last = j
            score[b] = dl[last]
            s = last
            for t in range(L - 1, -1, -1):
                path[b, t] = s
                s = bp[b, t, s]
    return path, score


def expand_log_A(log_A, B, T):
    """The time-varying route's transition table: log_A (S,S) broadcast to (B,T,S,S), materialised."""
    log_A = np.asarray(log_A, np.float32)
    return np.ascontiguousarray(np.broadcast_to(log_A, (B, T) + log_A.shape))


def filter_em_ref(log_pi, log_A, em, lengths=None, prev=None, want_masses=False):
    """em (B,T,S) -> dict(filt (B,T,S), last (B,S), loglik (B,)) float64 [, masses: the kernel's linear step
    masses c_t (B,T), computed with e_t = exp(em_t - max em_t): the quantity whose range decides its fast step]."""
    log_A = np.asarray(log_A, np.float64)
    em = np.asarray(em, np.float64)
    B, T, S = em.shape
    Ls = clamp_lengths(lengths, B, T)
    filt = np.zeros((B, T, S))
    last = np.zeros((B, S))
    loglik = np.full(B, np.nan)
    masses = np.full((B, T), np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            L = int(Ls[b])
            pv = None if prev is None else np.asarray(prev[b], np.float64)
            if L == 0:
                if pv is not None:
                    last[b] = pv
                continue
            if pv is None:
                lx = None
            else:
                if not (pv.sum() > 0 and np.isfinite(pv.sum())):
                    loglik[b] = -np.inf
                    continue
                lx = np.log(pv / pv.sum())
            ll = 0.0
            ok = True
            for t in range(L):
                if not np.isfinite(em[b, t]).all():
                    ll, ok = np.nan, False
                    filt[b, t:] = 0
                    break
                pred = np.asarray(log_pi, np.float64) if lx is None else lse(lx[:, None] + log_A, 0)
                ly = pred + em[b, t]
                z = lse(ly, 0)
                if not np.isfinite(z):
                    ll, ok = -np.inf, False
                    break
                masses[b, t] = np.exp(z - em[b, t].max())
                ll += z
                lx = ly - z
                filt[b, t] = np.exp(lx)
            loglik[b] = ll
            if ok:
                last[b] = filt[b, L - 1]
    out = dict(filt=filt, last=last, loglik=loglik)
    if want_masses:
        out["masses"] = masses
    return out


def path_weight(log_pi, log_A, em, path):
    """fp64 log weight of one state path of one sequence (em (L,S))."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    em = np.asarray(em, np.float64)
    w = log_pi[path[0]] + em[0, path[0]]
    for t in range(1, len(path)):
        w += log_A[path[t - 1], path[t]] + em[t, path[t]]
    return w


def brute_best(log_pi, log_A, em):
    """The best fp64 path weight of one sequence over all S^L paths, and among the paths that attain it the one
    the tie rule selects: the lowest last state, then the lowest state before it, and so on backwards."""
    L, S = np.asarray(em).shape
    best, arg = -np.inf, None
    with np.errstate(invalid="ignore"):
        for q in itertools.product(range(S), repeat=L):
            p = q[::-1]  # the last state varies slowest
            w = path_weight(log_pi, log_A, em, p)
            if arg is None or w > best:
                best, arg = w, p
    return best, np.array(arg)


def brute_filter(log_pi, log_A, em, prev=None):
    """Prefix marginals of one sequence by enumeration: filt (L,S) with filt[t] = p(z_t | x[:t+1]) and loglik =
    log p(x).  prev (S,): the paths start one position earlier, at a state drawn from prev / sum(prev)."""
    L, S = np.asarray(em).shape
    log_A = np.asarray(log_A, np.float64)
    if prev is None:
        start = np.asarray(log_pi, np.float64)
    else:
        pv = np.asarray(prev, np.float64)
        with np.errstate(divide="ignore"):
            start = lse(np.log(pv / pv.sum())[:, None] + log_A, 0)
    filt = np.zeros((L, S))
    z = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(L):
            for p in itertools.product(range(S), repeat=t + 1):
                filt[t, p[-1]] += np.exp(path_weight(start, log_A, em[:t + 1], p))
            z = filt[t].sum()
            filt[t] /= z
        return filt, np.log(z)
