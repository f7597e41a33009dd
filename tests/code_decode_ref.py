"""numpy restatements of CodeHMM's decode and causal filter (a helper for the tests, not a test):

  viterbi_f32   the fp32 max-plus rule of include/vqhmm.h, op for op, so the kernel is compared bit for bit:
                  d_0[j] = log_pi[j] + log_B[j,c_0],  d_t[j] = (max_i (d_{t-1}[i] + log_A[i,j])) + log_B[j,c_t]
                i ascending with a strict >, last = first argmax of d_{L-1}
  filter_ref    the fp64 log-space causal filter with the carried state `prev` and `last`
  brute_*       enumeration of the S^L paths: the best path weight and the prefix marginals

Conventions of include/vqhmm.h: length 0 -> path all -1, score -inf, loglik NaN, last = prev (or zeros);
a code outside [0, V) inside the length -> path all -1 and score NaN; loglik NaN, filt rows from the
failing position on and last 0; an impossible sequence -> loglik -inf, the same zero rows.
"""
import itertools

import numpy as np

from hmm_pair_ref import lse


def clamp_lengths(lengths, B, T):
    L = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    return np.clip(L, 0, T)


def viterbi_f32(log_pi, log_A, log_B, codes, lengths=None):
    """-> path (B,T) int32, score (B,) float32."""
    log_pi = np.asarray(log_pi, np.float32)
    log_A = np.asarray(log_A, np.float32)
    log_B = np.asarray(log_B, np.float32)
    codes = np.asarray(codes)
    B, T = codes.shape
    S, V = log_B.shape
    Ls = clamp_lengths(lengths, B, T)
    path = np.full((B, T), -1, np.int32)
    score = np.full(B, -np.inf, np.float32)
    if T == 0:
        return path, score
    inside = np.arange(T)[None, :] < Ls[:, None]
    bad = (inside & ((codes < 0) | (codes >= V))).any(1)
    c = np.where((codes >= 0) & (codes < V), codes, 0).astype(np.int64)
    em = np.transpose(log_B[:, c], (1, 2, 0))  # (B,T,S) fp32: em[b,t,j] = log_B[j, c_t]
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


def expand_tables(log_A, log_B, codes):
    """The time-varying route's inputs: log_A (B,T,S,S) broadcast, em[b,t,j] = log_B[j, codes[b,t]] (codes
    outside [0, V), i.e. padding, read column 0: those positions are past the lengths)."""
    log_A = np.asarray(log_A, np.float32)
    log_B = np.asarray(log_B, np.float32)
    codes = np.asarray(codes)
    B, T = codes.shape
    S, V = log_B.shape
    c = np.where((codes >= 0) & (codes < V), codes, 0)
    em = np.ascontiguousarray(np.transpose(log_B[:, c], (1, 2, 0)))
    return np.ascontiguousarray(np.broadcast_to(log_A, (B, T, S, S))), em


def filter_ref(log_pi, log_A, log_B, codes, lengths=None, prev=None, want_masses=False):
    """-> dict(filt (B,T,S), last (B,S), loglik (B,)) float64 [, masses: the linear step masses c_t (B,T), the
    quantity whose range decides the kernel's fast step]."""
    log_A = np.asarray(log_A, np.float64)
    log_B = np.asarray(log_B, np.float64)
    codes = np.asarray(codes)
    B, T = codes.shape
    S, V = log_B.shape
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
                if not pv.sum() > 0:
                    loglik[b] = -np.inf
                    continue
                lx = np.log(pv / pv.sum())
            ll = 0.0
            ok = True
            for t in range(L):
                c = int(codes[b, t])
                if c < 0 or c >= V:
                    ll, ok = np.nan, False
                    break
                pred = np.asarray(log_pi, np.float64) if lx is None else lse(lx[:, None] + log_A, 0)
                ly = pred + log_B[:, c]
                z = lse(ly, 0)
                if not np.isfinite(z):
                    ll, ok = -np.inf, False
                    break
                masses[b, t] = np.exp(z)
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


def path_weight(log_pi, log_A, log_B, codes, path):
    """fp64 log weight of one state path of one sequence."""
    log_pi = np.asarray(log_pi, np.float64)
    log_A = np.asarray(log_A, np.float64)
    log_B = np.asarray(log_B, np.float64)
    w = log_pi[path[0]] + log_B[path[0], codes[0]]
    for t in range(1, len(codes)):
        w += log_A[path[t - 1], path[t]] + log_B[path[t], codes[t]]
    return w


def brute_best(log_pi, log_A, log_B, codes):
    """The best fp64 path weight of one sequence over all S^L paths."""
    S = np.asarray(log_B).shape[0]
    return max(path_weight(log_pi, log_A, log_B, codes, p) for p in itertools.product(range(S), repeat=len(codes)))


def brute_filter(log_pi, log_A, log_B, codes):
    """Prefix marginals of one sequence by enumeration: filt (L,S) with filt[t] = p(z_t | codes[:t+1]) and
    loglik = log p(codes)."""
    S = np.asarray(log_B).shape[0]
    L = len(codes)
    filt = np.zeros((L, S))
    z = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(L):
            for p in itertools.product(range(S), repeat=t + 1):
                filt[t, p[-1]] += np.exp(path_weight(log_pi, log_A, log_B, codes[:t + 1], p))
            z = filt[t].sum()
            filt[t] /= z
        return filt, np.log(z)
