"""fp64 numpy restatement of the codebook-learning contracts (include/vqhmm.h "codebook learning",
vqhmm/codebook.py): the per-code statistics, the quantizer's backward with its fp32 dz rule, the k-means and
EMA updates, the lookup and the perplexity.  Test infrastructure only."""
import numpy as np


def counted(idx, lengths, K):
    """(B,T) bool: t < clamp(lengths[b], 0, T) and 0 <= idx < K."""
    idx = np.asarray(idx)
    B, T = idx.shape
    ok = (idx >= 0) & (idx < K)
    if lengths is not None:
        L = np.clip(np.asarray(lengths, np.int64), 0, T)
        ok &= np.arange(T)[None, :] < L[:, None]
    return ok


def residual_f32(z, idx, lengths, codebook):
    """r (B,Dv,T) fp32 = fl32(z - c[idx]) at counted positions, 0 elsewhere; and the counted mask."""
    z = np.asarray(z, np.float32)
    c = np.asarray(codebook, np.float32)
    ok = counted(idx, lengths, c.shape[0])
    safe = np.where(ok, idx, 0).astype(np.int64)
    zq = np.transpose(c[safe], (0, 2, 1))                      # (B,Dv,T)
    r = (z - zq).astype(np.float32)
    return np.where(ok[:, None, :], r, np.float32(0)), ok


def stats(z, idx, lengths, codebook):
    """-> dict(count (K,), rsum (K,Dv), sse, rabs (K,Dv) = sum |r| per bin), all fp64."""
    c = np.asarray(codebook, np.float32)
    K, Dv = c.shape
    r, ok = residual_f32(z, idx, lengths, c)
    r = r.astype(np.float64)
    count = np.zeros(K)
    rsum = np.zeros((K, Dv))
    rabs = np.zeros((K, Dv))
    kk = np.asarray(idx)[ok].astype(np.int64)                  # (n,)
    rr = np.transpose(r, (0, 2, 1))[ok]                        # (n,Dv)
    np.add.at(count, kk, 1.0)
    np.add.at(rsum, kk, rr)
    np.add.at(rabs, kk, np.abs(rr))
    return {"count": count, "rsum": rsum, "sse": float((rr ** 2).sum()), "rabs": rabs}


def bwd(z, idx, lengths, codebook, g_zq, dz_scale, dcb_scale):
    """-> dz (B,Dv,T) fp32 = fl(g + fl(s r)) (two fp32 roundings), dcodebook (K,Dv) fp64 = dcb_scale * rsum
    (the kernel rounds it to fp32 once)."""
    r, _ = residual_f32(z, idx, lengths, codebook)
    s = np.float32(dz_scale)
    g = np.zeros_like(r) if g_zq is None else np.asarray(g_zq, np.float32)
    p = (s * r).astype(np.float32)
    dz = (g + p).astype(np.float32)
    dcb = float(np.float32(dcb_scale)) * stats(z, idx, lengths, codebook)["rsum"]
    return dz, dcb


def kmeans_step(weight, st):
    """weight[k] + rsum[k] / count[k] where count[k] > 0 (fp64, rounded to fp32 once)."""
    w = np.asarray(weight, np.float32).astype(np.float64)
    cnt = st["count"][:, None]
    return np.where(cnt > 0, w + st["rsum"] / np.maximum(cnt, 1.0), w).astype(np.float32)


def ema_update(weight, ema_count, ema_sum, st, decay, eps):
    """-> (weight fp32, ema_count, ema_sum fp64) after one update."""
    w = np.asarray(weight, np.float32).astype(np.float64)
    K = w.shape[0]
    ec = decay * np.asarray(ema_count, np.float64) + (1.0 - decay) * st["count"]
    es = decay * np.asarray(ema_sum, np.float64) + (1.0 - decay) * (st["rsum"] + st["count"][:, None] * w)
    N = ec.sum()
    smooth = (ec + eps) / (N + K * eps) * N if N > 0 else np.zeros(K)
    live = ec > 0
    new = w.copy()
    new[live] = es[live] / smooth[live, None]
    return new.astype(np.float32), ec, es


def lookup(codebook, idx):
    """(B,Dv,T) fp32 = codebook[idx] channels-first, 0 where idx is outside [0, K)."""
    c = np.asarray(codebook, np.float32)
    idx = np.asarray(idx).astype(np.int64)
    ok = (idx >= 0) & (idx < c.shape[0])
    out = np.transpose(c[np.where(ok, idx, 0)], (0, 2, 1))
    return np.where(ok[:, None, :], out, np.float32(0)).astype(np.float32)


def perplexity(count):
    p = np.asarray(count, np.float64)
    p = p / p.sum()
    nz = p > 0
    return float(np.exp(-(p[nz] * np.log(p[nz])).sum()))
