"""GPU checks of codebook learning (vq_codebook.hip, vqhmm.Codebook) against tests/vq_codebook_ref.py: the
statistics and the backward on every path (odd sizes, tile tails, empty bins, both tiers and both sides of
their boundary; no lengths, ragged lengths, codes outside [0, K)), determinism, Codebook.forward against
vqhmm.quantize, the EMA and k-means updates step by step, the lookup and the dead-code reset."""
import numpy as np
import pytest
import torch

import vq_codebook_ref as R
from gpu_buffers import check_all, guarded

pytestmark = pytest.mark.gpu

# the slab fits LDS while (K*Dv + K + 1)*8 + 64*65*4 <= 156 KB: at Dv = 64 that is K <= 275
SHAPES = [(3, 5, 67, 3), (4, 16, 100, 8), (2, 64, 64, 32), (2, 64, 130, 32), (1, 1, 1, 1), (5, 7, 3, 17),
          (2, 8, 130, 70), (3, 33, 65, 200), (2, 64, 96, 1024), (2, 64, 70, 275), (2, 64, 70, 276)]
MODES = ["full", "ragged", "badidx"]


def _inputs(B, Dv, T, K, mode):
    """z, codebook, idx (the kernel's own argmin, bit-exact against the C oracle), lengths."""
    import vqhmm
    rng = np.random.default_rng(B * 1000 + Dv * 10 + K + 7 * MODES.index(mode))
    z = rng.standard_normal((B, Dv, T)).astype(np.float32)
    cb = rng.standard_normal((K, Dv)).astype(np.float32)
    idx = vqhmm.vq_argmin(torch.from_numpy(z).cuda(), torch.from_numpy(cb).cuda()).cpu().numpy()
    lengths = None
    if mode == "ragged":
        pat = [0, T, T + 5, -2, max(T // 2, 1)]
        rot = (B + K) % len(pat)
        lengths = np.array([(pat[rot:] + pat[:rot])[b % len(pat)] for b in range(B)], np.int64)
    if mode == "badidx":
        bad = rng.random((B, T)) < 0.2
        bad[0, 0] = True
        idx = np.where(bad, np.where(rng.random((B, T)) < 0.5, -1, K), idx).astype(np.int32)
    return rng, z, cb, idx, lengths


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats(z, idx, lengths, cb):
    """vqhmm_vq_stats_f32 on guarded, NaN-prefilled count / sum / sse buffers and a guarded, poisoned workspace of
    exactly the queried size (gpu_buffers.guarded) -> the three outputs concatenated."""
    from vqhmm import _ext
    lib = _ext.load()
    B, Dv, T = z.shape
    K = cb.shape[0]
    outs = [guarded((n,), torch.float64, fill=float("nan")) for n in (K, K * Dv, 1)]
    nb = lib.vqhmm_vq_stats_workspace_size(B, Dv, T, K)
    ws = guarded(nb, torch.uint8)
    _ext.check(lib.vqhmm_vq_stats_f32(_ext.ptr(z), _ext.ptr(idx), _ext.ptr(lengths), B, Dv, T, _ext.ptr(cb), K,
                                      outs[0].ptr, outs[1].ptr, outs[2].ptr, ws.ptr, nb, _ext.stream_ptr()), "stats")
    check_all(*outs, ws)
    return torch.cat([g.t for g in outs])


def _bwd(z, idx, lengths, cb, g, s, c):
    """vqhmm_vq_quantize_bwd_f32 on guarded, NaN-prefilled dz / dcodebook and a guarded, poisoned workspace."""
    from vqhmm import _ext
    lib = _ext.load()
    B, Dv, T = z.shape
    K = cb.shape[0]
    dz = guarded(z.shape, torch.float32, fill=float("nan"))
    dcb = guarded(cb.shape, torch.float32, fill=float("nan"))
    st = torch.tensor([s], dtype=torch.float32, device="cuda")
    ct = torch.tensor([c], dtype=torch.float32, device="cuda")
    nb = lib.vqhmm_vq_quantize_bwd_workspace_size(B, Dv, T, K)
    ws = guarded(nb, torch.uint8)
    _ext.check(lib.vqhmm_vq_quantize_bwd_f32(_ext.ptr(z), _ext.ptr(idx), _ext.ptr(lengths), B, Dv, T, _ext.ptr(cb), K,
                                             _ext.ptr(g), _ext.ptr(st), _ext.ptr(ct), dz.ptr, dcb.ptr,
                                             ws.ptr, nb, _ext.stream_ptr()), "bwd")
    check_all(dz, dcb, ws)
    return dz.t, dcb.t


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,Dv,T,K", SHAPES)
def test_stats_and_backward_vs_ref(B, Dv, T, K, mode):
    rng, z, cb, idx, lengths = _inputs(B, Dv, T, K, mode)
    zt, ct, it, lt = _dev(z), _dev(cb), _dev(idx), _dev(lengths)
    ref = R.stats(z, idx, lengths, cb)
    flat = _stats(zt, it, lt, ct)
    got = flat.cpu().numpy()
    count, rsum, sse = got[:K], got[K:K + K * Dv].reshape(K, Dv), got[-1]
    assert np.array_equal(count, ref["count"])
    err = np.abs(rsum - ref["rsum"])
    print(f"rsum: worst err / sum|r| = {(err / np.maximum(ref['rabs'], 1e-300)).max():.3e}, "
          f"sse rel err = {abs(sse - ref['sse']) / max(ref['sse'], 1e-300):.3e}")
    assert (err <= 1e-5 * ref["rabs"]).all()
    assert abs(sse - ref["sse"]) <= 1e-6 * ref["sse"]
    assert torch.equal(_stats(zt, it, lt, ct), flat)          # the same bits run to run (NaN-free by the above)

    g = rng.standard_normal(z.shape).astype(np.float32)
    s, c = 0.37 / z.size, -1.9 / z.size
    rdz, rdcb = R.bwd(z, idx, lengths, cb, g, s, c)
    dz, dcb = _bwd(zt, it, lt, ct, _dev(g), s, c)
    assert np.array_equal(dz.cpu().numpy(), rdz)
    assert np.abs(dcb.cpu().numpy().astype(np.float64) - rdcb).max() <= 1e-5 * max(np.abs(rdcb).max(), 1e-300)
    dz2, dcb2 = _bwd(zt, it, lt, ct, _dev(g), s, c)
    assert torch.equal(dcb2, dcb) and torch.equal(dz2, dz)
    # without g_zq the straight-through term is 0
    dz0, _ = _bwd(zt, it, lt, ct, None, s, c)
    assert np.array_equal(dz0.cpu().numpy(), R.bwd(z, idx, lengths, cb, None, s, c)[0])


@pytest.mark.parametrize("B,Dv,T,K", SHAPES)
def test_forward_matches_quantize(B, Dv, T, K):
    import vqhmm
    rng, z, cb, idx, _ = _inputs(B, Dv, T, K, "full")
    w = rng.standard_normal(z.shape).astype(np.float32)
    beta = 0.25
    mod = vqhmm.Codebook(K, Dv, beta=beta).cuda()
    with torch.no_grad():
        mod.weight.copy_(_dev(cb))
    z1 = _dev(z).requires_grad_(True)
    z2 = _dev(z).requires_grad_(True)
    c2 = _dev(cb).requires_grad_(True)
    out1 = mod(z1)
    out2 = vqhmm.quantize(z2, c2, beta=beta)
    for a, b in zip(out1, out2):
        assert a.dtype == b.dtype and torch.equal(a, b)
    wt = _dev(w)
    (out1[0] * wt).sum().add(out1[2]).add(out1[3]).backward()
    (out2[0] * wt).sum().add(out2[2]).add(out2[3]).backward()
    n = z.size
    rdz, rdcb = R.bwd(z, idx, None, cb, w, 2.0 * beta / n, -2.0 / n)
    tol_z = 1e-6 * np.abs(w).max()
    tol_c = 1e-5 * max(np.abs(rdcb).max(), 1e-12)
    dz = z1.grad.cpu().numpy().astype(np.float64)
    dc = mod.weight.grad.cpu().numpy().astype(np.float64)
    assert np.abs(dz - rdz).max() <= tol_z and np.abs(dz - z2.grad.cpu().numpy()).max() <= tol_z
    assert np.abs(dc - rdcb).max() <= tol_c and np.abs(dc - c2.grad.cpu().numpy()).max() <= tol_c


@pytest.mark.parametrize("B,Dv,T,K", [(4, 16, 100, 8), (5, 7, 3, 17), (2, 64, 130, 32)])
def test_forward_with_lengths(B, Dv, T, K):
    import vqhmm
    rng, z, cb, idx, lengths = _inputs(B, Dv, T, K, "ragged")
    w = rng.standard_normal(z.shape).astype(np.float32)
    beta = 0.5
    mod = vqhmm.Codebook(K, Dv, beta=beta).cuda()
    with torch.no_grad():
        mod.weight.copy_(_dev(cb))
    zt = _dev(z).requires_grad_(True)
    zq_st, gi, commit, cbl = mod(zt, _dev(lengths))
    full = vqhmm.quantize(_dev(z), _dev(cb), beta=beta)
    assert torch.equal(zq_st, full[0]) and torch.equal(gi, full[1])       # written everywhere
    st = R.stats(z, idx, lengths, cb)
    n = Dv * max(int(np.clip(lengths, 0, T).sum()), 1)
    assert abs(cbl.item() - st["sse"] / n) <= 1e-6 * st["sse"] / n
    assert abs(commit.item() - beta * st["sse"] / n) <= 1e-6 * beta * st["sse"] / n
    (zq_st * _dev(w)).sum().add(commit).add(cbl).backward()
    rdz, rdcb = R.bwd(z, idx, lengths, cb, w, 2.0 * beta / n, -2.0 / n)
    assert np.abs(zt.grad.cpu().numpy().astype(np.float64) - rdz).max() <= 1e-6 * np.abs(w).max()
    assert np.abs(mod.weight.grad.cpu().numpy() - rdcb).max() <= 1e-5 * max(np.abs(rdcb).max(), 1e-12)


@pytest.mark.parametrize("B,Dv,T,K,ragged", [(4, 16, 100, 8, False), (5, 7, 3, 17, True), (2, 64, 96, 1024, False)])
def test_ema_updates_vs_ref(B, Dv, T, K, ragged):
    import vqhmm
    rng, z, cb, _, lengths = _inputs(B, Dv, T, K, "ragged" if ragged else "full")
    decay, eps = 0.9, 1e-5
    mod = vqhmm.Codebook(K, Dv, decay=decay, eps=eps).cuda().train()
    mod.weight.copy_(_dev(cb))
    for step in range(3):
        zs = (z + 0.1 * step * rng.standard_normal(z.shape)).astype(np.float32)
        w0, ec0, es0 = (t.cpu().numpy().copy() for t in (mod.weight, mod.ema_count, mod.ema_sum))
        zq_st, idx, commit, cbl = mod(_dev(zs), _dev(lengths))
        assert cbl.item() == 0.0
        st = R.stats(zs, idx.cpu().numpy(), lengths, w0)
        w1, ec1, es1 = R.ema_update(w0, ec0, es0, st, decay, eps)
        assert np.abs(mod.weight.cpu().numpy() - w1).max() <= 1e-6
        assert np.abs(mod.ema_count.cpu().numpy() - ec1).max() <= 1e-12 * max(np.abs(ec1).max(), 1e-300)
        assert np.abs(mod.ema_sum.cpu().numpy() - es1).max() <= 1e-12 * max(np.abs(es1).max(), 1e-300)
    # evaluation mode leaves the state alone
    before = [t.clone() for t in (mod.weight, mod.ema_count, mod.ema_sum)]
    mod.eval()(_dev(z))
    assert all(torch.equal(a, b) for a, b in zip(before, (mod.weight, mod.ema_count, mod.ema_sum)))
    p = float(vqhmm.Codebook.perplexity(mod.ema_count))
    assert abs(p - R.perplexity(mod.ema_count.cpu().numpy())) <= 1e-9 * p


def kmeans_inputs(B, Dv, T, K):
    rng = np.random.default_rng(B * 1000 + Dv * 10 + K)
    cent = 3.0 * rng.standard_normal((K, Dv))
    lab = rng.integers(0, K, (B, T))
    z = (cent[lab].transpose(0, 2, 1) + 0.3 * rng.standard_normal((B, Dv, T))).astype(np.float32)
    pos = rng.permutation(B * T)[:K]
    weight = np.ascontiguousarray(z.transpose(0, 2, 1).reshape(-1, Dv)[pos])
    return z, weight


@pytest.mark.parametrize("B,Dv,T,K", SHAPES[:4])
def test_kmeans_step_by_step(B, Dv, T, K):
    import vqhmm
    z, weight = kmeans_inputs(B, Dv, T, K)
    zt = _dev(z)
    mod = vqhmm.Codebook(K, Dv).cuda()
    whole = vqhmm.Codebook(K, Dv).cuda()
    with torch.no_grad():
        mod.weight.copy_(_dev(weight))
        whole.weight.copy_(_dev(weight))
    hist = []
    for it in range(8):
        w0 = mod.weight.detach().cpu().numpy().copy()
        idx = vqhmm.vq_argmin(zt, mod.weight.detach()).cpu().numpy()
        st = R.stats(z, idx, None, w0)
        assert (st["count"] > 0).all(), (it, st["count"])
        h = mod.fit_kmeans(zt, n_iter=1, init=False)
        assert len(h) == 1 and h[0].dim() == 0 and h[0].is_cuda
        hist.append(float(h[0]))
        assert abs(hist[-1] - st["sse"] / (Dv * B * T)) <= 1e-6 * st["sse"] / (Dv * B * T)
        assert np.abs(mod.weight.detach().cpu().numpy() - R.kmeans_step(w0, st)).max() <= 1e-6
    print("distortion history:", hist)
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1.0 + 1e-6)
    # one call of 8 iterations is the same deterministic trajectory
    h8 = whole.fit_kmeans(zt, n_iter=8, init=False)
    assert [float(h) for h in h8] == hist
    assert torch.equal(whole.weight, mod.weight)


def test_fit_kmeans_init_seeds_from_counted_positions():
    import vqhmm
    B, Dv, T, K = 4, 16, 100, 8
    z, _ = kmeans_inputs(B, Dv, T, K)
    lengths = np.array([0, T, 40, -2], np.int64)
    mod = vqhmm.Codebook(K, Dv).cuda()
    g = torch.Generator(device="cuda").manual_seed(5)
    hist = mod.fit_kmeans(_dev(z), _dev(lengths), n_iter=0, generator=g)
    assert hist == []
    rows = {z[b, :, t].tobytes() for b in range(B) for t in range(min(max(int(lengths[b]), 0), T))}
    seeded = [r.tobytes() for r in mod.weight.detach().cpu().numpy()]
    assert all(r in rows for r in seeded) and len(set(seeded)) == K
    hist = mod.fit_kmeans(_dev(z), _dev(lengths), n_iter=3, init=False)
    assert len(hist) == 3 and float(hist[2]) <= float(hist[0])


@pytest.mark.parametrize("B,Dv,T,K", [(3, 5, 67, 3), (2, 64, 130, 32), (5, 7, 3, 17), (2, 64, 96, 1024)])
def test_lookup(B, Dv, T, K):
    import vqhmm
    rng, z, cb, idx, _ = _inputs(B, Dv, T, K, "badidx")
    mod = vqhmm.Codebook(K, Dv).cuda()
    with torch.no_grad():
        mod.weight.copy_(_dev(cb))
    assert (idx == -1).any()
    ref = R.lookup(cb, idx)
    for dtype in (torch.int32, torch.int64):
        out = mod.lookup(_dev(idx).to(dtype))
        assert out.shape == (B, Dv, T) and out.dtype == torch.float32 and not out.requires_grad
        assert np.array_equal(out.cpu().numpy(), ref)


def test_lookup_of_codehmm_samples():
    import vqhmm
    K, Dv, n, L = 12, 6, 5, 9
    hmm = vqhmm.CodeHMM(3, K, generator=torch.Generator().manual_seed(0)).cuda()
    mod = vqhmm.Codebook(K, Dv, generator=torch.Generator().manual_seed(1)).cuda()
    codes = hmm.sample(n, L, generator=torch.Generator(device="cuda").manual_seed(2))[1]
    out = mod.lookup(codes)
    assert out.shape == (n, Dv, L)
    assert np.array_equal(out.cpu().numpy(), R.lookup(mod.weight.detach().cpu().numpy(), codes.cpu().numpy()))
    path, _ = hmm.decode(codes, torch.tensor([L, 3, 0, L, 1]))           # -1 padded
    assert mod.lookup(path).shape == (n, Dv, L)


@pytest.mark.parametrize("ema", [False, True])
def test_reset_dead_codes(ema):
    import vqhmm
    B, Dv, T, K = 4, 16, 100, 8
    z, weight = kmeans_inputs(B, Dv, T, K)
    lengths = np.array([T, 0, 37, T + 5], np.int64)
    mod = vqhmm.Codebook(K, Dv, decay=0.9 if ema else None).cuda()
    dead = [1, 6]
    with torch.no_grad():
        mod.weight.copy_(_dev(weight))
        if ema:
            mod.ema_count.copy_(torch.tensor([5.0, 0.2, 3.0, 1.0, 9.0, 2.0, 0.0, 1.5], dtype=torch.float64))
        else:
            mod.weight[dead] = 1e3                                         # no position chooses these rows
    w0 = mod.weight.detach().cpu().numpy().copy()
    n = mod.reset_dead_codes(_dev(z), _dev(lengths), generator=torch.Generator(device="cuda").manual_seed(3))
    w1 = mod.weight.detach().cpu().numpy()
    assert n == len(dead)
    rows = {z[b, :, t].tobytes() for b in range(B) for t in range(min(max(int(lengths[b]), 0), T))}
    for k in range(K):
        if k in dead:
            assert w1[k].tobytes() in rows
        else:
            assert np.array_equal(w1[k], w0[k])
    assert mod.reset_dead_codes(_dev(z), _dev(lengths)) == 0                 # nothing is dead any more
