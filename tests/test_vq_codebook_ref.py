"""CPU checks of codebook learning: the fp64 helper (tests/vq_codebook_ref.py) against brute-force loops and
against the pinned quantizer restatement (oracle/hmm_ref.quantize_f32 on the C oracle's indices), the update
rules' identities, the C-ABI's host-side behaviour and the Python surface.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import vq_codebook_ref as R
from conftest import ROOT

NEW_SYMBOLS = ("vqhmm_vq_stats_workspace_size", "vqhmm_vq_stats_f32", "vqhmm_vq_quantize_bwd_workspace_size",
               "vqhmm_vq_quantize_bwd_f32", "vqhmm_vq_lookup_f32")


def _case(B, Dv, T, K, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, Dv, T)).astype(np.float32)
    cb = rng.standard_normal((K, Dv)).astype(np.float32)
    idx = rng.integers(0, K, (B, T)).astype(np.int32)
    return rng, z, cb, idx


@pytest.mark.parametrize("B,Dv,T,K", [(3, 5, 9, 4), (2, 1, 7, 1), (4, 3, 5, 11)])
@pytest.mark.parametrize("ragged", [False, True])
def test_stats_match_brute_force(B, Dv, T, K, ragged):
    rng, z, cb, idx = _case(B, Dv, T, K, B * 100 + K)
    lengths = None
    if ragged:
        lengths = np.array(([0, T, T + 5, -2] * B)[:B], np.int64)
        idx[0, 0], idx[-1, -1] = -1, K
    st = R.stats(z, idx, lengths, cb)
    count = np.zeros(K)
    rsum = np.zeros((K, Dv))
    zsum = np.zeros((K, Dv))
    sse = 0.0
    for b in range(B):
        L = T if lengths is None else min(max(int(lengths[b]), 0), T)
        for t in range(L):
            k = int(idx[b, t])
            if not 0 <= k < K:
                continue
            count[k] += 1
            for d in range(Dv):
                r = float(np.float32(z[b, d, t] - cb[k, d]))
                rsum[k, d] += r
                zsum[k, d] += float(z[b, d, t])
                sse += r * r
    assert np.array_equal(st["count"], count)
    assert np.allclose(st["rsum"], rsum, rtol=0, atol=1e-12)
    assert abs(st["sse"] - sse) <= 1e-12 * max(sse, 1.0)
    # the plain sum comes back out of the residual form (up to the fp32 rounding of each residual)
    assert np.allclose(st["rsum"] + st["count"][:, None] * cb.astype(np.float64), zsum, rtol=0,
                       atol=2.0 ** -23 * 8 * max(B * T, 1))
    # the backward's dz is 0-residual off the counted set, and its dcodebook is the scaled rsum
    g = rng.standard_normal((B, Dv, T)).astype(np.float32)
    dz, dcb = R.bwd(z, idx, lengths, cb, g, 0.37, -1.5)
    off = ~R.counted(idx, lengths, K)
    assert np.array_equal(dz[off.nonzero()[0], :, off.nonzero()[1]], g[off.nonzero()[0], :, off.nonzero()[1]])
    assert np.allclose(dcb, -1.5 * rsum, rtol=0, atol=1e-12)


@pytest.mark.parametrize("B,Dv,T,K,beta", [(3, 16, 50, 8, 0.25), (2, 5, 33, 3, 1.0), (2, 8, 40, 70, 0.5)])
def test_bwd_matches_the_pinned_quantizer_restatement(B, Dv, T, K, beta):
    from oracle import c_oracle, hmm_ref
    rng, z, cb, _ = _case(B, Dv, T, K, 7 + K)
    w = rng.standard_normal(z.shape).astype(np.float32)
    ridx = c_oracle.vq_argmin(z, cb, want_dmin=False)
    ref = hmm_ref.quantize_f32(z, cb, ridx, beta)
    n = z.size
    dz, dcb = R.bwd(z, ridx, None, cb, w, 2.0 * beta / n, -2.0 / n)
    assert np.abs(dz.astype(np.float64) - (w + ref["dz_extra"])).max() <= 1e-6 * np.abs(w).max()
    assert np.abs(dcb - ref["dcodebook"]).max() <= 1e-5 * max(np.abs(ref["dcodebook"]).max(), 1e-12)
    st = R.stats(z, ridx, None, cb)
    assert abs(st["sse"] / n - ref["codebook"]) <= 1e-6 * ref["codebook"]


def test_updates_and_readouts():
    rng, z, cb, idx = _case(4, 6, 20, 5, 3)
    idx[idx == 4] = 0                                  # code 4 stays empty
    st = R.stats(z, idx, None, cb)
    mean = np.stack([z.transpose(0, 2, 1)[idx == k].astype(np.float64).mean(axis=0) if (idx == k).any()
                     else cb[k].astype(np.float64) for k in range(5)])
    km = R.kmeans_step(cb, st)
    assert np.allclose(km, mean, rtol=0, atol=1e-6)
    assert np.array_equal(km[4], cb[4])
    # decay 0 and eps 0: the EMA is the batch mean, from any previous state
    w, ec, es = R.ema_update(cb, rng.random(5), rng.standard_normal((5, 6)), st, 0.0, 0.0)
    assert np.allclose(w, mean, rtol=0, atol=1e-6)
    assert np.array_equal(w[4], cb[4])
    assert np.array_equal(ec, st["count"])
    # with a decay the buffers are the convex combination
    w2, ec2, es2 = R.ema_update(w, ec, es, st, 0.9, 1e-5)
    assert np.allclose(ec2, 0.9 * ec + 0.1 * st["count"])
    assert R.perplexity(np.full(7, 3.0)) == pytest.approx(7.0, rel=1e-12)
    assert R.perplexity(np.array([0.0, 5.0, 0.0])) == pytest.approx(1.0, rel=1e-12)
    lk = R.lookup(cb, np.array([[0, -1, 4], [5, 2, 1]]))
    assert lk.shape == (2, 6, 3)
    assert np.array_equal(lk[0, :, 0], cb[0]) and np.array_equal(lk[1, :, 1], cb[2])
    assert not lk[0, :, 1].any() and not lk[1, :, 0].any()


# --------------------------------------------------------------------------- C ABI
def test_new_symbols_declared_exported_and_bound():
    from vqhmm import _ext
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vqhmm.h")).read(), flags=re.S)
    lib = _ext.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _ext.exported_symbols(), name
    assert lib.vqhmm_abi_version() == 8


def _entry_points(lib, p):
    """name -> (function, argument list for B=2, Dv=3, T=4, K=5 with every pointer set, required pointer slots,
    slots of Dv and K, slots of B and T, workspace-size slot or None)."""
    return {
        "stats": (lib.vqhmm_vq_stats_f32, [p, p, p, 2, 3, 4, p, 5, p, p, p, p, 1 << 20, None],
                  (0, 1, 6, 8, 9), (4, 7), (3, 5), 12),
        "bwd": (lib.vqhmm_vq_quantize_bwd_f32, [p, p, p, 2, 3, 4, p, 5, p, p, p, p, p, p, 1 << 20, None],
                (0, 1, 6, 9, 10), (4, 7), (3, 5), 14),
        "lookup": (lib.vqhmm_vq_lookup_f32, [p, 5, 3, p, 2, 4, p, None], (0, 3, 6), (2, 1), (4, 5), None),
    }


@pytest.mark.parametrize("which", ["stats", "bwd", "lookup"])
def test_host_side_checks_without_gpu(which):
    from vqhmm import _ext
    lib = _ext.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fn, full, required, (iDv, iK), (iB, iT), iws = _entry_points(lib, p)[which]
    for hole in required:
        args = list(full)
        args[hole] = None
        assert fn(*args) == -1, hole
    # a negative size comes first, then the unsupported sizes, before any pointer is looked at
    for slot in (iB, iT, iDv, iK):
        args = [None if a is p else a for a in full]
        args[slot] = -1
        assert fn(*args) == -1, slot
    for Dv, K in ((3, 65537), (513, 5), (512, 4097), (0, 5), (3, 0)):
        args = [None if a is p else a for a in full]
        args[iDv], args[iK] = Dv, K
        assert fn(*args) == -4, (Dv, K)
    # B*T == 0: nothing to do, whatever the pointers
    for B, T in ((0, 4), (2, 0), (0, 0)):
        args = [None if a is p else a for a in full]
        args[iB], args[iT] = B, T
        if iws is not None:
            args[iws] = 0
        assert fn(*args) == 0, (B, T)
    if iws is not None:
        query = lib.vqhmm_vq_stats_workspace_size if which == "stats" else lib.vqhmm_vq_quantize_bwd_workspace_size
        need = query(2, 3, 4, 5)
        assert need > 0
        args = list(full)
        args[iws] = need - 1
        assert fn(*args) == -3
        args[iws - 1] = None
        assert fn(*args) == -3


def test_workspace_query_limits():
    from vqhmm import _ext
    lib = _ext.load()
    for query in (lib.vqhmm_vq_stats_workspace_size, lib.vqhmm_vq_quantize_bwd_workspace_size):
        assert query(4, 64, 100, 256) > 0
        assert query(4, 32, 100, 65536) > 0
        assert query(4, 512, 100, 4096) > 0
        assert query(4, 3, 100, 65537) == 0
        assert query(4, 513, 100, 8) == 0
        assert query(4, 512, 100, 4097) == 0
        assert query(4, 0, 100, 8) == 0
        assert query(4, 8, 100, 0) == 0
        assert query(-1, 8, 100, 8) == 0
        # one partial at least, and the partials stay under the cap unless a single one is larger
        assert query(1, 8, 1, 8) >= (8 * 8 + 8 + 1) * 8
        assert query(1 << 20, 64, 200, 1024) <= 64 << 20


# --------------------------------------------------------------------------- module
def test_python_surface_and_cpu_refusal():
    import torch
    import vqhmm
    assert "Codebook" in vqhmm.__all__
    for m in ("forward", "stats", "kmeans_step", "ema_update", "fit_kmeans", "reset_dead_codes", "lookup",
              "perplexity"):
        assert callable(getattr(vqhmm.Codebook, m))
    cb = vqhmm.Codebook(7, 5, generator=torch.Generator().manual_seed(1))
    assert isinstance(cb.weight, torch.nn.Parameter) and cb.weight.shape == (7, 5) and cb.weight.dtype == torch.float32
    assert set(cb.state_dict()) == {"weight"}
    ema = vqhmm.Codebook(7, 5, decay=0.99, generator=torch.Generator().manual_seed(2))
    assert not isinstance(ema.weight, torch.nn.Parameter) and not list(ema.parameters())
    assert set(ema.state_dict()) == {"weight", "ema_count", "ema_sum"}
    assert ema.ema_count.dtype == torch.float64 and ema.ema_count.shape == (7,)
    assert ema.ema_sum.dtype == torch.float64 and ema.ema_sum.shape == (7, 5)
    assert not torch.equal(ema.weight, cb.weight.detach())
    other = vqhmm.Codebook(7, 5, decay=0.5)
    other.load_state_dict(ema.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), ema.state_dict().values()))
    z = torch.zeros(2, 5, 4)
    codes = torch.zeros(2, 4, dtype=torch.int64)
    for call in (lambda: cb(z), lambda: cb.stats(z), lambda: cb.stats(z, codes), lambda: cb.fit_kmeans(z, n_iter=1),
                 lambda: cb.reset_dead_codes(z), lambda: cb.lookup(codes), lambda: ema(z)):
        with pytest.raises(RuntimeError, match="HIP"):
            call()
    for bad in ((0, 5), (65537, 5), (7, 0), (7, 513), (4097, 512)):
        with pytest.raises(ValueError):
            vqhmm.Codebook(*bad)
    for decay in (1.0, -0.1):
        with pytest.raises(ValueError):
            vqhmm.Codebook(7, 5, decay=decay)
    with pytest.raises(RuntimeError):
        cb.ema_update({"count": torch.zeros(7, dtype=torch.float64), "rsum": torch.zeros(7, 5, dtype=torch.float64)})
    # the read-out is plain torch and agrees with the helper
    cnt = torch.tensor([3.0, 0.0, 1.0, 4.0], dtype=torch.float64)
    assert float(vqhmm.Codebook.perplexity(cnt)) == pytest.approx(R.perplexity(cnt.numpy()), rel=1e-12)
    assert float(vqhmm.Codebook.perplexity(torch.full((9,), 2.0))) == pytest.approx(9.0, rel=1e-12)
