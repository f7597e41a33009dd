"""The kernel variants that vq_argmin / quantize, viterbi, forward_backward and the samplers pick on the
host from facts no other test varies: a log_A, em or z that is not 16-byte aligned, Dv > 64, K > 70 on
the VALU kernel, B * T * Dv at 2^30, non-finite z, and -inf tables in the K <= 32 Viterbi kernels.

Inputs only are misaligned (gpu_buffers.offset_view: 4 bytes past a 16-byte boundary); outputs and
workspaces are the fresh allocations the Python API makes.  No new reference and no new tolerance:
indices, paths, scores, dmin and z_q_st are compared bit for bit with oracle/c_oracle.py (and with
the same call on aligned copies), gamma / logZ by test_gpu_hmm.py's check_gamma and its logZ rule
against oracle.hmm_ref.forward_backward_f64, the losses of quantize by test_gpu_vq.py's 1e-6 relative,
the samplers' paths exactly against tests/sample_ref.py.  Where the oracle's dmin is NaN the NaN masks
are compared, not the payload bits.
"""
import functools
import time

import numpy as np
import pytest
import torch

import sample_ref as SR
from gpu_buffers import offset_view
from oracle import c_oracle, hmm_ref
from test_gpu_hmm import FB_KERNELS, check_gamma, gpu, random_hmm, use_fb_kernel
from test_gpu_sample import raw_sample

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(t):
    return t.detach().cpu().numpy()


def check_logZ(z, rz, L):
    """test_gpu_hmm.py's logZ rule: rel 1e-5 of max(1, |ref|) inside the batch, NaN for length 0."""
    live = np.asarray(L) > 0
    assert np.all(np.abs(z[live] - rz[live]) <= 1e-5 * np.maximum(1.0, np.abs(rz[live])))
    assert np.all(np.isnan(z[~live]))


def check_posteriors(gamma, logZ, ref, L, T):
    g, z = host(gamma), host(logZ)
    check_gamma(g, ref[0])
    check_logZ(z, ref[1], L)
    past = np.arange(T)[None, :] >= np.asarray(L)[:, None]
    assert np.all(g[past] == 0)


# ------------------------------------------------------------------ 1. HMM kernels on misaligned tables
# lengths around both chunk sizes of hmm.hip's staging ring (16 steps for a misaligned K = 4 / 8 table,
# 32 for an aligned one): the CHECK path, Lmin / Lmax and the mask flush all move with the chunk size
T_RAG = 70
L_RAG = (T_RAG, 0, 1, 15, 16, 17, 31, 32, 33)
# the same pattern around the 64-step segments of hmm_seg.hip
T_SEG = 200
L_SEG = (T_SEG, 0, 1, 63, 64, 65, 127, 128, 129)
K_SMALL = [3, 4, 8]        # hmm.hip
K_WIDE = [12, 16, 17, 32]  # hmm_wide.hip


@functools.lru_cache(maxsize=None)
def hmm_case(K, T, lengths):
    """Tables and both references, computed once per process and shared; callers must not modify them."""
    L = np.array(lengths, np.int64)
    log_pi, log_A, em = random_hmm(K * 17 + T, len(L), T, K)
    return dict(log_pi=log_pi, log_A=log_A, em=em, L=L, vit=c_oracle.viterbi(log_pi, log_A, em, L),
                fb=hmm_ref.forward_backward_f64(log_pi, log_A, em, L))


def tables(c, offset):
    arrs = (c["log_pi"], c["log_A"], c["em"])
    return [offset_view(a) for a in arrs] if offset else gpu(*arrs)


@pytest.mark.parametrize("K", K_SMALL + K_WIDE)
def test_viterbi_misaligned_tables(K):
    """viterbi_kernel<K, false> (K = 4, 8: 16-step chunks instead of 32) and the wide kernel through
    4-byte aligned log_pi, log_A and em: the oracle's bits, and the aligned call's."""
    import vqhmm
    c = hmm_case(K, T_RAG, L_RAG)
    L = torch.from_numpy(c["L"])
    pm, sm = vqhmm.viterbi(*tables(c, True), L)
    pa, sa = vqhmm.viterbi(*tables(c, False), L)
    rp, rs = c["vit"]
    assert np.array_equal(host(pm), rp)
    assert np.array_equal(bits(host(sm)), bits(rs))
    assert torch.equal(pm, pa) and np.array_equal(bits(host(sm)), bits(host(sa)))


@pytest.mark.parametrize("K,kernel", [(K, k) for K in K_SMALL for k in FB_KERNELS] + [(K, None) for K in K_WIDE])
def test_forward_backward_misaligned_tables(K, kernel, monkeypatch):
    """Every K <= 8 kernel (the three streaming forms run fwdbwd_kernel<K, false, ..>) and the wide
    kernel's V4 = false loads at K % 4 == 0, on misaligned tables."""
    import vqhmm
    if kernel is not None:
        use_fb_kernel(monkeypatch, kernel)
    c = hmm_case(K, T_RAG, L_RAG)
    gamma, logZ = vqhmm.forward_backward(*tables(c, True), torch.from_numpy(c["L"]))
    check_posteriors(gamma, logZ, c["fb"], c["L"], T_RAG)


def test_forward_backward_default_choice_misaligned():
    """No switch set at K = 8, T = 200: the default choice (the parallel-in-time kernel, whose table
    loads are 4-byte buffer loads) on a misaligned table, lengths around its 64-step segments."""
    import vqhmm
    c = hmm_case(8, T_SEG, L_SEG)
    gamma, logZ = vqhmm.forward_backward(*tables(c, True), torch.from_numpy(c["L"]))
    check_posteriors(gamma, logZ, c["fb"], c["L"], T_SEG)


@pytest.mark.parametrize("fuse", [None, "0"])
def test_forward_backward_long_misaligned(fuse, monkeypatch):
    """K = 8, T = 1100: past the parallel-in-time kernel's 1024 steps and the resident kernel's LDS, so
    the streaming kernel runs.  An aligned table of this length is past the fused form's LDS limit too;
    the misaligned form's 16-step chunks keep a smaller ring, and it still fuses (fuse = None), so the
    second case switches the fusion off: fwdbwd_kernel<8, false, false> with its workspace and gamma
    pass."""
    import vqhmm
    if fuse is not None:
        monkeypatch.setenv("VQHMM_FB_FUSE", fuse)
    T = 1100
    c = hmm_case(8, T, (1100, 1000, 513))
    gamma, logZ = vqhmm.forward_backward(*tables(c, True), torch.from_numpy(c["L"]))
    check_posteriors(gamma, logZ, c["fb"], c["L"], T)


def test_prior_viterbi_misaligned_inputs():
    """The fused Prior -> Viterbi kernel with u and em 4 bytes off: bit-identical to vqhmm.viterbi on
    Prior.forward's tables (and to the C oracle on them, and to the aligned fused call)."""
    import vqhmm
    K, U, TH, B, T = 8, 4, 128, len(L_RAG), T_RAG
    torch.manual_seed(1000 * K + TH + U)
    prior = vqhmm.Prior(K, u_dim=U, trans_hidden=TH)
    with torch.no_grad():  # sharper tables than the default init: paths that actually switch
        prior.transition_net[2].weight.mul_(4.0)
        prior.log_prior.normal_()
    prior = prior.cuda()
    u = (2.0 * torch.randn(B, U, T)).cuda()
    em = torch.log_softmax(3.0 * torch.randn(B, T, K), dim=2).cuda()
    L = torch.tensor(L_RAG)
    got = vqhmm.prior_viterbi(prior, offset_view(u), offset_view(em), L)
    assert got is not None
    with torch.no_grad():
        log_pi, log_A = prior(u)
    ref = vqhmm.viterbi(log_pi, log_A, em, L)
    assert torch.equal(got[0], ref[0]) and np.array_equal(bits(host(got[1])), bits(host(ref[1])))
    rp, rs = c_oracle.viterbi(host(log_pi), host(log_A), host(em), L.numpy())
    assert np.array_equal(host(got[0]), rp) and np.array_equal(bits(host(got[1])), bits(rs))
    al = vqhmm.prior_viterbi(prior, u, em, L)
    assert torch.equal(got[0], al[0]) and np.array_equal(bits(host(got[1])), bits(host(al[1])))
    assert len(np.unique(rp[rp >= 0])) > 1


# ------------------------------------------------------------------ 2. structural zeros in Viterbi, K <= 32
@functools.lru_cache(maxsize=None)
def zeros_case(K):
    """b0 left-to-right log_A (test_forward_backward_extreme_tables' construction), b1 an impossible
    sequence (every emission -inf at T // 3), b2 and b3 ordinary (b3 of length T - 7).  log_pi is one
    vector for the whole batch, so "a log_pi with a single finite entry" is a second launch on the same
    tables: there every sequence starts from the one state K // 2 (and b0 can never leave the states
    above it).  Oracle answers for both launches; shared, read-only."""
    B, T = 4, 70
    log_pi, log_A, em = random_hmm(K + 300, B, T, K)
    log_A = log_A.astype(np.float64)
    tri = np.triu(np.ones((K, K), bool))
    la = np.where(tri, log_A[0], -np.inf)
    log_A[0] = la - np.logaddexp.reduce(la, axis=-1, keepdims=True)
    log_A = log_A.astype(np.float32)
    em = em.copy()
    em[1, T // 3, :] = -np.inf
    L = np.array([T, T, T, T - 7], np.int64)
    single = np.full(K, -np.inf, np.float32)
    single[K // 2] = 0.0
    out = []
    for lp in (log_pi, single):
        rp, rs = c_oracle.viterbi(lp, log_A, em, L)
        out.append(dict(log_pi=lp, log_A=log_A, em=em, L=L, vit=(rp, rs)))
    rp, rs = out[0]["vit"]
    assert rs[1] == -np.inf and np.all(rp[1, T // 3:] == 0) and np.all(np.isfinite(rs[[0, 2, 3]]))
    assert out[1]["vit"][1][1] == -np.inf and np.all(np.isfinite(out[1]["vit"][1][[0, 2, 3]]))
    return out


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("K", [3, 4, 8, 16, 17, 32])
def test_viterbi_structural_zeros(K, offset):
    """-inf tables in the K <= 8 kernel (back-pointers as ballot(v == m): -inf == -inf in every lane,
    the padded ones included) and the wide kernel's own arg-max: path and score bits of the C oracle."""
    import vqhmm
    for c in zeros_case(K):
        path, score = vqhmm.viterbi(*tables(c, offset), torch.from_numpy(c["L"]))
        rp, rs = c["vit"]
        assert np.array_equal(host(path), rp)
        assert np.array_equal(bits(host(score)), bits(rs))


# ------------------------------------------------------------------ VQ
def vq_run(z, cb, offset_z=False, offset_cb=False):
    import vqhmm
    zt = offset_view(z) if offset_z else torch.from_numpy(z).cuda()
    ct = offset_view(cb) if offset_cb else torch.from_numpy(cb).cuda()
    idx, d = vqhmm.vq_argmin(zt, ct, return_dist=True)
    return host(idx), host(d)


@functools.lru_cache(maxsize=None)
def vq_case(B, Dv, T, K):
    rng = np.random.default_rng(B * 1000 + Dv * 10 + K + 7)
    z = rng.standard_normal((B, Dv, T)).astype(np.float32)
    cb = rng.standard_normal((K, Dv)).astype(np.float32)
    return z, cb, c_oracle.vq_argmin(z, cb)


# T % 4 == 0 and Dv in {4, 8, 16, 32, 64}: the row-load kernel's shapes
ROW_SHAPES = [(3, 4, 64, 3), (2, 8, 100, 8), (2, 16, 36, 16), (2, 32, 96, 17), (2, 64, 200, 32)]


@pytest.mark.parametrize("offset_cb", [False, True])
@pytest.mark.parametrize("B,Dv,T,K", ROW_SHAPES)
def test_vq_tile32_on_misaligned_z(B, Dv, T, K, offset_cb):
    """3. A misaligned z at the row-load kernel's shapes runs vq_mfma_kernel<Dv / 2> instead, and
    quantize the argmin-plus-gather route instead of the fused epilogue."""
    import vqhmm
    z, cb, (ridx, rd) = vq_case(B, Dv, T, K)
    idx, d = vq_run(z, cb, True, offset_cb)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(d), bits(rd))
    aidx, ad = vq_run(z, cb)
    assert np.array_equal(idx, aidx) and np.array_equal(bits(d), bits(ad))

    beta = 0.25
    ref = hmm_ref.quantize_f32(z, cb, ridx, beta)
    ct = offset_view(cb) if offset_cb else torch.from_numpy(cb).cuda()
    out = {}
    for name, zt in (("off", offset_view(z)), ("al", torch.from_numpy(z).cuda())):
        zq_st, qidx, commit, cb_loss = vqhmm.quantize(zt, ct, beta=beta)
        assert zq_st.data_ptr() % 16 == 0
        out[name] = (host(zq_st), host(qidx), commit.item(), cb_loss.item())
        assert np.array_equal(out[name][1], ridx)
        assert np.array_equal(bits(out[name][0]), bits(ref["z_q_st"]))
        print(name, "commit rel", abs(out[name][2] - ref["commit"]) / ref["commit"],
              "codebook rel", abs(out[name][3] - ref["codebook"]) / ref["codebook"])
        assert abs(out[name][2] - ref["commit"]) <= 1e-6 * ref["commit"]
        assert abs(out[name][3] - ref["codebook"]) <= 1e-6 * ref["codebook"]
    assert np.array_equal(bits(out["off"][0]), bits(out["al"][0])) and np.array_equal(out["off"][1], out["al"][1])


# what each shape reaches in vq_argmin_kernel<KB> (KB codes per LDS block, ldc = Dv rounded up to 16)
VALU_SHAPES = [(2, 65, 37, 3),       # KB = 4, ldc padding
               (1, 100, 70, 8),      # KB = 8
               (2, 128, 64, 16),     # KB = 16, T % 4 == 0
               (1, 512, 40, 32),     # KB = 32: exactly 64 KiB of dynamic LDS beside the static cns[]
               (1, 513, 33, 32),     # 32 * 528 * 4 > 64 KiB: halved to KB = 16
               (1, 2048, 20, 33),    # KB = 8, five code blocks, the last of one code
               (1, 8, 300, 1000),    # KB = 32, 32 blocks, the last of 8 codes
               (3, 64, 171, 257)]    # N = 513: a second workgroup with one live position


@pytest.mark.parametrize("B,Dv,T,K", VALU_SHAPES)
def test_vq_valu_kernel(B, Dv, T, K):
    """4. Dv > 64 or K > 32: idx and dmin bit-exact against the C oracle."""
    z, cb, (ridx, rd) = vq_case(B, Dv, T, K)
    idx, d = vq_run(z, cb)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(d), bits(rd))


def test_vq_valu_kernel_duplicates_across_blocks():
    """cb[40] = cb[7] (code blocks 1 and 0 of KB = 32): z exactly on cb[40] must give 7, the lowest
    index across blocks; z on cb[69] (block 2) gives 69."""
    B, Dv, T, K = 2, 100, 50, 70
    rng = np.random.default_rng(41)
    cb = rng.standard_normal((K, Dv)).astype(np.float32)
    cb[40] = cb[7]
    z = rng.standard_normal((B, Dv, T)).astype(np.float32)
    z[:, :, 0::5] = cb[40][None, :, None]
    z[:, :, 2::5] = cb[69][None, :, None]
    idx, d = vq_run(z, cb)
    ridx, rd = c_oracle.vq_argmin(z, cb)
    assert np.all(ridx[:, 0::5] == 7) and np.all(ridx[:, 2::5] == 69)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(d), bits(rd))


def test_vq_dv_over_2048_is_refused_before_any_launch():
    import vqhmm
    from vqhmm import _ext
    B, Dv, T, K = 1, 2049, 4, 2
    z = torch.zeros(B, Dv, T, device="cuda")
    cb = torch.zeros(K, Dv, device="cuda")
    idx = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    dmin = torch.full((B, T), -7.0, device="cuda")
    rc = _ext.load().vqhmm_vq_argmin_f32(_ext.ptr(z), B, Dv, T, _ext.ptr(cb), K, _ext.ptr(idx), _ext.ptr(dmin),
                                         _ext.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1  # VQHMM_EINVAL
    assert (idx == -7).all() and (dmin == -7.0).all()
    with pytest.raises(RuntimeError, match="invalid argument"):
        vqhmm.vq_argmin(z, cb)
    with pytest.raises(RuntimeError, match="invalid argument"):
        vqhmm.quantize(z, cb)


def test_vq_row_load_offset_limit():
    """5. The row-load kernel addresses z by 32-bit byte offsets and is used below 2^30 elements.
    Dv = 64, T = 200, K = 32: the first B = 83886 sequences of one allocation are 1 073 740 800
    elements (byte offsets to just under 2^32: the row-load kernel), all B = 83887 are over the limit
    (the tile-32 kernel).  The one allocation of 4.3 GB serves both launches (the smaller is its
    prefix, at the same pointer), so both see the same data.  idx bit-exact against the C oracle on
    three 32-sequence slices of each launch: the first, the one straddling byte offset 2^31
    (2^31 / 51200 = 41943.04) and the last; and the launches agree on all their common sequences.
    The one large test of the module; it prints its wall time."""
    import vqhmm
    t_start = time.perf_counter()
    Dv, T, K = 64, 200, 32
    B0, B1 = 83886, 83887
    assert B0 * T * Dv < 2 ** 30 <= B1 * T * Dv and 41927 * Dv * T * 4 < 2 ** 31 < 41959 * Dv * T * 4
    g = torch.Generator(device="cuda").manual_seed(2030)
    cb = torch.randn(K, Dv, device="cuda", generator=g)
    z = torch.randn(B1, Dv, T, device="cuda", generator=g)
    assert z.data_ptr() % 16 == 0
    cbh = host(cb)
    out = {}
    for B in (B0, B1):
        idx = vqhmm.vq_argmin(z[:B], cb)
        for lo in (0, 41927, B - 32):
            ref = c_oracle.vq_argmin(host(z[lo:lo + 32]), cbh, want_dmin=False)
            assert np.array_equal(host(idx[lo:lo + 32]), ref), (B, lo)
        out[B] = idx
    assert torch.equal(out[B0], out[B1][:B0])
    del z, out
    torch.cuda.empty_cache()
    print(f"test_vq_row_load_offset_limit: wall time {time.perf_counter() - t_start:.2f} s")


NONFINITE_SHAPES = ([(s, off) for s in ROW_SHAPES for off in (False, True)]
                    + [((2, 5, 40, 3), False), ((2, 33, 37, 5), False), ((2, 100, 40, 8), False)])


@pytest.mark.parametrize("shape,offset", NONFINITE_SHAPES)
def test_vq_nonfinite_z(shape, offset):
    """6. The contract is the C oracle's: the strict < scan and the fmaf chain over the real dims
    only.  +inf in dim 0, +inf and -inf in dim Dv - 1 (for an odd Dv the element the tile-32 kernel
    also loads into its padded dim slot), a NaN and an all-NaN column, each at its own position, two
    of them in the launch's last positions.  A random normal codebook has no zero, so the oracle's own
    scores there are +-inf (or NaN where the chain itself gives one), never 0 * inf."""
    B, Dv, T, K = shape
    z, cb, _ = vq_case(B, Dv, T, K)
    assert np.all(cb != 0)
    z = z.copy()
    z[0, 0, 1] = np.inf
    z[0, Dv - 1, 2] = np.inf
    z[1, Dv - 1, 3] = -np.inf
    z[0, Dv // 2, 5] = np.nan
    z[1, :, 7] = np.nan
    z[B - 1, Dv - 1, T - 1] = np.inf
    z[B - 1, 0, T - 2] = -np.inf
    ridx, rd = c_oracle.vq_argmin(z, cb)
    idx, d = vq_run(z, cb, offset)
    assert np.array_equal(idx, ridx), (np.argwhere(idx != ridx)[:5], idx[idx != ridx][:5], ridx[idx != ridx][:5])
    nan = np.isnan(rd)
    assert np.array_equal(np.isnan(d), nan)
    assert np.array_equal(bits(d)[~nan], bits(rd)[~nan])


# ------------------------------------------------------------------ 7. samplers
@pytest.mark.parametrize("kind", ["ffbs", "markov"])
@pytest.mark.parametrize("K,T,N", [(8, 65, 130), (16, 64, 1), (32, 130, 130), (8, 130, 1), (32, 63, 65)])
def test_sampler_paths_on_misaligned_inputs(kind, K, T, N):
    """SR.EXACT_CASES with K % 4 == 0 (row16 = false in sample_go) with the head (filt / log_pi),
    log_A and u 4 bytes off: the reference's paths exactly, and the aligned call's."""
    assert (K, T, N) in SR.EXACT_CASES
    c = SR.exact_case(K, T, N)
    ref, u_used, _ = c[kind]
    head = c["filt"] if kind == "ffbs" else c["log_pi"]
    d_L = torch.from_numpy(c["lengths"]).cuda()
    got = raw_sample(kind, offset_view(head), offset_view(c["log_A"]), d_L, offset_view(u_used))
    g = host(got)
    assert np.array_equal(g, ref), (np.argwhere(g != ref)[:5], g[g != ref][:5], ref[g != ref][:5])
    al = raw_sample(kind, *gpu(head, c["log_A"]), d_L, *gpu(u_used))
    assert torch.equal(got, al)
