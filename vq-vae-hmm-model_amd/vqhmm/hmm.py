"""Hard-regime kernels: VQ nearest-codeword argmin, HMM forward-backward and
Viterbi over the Prior's tables.  HIP only (libvqhmm.so).

The reference defines these only in prose:
  VQ         pseudocode.txt:11-18 (`quantize`), hard regimes backtesting.py:154-155
  fwd-bwd    math.md:23-67 with Prior.forward tables (VQ_VAE_HMM_fixed.py:59-71)
  Viterbi    same tables, max-plus
The exact numerical contracts are documented in include/vqhmm.h.
"""
import torch

from . import _ext


def vq_argmin(z, codebook, return_dist=False):
    """z (B, Dv, T) channels-first, codebook (K, Dv) -> idx (B, T) int32 [, dmin (B, T)].

    idx[b, t] = argmin_k sum_d (z[b, d, t] - codebook[k, d])^2, ties -> lowest k.
    """
    _ext.require_device(z, codebook)
    if z.dim() != 3 or codebook.dim() != 2 or z.shape[1] != codebook.shape[1]:
        raise ValueError(f"vq_argmin: expected z (B,Dv,T) and codebook (K,Dv), got {tuple(z.shape)} {tuple(codebook.shape)}")
    z = z.contiguous().float()
    codebook = codebook.contiguous().float()
    B, Dv, T = z.shape
    K = codebook.shape[0]
    idx = torch.empty((B, T), dtype=torch.int32, device=z.device)
    dmin = torch.empty((B, T), dtype=torch.float32, device=z.device) if return_dist else None
    lib = _ext.load()
    _ext.check(lib.vqhmm_vq_argmin_f32(_ext.ptr(z), B, Dv, T, _ext.ptr(codebook), K, _ext.ptr(idx),
                                       _ext.ptr(dmin), _ext.stream_ptr(z.device)), "vq_argmin")
    return (idx, dmin) if return_dist else idx


def regime_argmax(q):
    """q (B, K, T) -> (B, T) int64: q.argmax(dim=1) by torch.argmax's rule (first index on
    ties, NaN is the maximum), the hard regimes of backtesting.py:154-155 on given probabilities."""
    _ext.require_device(q)
    if q.dim() != 3:
        raise ValueError(f"regime_argmax: expected q (B, K, T), got {tuple(q.shape)}")
    q = q.contiguous().float()
    B, K, T = q.shape
    idx = torch.empty((B, T), dtype=torch.int32, device=q.device)
    _ext.check(_ext.load().vqhmm_argmax_f32(_ext.ptr(q), B, K, T, _ext.ptr(idx), _ext.stream_ptr(q.device)),
               "regime_argmax")
    return idx.long()


class _Quantize(torch.autograd.Function):
    """Forward: ONE fused kernel pass (vqhmm_vq_quantize_f32: argmin, z_q gather, straight-through
    value, sum (z - z_q)^2 in fp64) + a fixed-order partial sum.  Backward (autograd of
    pseudocode.txt:13,17-18): the straight-through output passes its gradient to z unchanged;
    commit = beta * sse / n adds beta * 2 (z - z_q) / n to dz; the codebook loss sse / n gives
    dcodebook[k] = sum over positions with idx = k of 2 (z_q - z) / n."""

    @staticmethod
    def forward(ctx, z, codebook, beta):
        B, Dv, T = z.shape
        K = codebook.shape[0]
        idx = torch.empty((B, T), dtype=torch.int32, device=z.device)
        zq_st = torch.empty_like(z)
        sse = torch.zeros((), dtype=torch.float64, device=z.device)
        lib = _ext.load()
        nb = lib.vqhmm_vq_quantize_workspace_size(B, Dv, T, K)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=z.device)
        _ext.check(lib.vqhmm_vq_quantize_f32(_ext.ptr(z), B, Dv, T, _ext.ptr(codebook), K, _ext.ptr(idx),
                                             _ext.ptr(zq_st), _ext.ptr(sse), _ext.ptr(ws), ws.numel(),
                                             _ext.stream_ptr(z.device)), "quantize")
        n = float(max(z.numel(), 1))
        mse = (sse / n).float()
        ctx.save_for_backward(z, codebook, idx)
        ctx.beta, ctx.n = float(beta), n
        ctx.mark_non_differentiable(idx)
        return zq_st, idx, beta * mse, mse

    @staticmethod
    def backward(ctx, g_zq, g_idx, g_commit, g_cb):
        z, codebook, idx = ctx.saved_tensors
        dz = dcb = None
        zq = codebook[idx.long()].permute(0, 2, 1)  # (B, Dv, T)
        diff = z - zq
        if ctx.needs_input_grad[0]:
            dz = g_zq if g_zq is not None else torch.zeros_like(z)
            if g_commit is not None:
                dz = dz + g_commit * (ctx.beta * 2.0 / ctx.n) * diff
        if ctx.needs_input_grad[1] and g_cb is not None:
            w = (g_cb * (-2.0 / ctx.n)) * diff  # d cb_loss / d z_q
            dcb = torch.zeros_like(codebook).index_add_(0, idx.long().reshape(-1),
                                                        w.permute(0, 2, 1).reshape(-1, codebook.shape[1]))
        return dz, dcb, None


def quantize(z, codebook, beta=0.25):
    """VQ-VAE quantizer of pseudocode.txt:11-18 on channels-first z (B, Dv, T).

    Returns (z_q_st, idx, commit_loss, codebook_loss):
      idx = argmin_k ||z - c_k||^2 (the vq_argmin contract); z_q = codebook[idx];
      z_q_st = z + (z_q - z).detach() (straight-through, :13); commit = beta * MSE(z, sg(z_q)) (:17);
      codebook = MSE(z_q, sg(z)) (:18).
    The forward is one HIP pass (argmin + gather + straight-through value + the squared-error
    partial sums in the kernel's epilogue); the gradients follow the reference's autograd.
    """
    _ext.require_device(z, codebook)
    if z.dim() != 3 or codebook.dim() != 2 or z.shape[1] != codebook.shape[1]:
        raise ValueError(f"quantize: expected z (B,Dv,T) and codebook (K,Dv), got {tuple(z.shape)} "
                         f"{tuple(codebook.shape)}")
    return _Quantize.apply(z.contiguous().float(), codebook.contiguous().float(), float(beta))


def _hmm_inputs(log_pi, log_A, em, lengths):
    _ext.require_device(log_pi, log_A, em)
    if log_A.dim() != 4 or em.dim() != 3 or log_A.shape[:2] != em.shape[:2] or log_A.shape[2:] != (em.shape[2],) * 2:
        raise ValueError(f"expected log_A (B,T,K,K) and em (B,T,K), got {tuple(log_A.shape)} {tuple(em.shape)}")
    B, T, K = em.shape
    if log_pi.shape != (K,):
        raise ValueError(f"log_pi must have shape ({K},)")
    if lengths is None:
        lengths = torch.full((B,), T, dtype=torch.int64, device=em.device)
    lengths = torch.as_tensor(lengths).to(em.device, torch.int64).contiguous()
    return (log_pi.contiguous().float(), log_A.contiguous().float(), em.contiguous().float(), lengths, B, T, K)


def _length0(B, value, device):
    """The (B,) result of a batch of length-0 sequences.  For T = 0 the C entries launch nothing and
    write nothing (include/vqhmm.h), so the wrappers fill in what the kernels give a sequence of
    length 0: score = -inf, logZ = loglik = NaN."""
    return torch.full((B,), value, dtype=torch.float32, device=device)


def viterbi(log_pi, log_A, em, lengths=None):
    """MAP state path under the Prior's tables.

    log_pi (K,), log_A (B,T,K,K) with log_A[:, t] the t-1 -> t transition
    (as Prior.forward returns it, VQ_VAE_HMM_fixed.py:69-71), em (B,T,K)
    emission log-potentials, lengths (B,) -> path (B,T) int32 (-1 past the
    length), score (B,) fp32.  Bit-exact vs the fp32 oracle contract.
    """
    log_pi, log_A, em, lengths, B, T, K = _hmm_inputs(log_pi, log_A, em, lengths)
    if T == 0:
        return torch.empty((B, 0), dtype=torch.int32, device=em.device), _length0(B, float("-inf"), em.device)
    path = torch.empty((B, T), dtype=torch.int32, device=em.device)
    score = torch.empty((B,), dtype=torch.float32, device=em.device)
    lib = _ext.load()
    nb = lib.vqhmm_viterbi_workspace_size(B, T, K)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=em.device)
    _ext.check(lib.vqhmm_viterbi_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(em), _ext.ptr(lengths), B, T, K,
                                     _ext.ptr(path), _ext.ptr(score), _ext.ptr(ws), nb, _ext.stream_ptr(em.device)),
               "viterbi")
    return path, score


def _forward_backward_plain(log_pi, log_A, em, lengths=None):
    """gamma and logZ as plain tensors (vqhmm_fwdbwd_f32, any supported K)."""
    log_pi, log_A, em, lengths, B, T, K = _hmm_inputs(log_pi, log_A, em, lengths)
    if T == 0:
        return torch.empty((B, 0, K), dtype=torch.float32, device=em.device), _length0(B, float("nan"), em.device)
    gamma = torch.empty((B, T, K), dtype=torch.float32, device=em.device)
    logZ = torch.empty((B,), dtype=torch.float32, device=em.device)
    lib = _ext.load()
    nb = lib.vqhmm_fwdbwd_workspace_size(B, T, K)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=em.device)
    _ext.check(lib.vqhmm_fwdbwd_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(em), _ext.ptr(lengths), B, T, K,
                                    _ext.ptr(gamma), _ext.ptr(logZ), _ext.ptr(ws), nb, _ext.stream_ptr(em.device)),
               "forward_backward")
    return gamma, logZ


PAIR_MAX_K = 32  # the filter / xi kernels' state limit (hmm_pair.hip)


def _fwdbwd_xi(log_pi, log_A, em, lengths, B, T, K):
    """vqhmm_fwdbwd_xi_f32 on prepared inputs -> (gamma, xi, logZ)."""
    if T == 0:
        return (torch.empty((B, 0, K), dtype=torch.float32, device=em.device),
                torch.empty((B, 0, K, K), dtype=torch.float32, device=em.device), _length0(B, float("nan"), em.device))
    gamma = torch.empty((B, T, K), dtype=torch.float32, device=em.device)
    xi = torch.empty((B, T, K, K), dtype=torch.float32, device=em.device)
    logZ = torch.empty((B,), dtype=torch.float32, device=em.device)
    lib = _ext.load()
    nb = lib.vqhmm_fwdbwd_xi_workspace_size(B, T, K)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=em.device)
    _ext.check(lib.vqhmm_fwdbwd_xi_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(em), _ext.ptr(lengths), B, T, K,
                                       _ext.ptr(gamma), _ext.ptr(xi), _ext.ptr(logZ), _ext.ptr(ws), nb,
                                       _ext.stream_ptr(em.device)), "pairwise_posteriors")
    return gamma, xi, logZ


class _LogZFn(torch.autograd.Function):
    """forward_backward with logZ differentiable: the forward runs vqhmm_fwdbwd_xi_f32 (gamma and logZ
    by the same launch as the plain path, so the same bits) and keeps gamma and xi, which ARE the
    gradients: d logZ / d log_A = xi, d logZ / d em = gamma, d logZ / d log_pi = sum_b gamma[b, 0]."""

    @staticmethod
    def forward(ctx, log_pi, log_A, em, lengths):
        B, T, K = em.shape
        gamma, xi, logZ = _fwdbwd_xi(log_pi, log_A, em, lengths, B, T, K)
        ctx.save_for_backward(gamma, xi, lengths)
        ctx.mark_non_differentiable(gamma)
        return gamma, logZ

    @staticmethod
    def backward(ctx, g_gamma, g_logZ):
        gamma, xi, lengths = ctx.saved_tensors
        # a length-0 sequence has logZ = NaN and no gradient: whatever arrives for it is dropped
        g = torch.where(lengths > 0, g_logZ, torch.zeros_like(g_logZ))
        d_pi = d_A = d_em = None
        if ctx.needs_input_grad[0]:
            d_pi = (g[:, None] * gamma[:, 0]).sum(0) if gamma.shape[1] else torch.zeros_like(gamma[0, 0])
        if ctx.needs_input_grad[1]:
            d_A = g[:, None, None, None] * xi
        if ctx.needs_input_grad[2]:
            d_em = g[:, None, None] * gamma
        return d_pi, d_A, d_em, None


def forward_backward(log_pi, log_A, em, lengths=None):
    """Posterior state marginals gamma (B,T,K) and log-partition logZ (B,).

    When log_pi, log_A or em requires grad, logZ carries a grad_fn whose backward is exact:
    d logZ / d log_A = xi (the pairwise posteriors), d logZ / d em = gamma, d logZ / d log_pi =
    sum_b gamma[b, 0] (K <= 32); gamma itself is not differentiable.  Without gradient-requiring
    inputs this is the plain launch; gamma and logZ are the same bits either way."""
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in (log_pi, log_A, em))):
        return _forward_backward_plain(log_pi, log_A, em, lengths)
    log_pi, log_A, em, lengths, B, T, K = _hmm_inputs(log_pi, log_A, em, lengths)
    if K > PAIR_MAX_K:
        raise RuntimeError(f"forward_backward: gradients of logZ need K <= {PAIR_MAX_K} states (got K = {K}); "
                           "detach the inputs for the posteriors alone")
    if B * T == 0:
        return _forward_backward_plain(log_pi, log_A, em, lengths)
    return _LogZFn.apply(log_pi, log_A, em, lengths)


def forward_filter(log_pi, log_A, em, lengths=None):
    """Causal (filtered) posteriors filt (B,T,K), filt[b,t] = p(z_t | x_{1:t}) (rows sum to 1 inside
    the length, 0 past it), and loglik (B,) = log p(x_{1:L}) (NaN for length 0).  Unlike gamma,
    filt[b,t] does not look at steps after t.  1 <= K <= 32."""
    log_pi, log_A, em, lengths, B, T, K = _hmm_inputs(log_pi, log_A, em, lengths)
    if T == 0:
        if K > PAIR_MAX_K:
            raise RuntimeError(f"vqhmm: forward_filter (K = {K}, limit {PAIR_MAX_K}) failed: unsupported shape")
        return torch.empty((B, 0, K), dtype=torch.float32, device=em.device), _length0(B, float("nan"), em.device)
    filt = torch.empty((B, T, K), dtype=torch.float32, device=em.device)
    loglik = torch.empty((B,), dtype=torch.float32, device=em.device)
    with torch.no_grad():
        _ext.check(_ext.load().vqhmm_filter_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(em), _ext.ptr(lengths), B,
                                                T, K, _ext.ptr(filt), _ext.ptr(loglik), _ext.stream_ptr(em.device)),
                   f"forward_filter (K = {K}, limit {PAIR_MAX_K})")
    return filt, loglik


def _sample_uniforms(uniforms, B, N, T, device, generator, what):
    if uniforms is None:
        return torch.rand((B, N, T), generator=generator, device=device, dtype=torch.float32)
    _ext.require_device(uniforms)
    if tuple(uniforms.shape) != (B, N, T) or uniforms.dtype != torch.float32:
        raise ValueError(f"{what}: uniforms must be fp32 of shape ({B}, {N}, {T}), got {uniforms.dtype} "
                         f"{tuple(uniforms.shape)}")
    return uniforms.detach().contiguous()


def _n_samples(n_samples, what):
    n = int(n_samples)
    if n < 0:
        raise ValueError(f"{what}: n_samples must be >= 0 (got {n_samples})")
    return n


def sample_posterior_paths(log_pi, log_A, em, lengths=None, n_samples=1, generator=None, uniforms=None):
    """n_samples regime paths per sequence from the posterior p(z_{0:L-1} | x_{1:L}) by forward
    filtering, backward sampling: vqhmm_filter_f32, then vqhmm_ffbs_sample_f32 on its filt.

    Inputs as forward_filter's (1 <= K <= 32).  Returns paths (B, n_samples, T) int32, -1 past each
    length.  A sequence whose log-likelihood is not finite (impossible under the tables, or of
    length 0) has no posterior: all of its samples are -1, its batch neighbours are unaffected.
    uniforms: a (B, n_samples, T) fp32 device tensor in [0, 1), used as it is; uniforms[b, s, t]
    draws z_t of sample s by the inverse-CDF rule of include/vqhmm.h, so the same uniforms give the
    same paths (reproducible draws, common random numbers across scenarios).  Without it the
    function draws torch.rand((B, n_samples, T), generator=generator) on the device; either way that
    buffer costs 4 * B * n_samples * T bytes.  Runs under no_grad on detached inputs."""
    log_pi, log_A, em, lengths, B, T, K = _hmm_inputs(log_pi, log_A, em, lengths)
    N = _n_samples(n_samples, "sample_posterior_paths")
    if K > PAIR_MAX_K:
        raise RuntimeError(f"sample_posterior_paths: K <= {PAIR_MAX_K} states (got K = {K})")
    with torch.no_grad():
        if B * N * T == 0:
            return torch.full((B, N, T), -1, dtype=torch.int32, device=em.device)
        paths = torch.empty((B, N, T), dtype=torch.int32, device=em.device)  # the kernel writes every element
        u = _sample_uniforms(uniforms, B, N, T, em.device, generator, "sample_posterior_paths")
        log_pi, log_A, em = log_pi.detach(), log_A.detach(), em.detach()
        filt = torch.empty((B, T, K), dtype=torch.float32, device=em.device)
        loglik = torch.empty((B,), dtype=torch.float32, device=em.device)
        lib = _ext.load()
        st = _ext.stream_ptr(em.device)
        _ext.check(lib.vqhmm_filter_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(em), _ext.ptr(lengths), B, T, K,
                                        _ext.ptr(filt), _ext.ptr(loglik), st), "sample_posterior_paths (filter)")
        _ext.check(lib.vqhmm_ffbs_sample_f32(_ext.ptr(filt), _ext.ptr(log_A), _ext.ptr(lengths), _ext.ptr(u), B, T, K,
                                             N, _ext.ptr(paths), st), "sample_posterior_paths")
        return torch.where(torch.isfinite(loglik)[:, None, None], paths, torch.full_like(paths, -1))


def simulate_paths(log_pi, log_A, lengths=None, n_samples=1, generator=None, uniforms=None):
    """n_samples regime paths per sequence simulated under the tables alone: z_0 ~ softmax(log_pi),
    z_t ~ softmax_j(log_A[b, t, z_{t-1}, :]) (vqhmm_markov_sample_f32); no observations enter.

    log_pi (K,), log_A (B,T,K,K) as Prior.forward returns them (1 <= K <= 32; rows need not be
    normalised, -inf is a structural zero that is never drawn).  Returns paths (B, n_samples, T)
    int32, -1 past each length (and from the first position whose row has no mass onward).
    uniforms / generator: as sample_posterior_paths; the (B, n_samples, T) fp32 buffer costs
    4 * B * n_samples * T bytes.  Runs under no_grad on detached inputs."""
    _ext.require_device(log_pi, log_A)
    if log_A.dim() != 4 or log_A.shape[2] != log_A.shape[3]:
        raise ValueError(f"expected log_A (B,T,K,K), got {tuple(log_A.shape)}")
    B, T, K = log_A.shape[:3]
    em = log_A.new_empty((B, T, K))  # shape carrier for the shared validation, never read
    log_pi, log_A, _, lengths, B, T, K = _hmm_inputs(log_pi, log_A, em, lengths)
    N = _n_samples(n_samples, "simulate_paths")
    if K > PAIR_MAX_K:
        raise RuntimeError(f"simulate_paths: K <= {PAIR_MAX_K} states (got K = {K})")
    with torch.no_grad():
        if B * N * T == 0:
            return torch.full((B, N, T), -1, dtype=torch.int32, device=log_A.device)
        paths = torch.empty((B, N, T), dtype=torch.int32, device=log_A.device)  # the kernel writes every element
        u = _sample_uniforms(uniforms, B, N, T, log_A.device, generator, "simulate_paths")
        log_pi, log_A = log_pi.detach(), log_A.detach()
        _ext.check(_ext.load().vqhmm_markov_sample_f32(_ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(lengths),
                                                       _ext.ptr(u), B, T, K, N, _ext.ptr(paths),
                                                       _ext.stream_ptr(log_A.device)), "simulate_paths")
        return paths


def pairwise_posteriors(log_pi, log_A, em, lengths=None):
    """gamma (B,T,K), xi (B,T,K,K), logZ (B,): xi[b,t,i,j] = p(z_{t-1} = i, z_t = j | x_{1:L}) for
    1 <= t < L and 0 elsewhere (the E-step statistics of EM on the transition model: sum_t xi_t);
    gamma and logZ are forward_backward's, bit for bit.  1 <= K <= 32."""
    log_pi, log_A, em, lengths, B, T, K = _hmm_inputs(log_pi, log_A, em, lengths)
    if K > PAIR_MAX_K:
        raise RuntimeError(f"pairwise_posteriors: K <= {PAIR_MAX_K} states (got K = {K})")
    with torch.no_grad():
        return _fwdbwd_xi(log_pi.detach(), log_A.detach(), em.detach(), lengths, B, T, K)
