"""Stationary HMM with diagonal-Gaussian emissions on continuous observations (returns, the `u` features,
encoder latents): Baum-Welch EM, scoring, posteriors and ancestral sampling.  HIP only: the emission
log-densities, the fused E-step and the sampler are the kernels of hmm_gauss.hip (vqhmm_gauss_emission_f32 /
vqhmm_gauss_estep_f32 / vqhmm_gauss_sample_f32, contracts in include/vqhmm.h); the M-step is S*S + 2*S*D numbers
of torch arithmetic in fp64 on the device.  With every row of A tied to pi (`as_mixture`, `fit(mixture=True)`)
the model is a diagonal Gaussian mixture.  `gauss_log_prob` is the differentiable log-likelihood (its backward
is one weighted E-step).

covariance_type="full" gives every state a full covariance Sigma_s = L_s L_s^T (parameter scale_tril = L_s): the
kernels of hmm_gauss_full.hip (vqhmm_gauss_full_emission_f32 / vqhmm_gauss_full_estep_f32) take W_s = L_s^-1 and
return the S x D x D second moments; the M-step adds sklearn's reg_covar to the diagonal and factors in fp64 on the
device.  `gauss_full_log_prob` is its differentiable log-likelihood, `regime_moments` / `regime_covariance` the
same moments under a caller-supplied posterior (vqhmm_gauss_moments_f32).

Read-outs of a fitted model, both covariance types, fused on x (no emission table, no expanded log_A): `decode`
(the MAP regime path, vqhmm_gauss_viterbi_f32 / vqhmm_gauss_full_viterbi_f32), `filter` / `update` (the causal
filter with a carried (B,S) state, vqhmm_gauss_filter_f32 / vqhmm_gauss_full_filter_f32) and `predict_next`.

Restarts (`fit(n_init=R)`) run on gauss_hmm_ensemble.GaussianHMMEnsemble, R models in one launch
(vqhmm_gauss_estep_batched_f32 / vqhmm_gauss_full_estep_batched_f32).

Looking forward from a filtered state: `simulate` (vqhmm_gauss_scenario_f32, hmm_gauss_scenario.hip) draws N
scenario paths per start with the random numbers generated on chip (Philox4x32-10) and reduces a regime-dependent
portfolio's wealth path to final wealth and maximum drawdown per path; `scenario_summary` is the table over them.
"""
import torch

from . import _ext
from .codebook import Codebook
from .codehmm import CodeHMM

MAX_STATES = 32   # the kernels' limits (hmm_gauss.hip)
MAX_DIM = 64
MAX_DIM_FULL = 32      # hmm_gauss_full.hip: 1 <= D <= 32 and S * D * D <= MAX_SDD_FULL
MAX_SDD_FULL = 8192


def _full_supported(S, D):
    return 1 <= S <= MAX_STATES and 1 <= D <= MAX_DIM_FULL and S * D * D <= MAX_SDD_FULL


def _full_domain(what, S, D):
    if not _full_supported(S, D):
        raise ValueError(f"{what}: full covariances need 1 <= S <= {MAX_STATES}, 1 <= D <= {MAX_DIM_FULL} and "
                         f"S * D * D <= {MAX_SDD_FULL} (got {S}, {D})")


def _check_x(what, ref, x, lengths, D):
    """x (B,T,D) float and lengths (B,) or None on ref's device -> (fp32 contiguous x, int64 lengths, B, T)."""
    _ext.require_device(ref, x)
    if x.dim() != 3 or x.shape[2] != D or not x.dtype.is_floating_point:
        raise ValueError(f"{what}: expected x (B, T, {D}) floating point, got {tuple(x.shape)} {x.dtype}")
    x = x.detach().to(torch.float32).contiguous()
    B, T = x.shape[:2]
    if lengths is None:
        lengths = torch.full((B,), T, dtype=torch.int64, device=x.device)
    lengths = torch.as_tensor(lengths).to(x.device, torch.int64).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f"{what}: lengths must have shape ({B},)")
    return x, lengths, B, T


def _estep(what, log_pi, log_A, mean, log_var, x, lengths, shift, weights, want_loglik, want_gamma):
    """vqhmm_gauss_estep_f32 on contiguous fp32 device tensors -> dict of the fp64 counts (views of `flat`:
    pi_cnt, trans_cnt, occ, m1, m2) [, loglik (B) fp32] [, gamma (B,T,S) fp32] and the shift used."""
    S, D = mean.shape
    B, T = x.shape[:2]
    dev = x.device
    flat = torch.empty(S + S * S + S + 2 * S * D, dtype=torch.float64, device=dev)
    o = [0, S, S + S * S, 2 * S + S * S, 2 * S + S * S + S * D]
    out = {"pi_cnt": flat[o[0]:o[1]], "trans_cnt": flat[o[1]:o[2]].view(S, S), "occ": flat[o[2]:o[3]],
           "m1": flat[o[3]:o[4]].view(S, D), "m2": flat[o[4]:].view(S, D), "flat": flat, "shift": shift}
    loglik = torch.empty((B,), dtype=torch.float32, device=dev) if want_loglik else None
    gamma = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_gamma else None
    lib = _ext.load()
    nb = lib.vqhmm_gauss_estep_workspace_size(B, T, S, D)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        _ext.check(lib.vqhmm_gauss_estep_f32(
            _ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(log_var), _ext.ptr(x), _ext.ptr(lengths),
            _ext.ptr(shift), _ext.ptr(weights), B, T, S, D, _ext.ptr(out["pi_cnt"]), _ext.ptr(out["trans_cnt"]),
            _ext.ptr(out["occ"]), _ext.ptr(out["m1"]), _ext.ptr(out["m2"]), _ext.ptr(loglik), _ext.ptr(gamma),
            _ext.ptr(ws), nb, _ext.stream_ptr(dev)), what)
    if want_loglik:
        out["loglik"] = loglik
    if want_gamma:
        out["gamma"] = gamma
    return out


class _GaussLogProb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_pi, log_A, mean, log_var, x, lengths):
        ll = _estep("gauss_log_prob", log_pi, log_A, mean, log_var, x, lengths, None, None, True, False)["loglik"]
        ctx.save_for_backward(log_pi, log_A, mean, log_var, x, lengths)
        return ll

    @staticmethod
    def backward(ctx, g):
        log_pi, log_A, mean, log_var, x, lengths = ctx.saved_tensors
        w = g.detach().to(torch.float32).reshape(-1).contiguous()
        # moments about the centre of the means: (m1, m2) -> sums of (x - mu) and (x - mu)^2 without a
        # difference of numbers the size of |x|^2
        shift = mean.mean(0).contiguous()
        c = _estep("gauss_log_prob backward", log_pi, log_A, mean, log_var, x, lengths, shift, w, False, False)
        occ = c["occ"].unsqueeze(1)
        dm = mean.double() - shift.double()
        ivar = torch.exp(-log_var.double())
        r1 = c["m1"] - dm * occ                                  # sum w gamma (x - mu)
        r2 = c["m2"] - 2.0 * dm * c["m1"] + dm * dm * occ        # sum w gamma (x - mu)^2
        return (c["pi_cnt"].float(), c["trans_cnt"].float(), (r1 * ivar).float(),
                (0.5 * (r2 * ivar - occ)).float(), None, None)


def gauss_log_prob(log_pi, log_A, mean, log_var, x, lengths=None):
    """log p(x[b, :lengths[b]]) (B,) fp32 under the Gaussian HMM (log_pi (S,), log_A (S,S), mean (S,D), log_var
    (S,D), fp32 device tensors), differentiable with respect to the four parameter tensors (log_pi and log_A as
    free variables: train logits through log_softmax).  The forward is the fused E-step's loglik; the backward is
    one weighted E-step with weights = grad_output: d/dlog_pi = gamma_0, d/dlog_A = sum xi, d/dmean = (m1 -
    (mean - shift) occ) / var, d/dlog_var = (sum gamma (x - mean)^2 / var - occ) / 2.  A sequence whose loglik is
    not finite contributes exactly zero gradient.  x is data: it raises if x.requires_grad."""
    if not torch.is_tensor(mean) or mean.dim() != 2:
        raise ValueError("gauss_log_prob: mean must be a float32 tensor of shape (S, D)")
    S, D = int(mean.shape[0]), int(mean.shape[1])
    for name, t, shape in (("log_pi", log_pi, (S,)), ("log_A", log_A, (S, S)), ("mean", mean, (S, D)),
                           ("log_var", log_var, (S, D))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"gauss_log_prob: {name} must be a float32 tensor of shape {shape}")
    if not (1 <= S <= MAX_STATES and 1 <= D <= MAX_DIM):
        raise ValueError(f"gauss_log_prob: 1 <= S <= {MAX_STATES} and 1 <= D <= {MAX_DIM} (got {S}, {D})")
    if torch.is_tensor(x) and x.requires_grad:
        raise ValueError("gauss_log_prob: x is data and gets no gradient (x.requires_grad is set)")
    _ext.require_device(log_pi, log_A, mean, log_var)
    x, lengths, _, _ = _check_x("gauss_log_prob", log_pi, x, lengths, D)
    return _GaussLogProb.apply(log_pi.contiguous(), log_A.contiguous(), mean.contiguous(), log_var.contiguous(), x,
                               lengths)


# ------------------------------------------------------------------ full covariances
def _prec_chol(scale_tril):
    """W = L^-1 (S,D,D) fp32 from the lower Cholesky factors L of the covariances: derived in fp64 on the device,
    rounded once, the strict upper triangle exactly 0."""
    L = scale_tril.detach().double().tril()
    eye = torch.eye(L.shape[-1], dtype=torch.float64, device=L.device).expand_as(L)
    return torch.linalg.solve_triangular(L, eye, upper=False).tril().float().contiguous()


def _cholesky(cov):
    """Lower Cholesky factors of cov (S,D,D) fp64 and a per-matrix success mask, without a host sync:
    torch.linalg.cholesky_ex, or (a build without it on the device) the D-step column algorithm in torch ops."""
    try:
        L, info = torch.linalg.cholesky_ex(cov)
        return L, (info == 0) & torch.isfinite(L).all((-1, -2))
    except RuntimeError:
        D = cov.shape[-1]
        L = torch.zeros_like(cov)
        ok = torch.ones(cov.shape[:-2], dtype=torch.bool, device=cov.device)
        for k in range(D):
            d = cov[..., k, k] - (L[..., k, :k] ** 2).sum(-1)
            ok = ok & (d > 0)
            r = torch.sqrt(torch.where(d > 0, d, torch.ones_like(d)))
            L[..., k, k] = r
            if k + 1 < D:
                c = cov[..., k + 1:, k] - (L[..., k + 1:, :k] * L[..., k:k + 1, :k]).sum(-1)
                L[..., k + 1:, k] = c / r.unsqueeze(-1)
        return L, ok & torch.isfinite(L).all((-1, -2))


def _estep_full(what, log_pi, log_A, mean, prec, x, lengths, shift, weights, want_loglik, want_gamma):
    """vqhmm_gauss_full_estep_f32 on contiguous fp32 device tensors -> dict of the fp64 counts (views of `flat`:
    pi_cnt, trans_cnt, occ, m1, m2 (S,D,D)) [, loglik (B) fp32] [, gamma (B,T,S) fp32] and the shift used."""
    S, D = mean.shape
    B, T = x.shape[:2]
    dev = x.device
    flat = torch.empty(S + S * S + S + S * D + S * D * D, dtype=torch.float64, device=dev)
    o = [0, S, S + S * S, 2 * S + S * S, 2 * S + S * S + S * D]
    out = {"pi_cnt": flat[o[0]:o[1]], "trans_cnt": flat[o[1]:o[2]].view(S, S), "occ": flat[o[2]:o[3]],
           "m1": flat[o[3]:o[4]].view(S, D), "m2": flat[o[4]:].view(S, D, D), "flat": flat, "shift": shift}
    loglik = torch.empty((B,), dtype=torch.float32, device=dev) if want_loglik else None
    gamma = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_gamma else None
    lib = _ext.load()
    nb = lib.vqhmm_gauss_full_estep_workspace_size(B, T, S, D)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        _ext.check(lib.vqhmm_gauss_full_estep_f32(
            _ext.ptr(log_pi), _ext.ptr(log_A), _ext.ptr(mean), _ext.ptr(prec), _ext.ptr(x), _ext.ptr(lengths),
            _ext.ptr(shift), _ext.ptr(weights), B, T, S, D, _ext.ptr(out["pi_cnt"]), _ext.ptr(out["trans_cnt"]),
            _ext.ptr(out["occ"]), _ext.ptr(out["m1"]), _ext.ptr(out["m2"]), _ext.ptr(loglik), _ext.ptr(gamma),
            _ext.ptr(ws), nb, _ext.stream_ptr(dev)), what)
    if want_loglik:
        out["loglik"] = loglik
    if want_gamma:
        out["gamma"] = gamma
    return out


def _estep_members(what, full, log_pi, log_A, mean, last, x, lengths, shift, weights, want_loglik, want_gamma,
                   max_workspace_bytes=None):
    """vqhmm_gauss_estep_batched_f32 / vqhmm_gauss_full_estep_batched_f32 on stacked contiguous fp32 parameters
    (M,S) / (M,S,S) / (M,S,D) / `last` = log_var (M,S,D) or W (M,S,D,D), the shared x (B,T,D), lengths (B), shift (D)
    or None and weights (M,B) fp32 or None -> (pi_cnt (M,S), trans_cnt (M,S,S), occ (M,S), m1 (M,S,D), m2 (M,S,D) or
    (M,S,D,D) fp64, loglik (M,B) or None, gamma (M,B,T,S) or None).  The members run in groups whose workspace fits
    max_workspace_bytes (None: one group); a member's bits do not depend on its group."""
    M, S, D = mean.shape
    B, T = x.shape[:2]
    dev = x.device
    f64 = dict(dtype=torch.float64, device=dev)
    pi, tr, occ = torch.empty((M, S), **f64), torch.empty((M, S, S), **f64), torch.empty((M, S), **f64)
    m1 = torch.empty((M, S, D), **f64)
    m2 = torch.empty((M, S, D, D) if full else (M, S, D), **f64)
    ll = torch.empty((M, B), dtype=torch.float32, device=dev) if want_loglik else None
    gm = torch.empty((M, B, T, S), dtype=torch.float32, device=dev) if want_gamma else None
    lib = _ext.load()
    size, entry = ((lib.vqhmm_gauss_full_estep_batched_workspace_size, lib.vqhmm_gauss_full_estep_batched_f32) if full
                   else (lib.vqhmm_gauss_estep_batched_workspace_size, lib.vqhmm_gauss_estep_batched_f32))
    G = min(M, 65535)
    if max_workspace_bytes is not None:
        per = size(B, T, S, D, 1)
        G = max(1, min(G, int(max_workspace_bytes) // max(per, 1)))
    nb = size(B, T, S, D, G)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    st = _ext.stream_ptr(dev)

    def at(t, m0):
        return _ext.ptr(t[m0:]) if t is not None else _ext.ptr(None)

    with torch.no_grad():
        for m0 in range(0, M, G):
            _ext.check(entry(
                at(log_pi, m0), at(log_A, m0), at(mean, m0), at(last, m0), _ext.ptr(x), _ext.ptr(lengths),
                _ext.ptr(shift), at(weights, m0), B, T, S, D, min(G, M - m0), at(pi, m0), at(tr, m0), at(occ, m0),
                at(m1, m0), at(m2, m0), at(ll, m0), at(gm, m0), _ext.ptr(ws), nb, st), what)
    return pi, tr, occ, m1, m2, ll, gm


class _GaussFullLogProb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_pi, log_A, mean, scale_tril, x, lengths):
        prec = _prec_chol(scale_tril)
        ll = _estep_full("gauss_full_log_prob", log_pi, log_A, mean, prec, x, lengths, None, None, True,
                         False)["loglik"]
        ctx.save_for_backward(log_pi, log_A, mean, scale_tril, prec, x, lengths)
        return ll

    @staticmethod
    def backward(ctx, g):
        log_pi, log_A, mean, scale_tril, prec, x, lengths = ctx.saved_tensors
        w = g.detach().to(torch.float32).reshape(-1).contiguous()
        shift = mean.mean(0).contiguous()   # moments about the centre of the means, as gauss_log_prob
        c = _estep_full("gauss_full_log_prob backward", log_pi, log_A, mean, prec, x, lengths, shift, w, False,
                        False)
        occ = c["occ"]
        dm = mean.double() - shift.double()
        m1 = c["m1"]
        r1 = m1 - dm * occ[:, None]                                         # sum w gamma (x - mu)
        dm1 = dm[:, :, None] * m1[:, None, :]
        r2 = c["m2"] - dm1 - dm1.transpose(1, 2) + occ[:, None, None] * dm[:, :, None] * dm[:, None, :]
        L = scale_tril.double().tril()
        eye = torch.eye(L.shape[-1], dtype=torch.float64, device=L.device).expand_as(L)
        W = torch.linalg.solve_triangular(L, eye, upper=False)
        sinv = W.transpose(1, 2) @ W
        g_sigma = 0.5 * sinv @ (r2 - occ[:, None, None] * (L @ L.transpose(1, 2))) @ sinv
        return (c["pi_cnt"].float(), c["trans_cnt"].float(), (sinv @ r1.unsqueeze(-1)).squeeze(-1).float(),
                (2.0 * g_sigma @ L).tril().float(), None, None)


def gauss_full_log_prob(log_pi, log_A, mean, scale_tril, x, lengths=None):
    """log p(x[b, :lengths[b]]) (B,) fp32 under the full-covariance Gaussian HMM (log_pi (S,), log_A (S,S), mean
    (S,D), scale_tril (S,D,D) = the lower Cholesky factors L_s of the covariances; fp32 device tensors),
    differentiable with respect to the four parameter tensors.  The forward is the fused full E-step's loglik;
    the backward is one weighted full E-step about shift = mean.mean(0): with R2_s = sum w gamma (x - mu_s)(x -
    mu_s)^T rebuilt from (occ, m1, m2), d/dmean = Sigma^-1 (m1 - (mu - shift) occ), G = 1/2 Sigma^-1 (R2 - occ
    Sigma) Sigma^-1 and d/dscale_tril = tril(2 G L).  Only the lower triangle of scale_tril is read.  A sequence
    whose loglik is not finite contributes exactly zero gradient.  x is data: it raises if x.requires_grad."""
    if not torch.is_tensor(mean) or mean.dim() != 2:
        raise ValueError("gauss_full_log_prob: mean must be a float32 tensor of shape (S, D)")
    S, D = int(mean.shape[0]), int(mean.shape[1])
    for name, t, shape in (("log_pi", log_pi, (S,)), ("log_A", log_A, (S, S)), ("mean", mean, (S, D)),
                           ("scale_tril", scale_tril, (S, D, D))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"gauss_full_log_prob: {name} must be a float32 tensor of shape {shape}")
    _full_domain("gauss_full_log_prob", S, D)
    if torch.is_tensor(x) and x.requires_grad:
        raise ValueError("gauss_full_log_prob: x is data and gets no gradient (x.requires_grad is set)")
    _ext.require_device(log_pi, log_A, mean, scale_tril)
    x, lengths, _, _ = _check_x("gauss_full_log_prob", log_pi, x, lengths, D)
    return _GaussFullLogProb.apply(log_pi.contiguous(), log_A.contiguous(), mean.contiguous(),
                                   scale_tril.contiguous(), x, lengths)


def regime_moments(x, gamma, lengths=None, weights=None, shift=None):
    """The per-regime weighted moments of x (B,T,D) under a given posterior gamma (B,T,S) (an encoder's q, a
    filter's output; any non-negative weights), pooled over the batch (vqhmm_gauss_moments_f32) -> dict(occ (S,),
    m1 (S,D), m2 (S,D,D) fp64, flat, shift): occ = sum_b w_b sum_t gamma, m1 = sum w gamma (x - shift), m2 = sum w
    gamma (x - shift)(x - shift)^T (exactly symmetric).  `flat` is the one buffer they are views of.  A sequence
    with a non-finite x or gamma inside its length contributes nothing."""
    if not torch.is_tensor(gamma) or gamma.dim() != 3 or not gamma.dtype.is_floating_point:
        raise ValueError("regime_moments: gamma must be a floating point tensor of shape (B, T, S)")
    _ext.require_device(gamma)
    if not torch.is_tensor(x) or x.dim() != 3:
        raise ValueError("regime_moments: x must be a tensor of shape (B, T, D)")
    S, D = int(gamma.shape[2]), int(x.shape[2])
    _full_domain("regime_moments", S, D)
    x, lengths, B, T = _check_x("regime_moments", gamma, x, lengths, D)
    if tuple(gamma.shape[:2]) != (B, T):
        raise ValueError(f"regime_moments: gamma must have shape ({B}, {T}, S)")
    gamma = gamma.detach().to(torch.float32).contiguous()
    dev = x.device
    if shift is not None:
        shift = torch.as_tensor(shift).to(dev, torch.float32).contiguous()
        if shift.shape != (D,):
            raise ValueError(f"regime_moments: shift must have shape ({D},)")
    if weights is not None:
        weights = torch.as_tensor(weights).to(dev, torch.float32).contiguous()
        if weights.shape != (B,):
            raise ValueError(f"regime_moments: weights must have shape ({B},)")
    flat = torch.empty(S + S * D + S * D * D, dtype=torch.float64, device=dev)
    out = {"occ": flat[:S], "m1": flat[S:S + S * D].view(S, D), "m2": flat[S + S * D:].view(S, D, D), "flat": flat,
           "shift": shift}
    lib = _ext.load()
    nb = lib.vqhmm_gauss_moments_workspace_size(B, T, S, D)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        _ext.check(lib.vqhmm_gauss_moments_f32(
            _ext.ptr(x), _ext.ptr(gamma), _ext.ptr(lengths), _ext.ptr(shift), _ext.ptr(weights), B, T, S, D,
            _ext.ptr(out["occ"]), _ext.ptr(out["m1"]), _ext.ptr(out["m2"]), _ext.ptr(ws), nb,
            _ext.stream_ptr(dev)), "regime_moments")
    return out


def regime_covariance(x, gamma, lengths=None):
    """-> (mean (S,D), cov (S,D,D)) fp64: the gamma-weighted mean and (biased) covariance of x per regime, pooled
    over the batch; the moments are taken about the data mean.  A regime nothing was counted into gets NaN."""
    if not torch.is_tensor(x) or x.dim() != 3:
        raise ValueError("regime_covariance: x must be a tensor of shape (B, T, D)")
    xc, lc, B, T = _check_x("regime_covariance", gamma, x, lengths, int(x.shape[2]))
    mask = (torch.arange(T, device=xc.device).unsqueeze(0) < lc.clamp(0, T).unsqueeze(1)).unsqueeze(2)
    shift = (torch.where(mask, xc.double(), 0.0).sum((0, 1)) / mask.sum().clamp_min(1)).float().contiguous()
    c = regime_moments(xc, gamma, lc, None, shift)
    occ = c["occ"]
    o = torch.where(occ > 0, occ, torch.full_like(occ, float("nan")))
    mu = c["m1"] / o[:, None]
    cov = c["m2"] / o[:, None, None] - mu[:, :, None] * mu[:, None, :]
    return mu + shift.double(), cov


class Scenarios:
    """What GaussianHMM.simulate returns: final (B,N), drawdown (B,N), wealth (B,N,H), states (B,N,H) int32 and x
    (B,N,H,D); a field that was not computed is None."""
    __slots__ = ("final", "drawdown", "wealth", "states", "x")

    def __init__(self, final=None, drawdown=None, wealth=None, states=None, x=None):
        self.final, self.drawdown, self.wealth, self.states, self.x = final, drawdown, wealth, states, x

    def __repr__(self):
        have = ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__ if getattr(self, k) is not None)
        return f"Scenarios({have})"


def scenario_summary(final):
    """final (B,N) final wealths of N paths per start -> dict of (B,) fp64 tensors on its device: mean, std
    (unbiased), q05, q50, q95 (torch.quantile's linear interpolation) and prob_gain = P(final > 1).  NaN paths
    (failed starts) make their start's row NaN."""
    if not torch.is_tensor(final) or final.dim() != 2 or not final.dtype.is_floating_point:
        raise ValueError("scenario_summary: final must be a floating point tensor of shape (B, N)")
    f = final.detach().double()
    q = torch.quantile(f, torch.tensor([0.05, 0.5, 0.95], dtype=torch.float64, device=f.device), dim=1)
    gain = (f > 1).double().mean(1)
    gain = torch.where(torch.isnan(f).any(1), torch.full_like(gain, float("nan")), gain)
    return {"mean": f.mean(1), "std": f.std(1), "q05": q[0], "q50": q[1], "q95": q[2], "prob_gain": gain}


class GaussianHMM(torch.nn.Module):
    """HMM with `num_states` hidden states emitting `dim`-dimensional Gaussians, diagonal
    (covariance_type="diag", the default) or with a full covariance per state ("full").

    Parameters (fp32): log_pi (S,), log_A (S,S) with log_A[i,j] = log p(z_t=j | z_{t-1}=i) (natural logs; -inf
    entries are structural zeros that EM keeps), mean (S,D), and log_var (S,D) ("diag") or scale_tril (S,D,D)
    ("full": the lower Cholesky factor of each covariance, of which only the lower triangle is read).  They start
    random (from `generator`): pi and A row-normalised, means standard normal, unit (identity) covariances."""

    def __init__(self, num_states, dim, covariance_type="diag", generator=None):
        super().__init__()
        S, D = int(num_states), int(dim)
        if covariance_type not in ("diag", "full"):
            raise ValueError("GaussianHMM: covariance_type is 'diag' or 'full'")
        if not (1 <= S <= MAX_STATES and 1 <= D <= MAX_DIM):
            raise ValueError(f"GaussianHMM: 1 <= num_states <= {MAX_STATES} and 1 <= dim <= {MAX_DIM} "
                             f"(got {S}, {D})")
        self.full = covariance_type == "full"
        if self.full:
            _full_domain("GaussianHMM", S, D)
        self.covariance_type = covariance_type
        self.num_states, self.dim = S, D
        self.mixture = False

        def rows(*shape):
            w = torch.rand(*shape, generator=generator, dtype=torch.float64) + 0.5
            return torch.log(w / w.sum(-1, keepdim=True)).float()

        P = torch.nn.Parameter
        self.log_pi = P(rows(S), requires_grad=False)
        self.log_A = P(rows(S, S), requires_grad=False)
        self.mean = P(torch.randn(S, D, generator=generator, dtype=torch.float64).float(), requires_grad=False)
        if self.full:
            self.scale_tril = P(torch.eye(D).repeat(S, 1, 1), requires_grad=False)
        else:
            self.log_var = P(torch.zeros(S, D), requires_grad=False)

    # ------------------------------------------------------------------ inputs
    def _inputs(self, x, lengths):
        return _check_x("GaussianHMM", self.log_pi, x, lengths, self.dim)

    def _params(self):
        """The four tensors the kernels take: the last is log_var ("diag") or W = L^-1 ("full")."""
        last = _prec_chol(self.scale_tril) if self.full else self.log_var.detach().contiguous()
        return (self.log_pi.detach().contiguous(), self.log_A.detach().contiguous(),
                self.mean.detach().contiguous(), last)

    def _run(self, what, *args):
        """_estep / _estep_full(what, *args) by the covariance type."""
        return (_estep_full if self.full else _estep)(what, *args)

    @property
    def covariances(self):
        """Sigma (S,D,D) fp32: L L^T ("full") or diag(exp(log_var)) ("diag")."""
        if self.full:
            L = self.scale_tril.detach().double().tril()
            return (L @ L.transpose(1, 2)).float()
        return torch.diag_embed(torch.exp(self.log_var.detach()))

    @property
    def precisions_cholesky(self):
        """W (S,D,D) fp32, lower-triangular with Sigma^-1 = W^T W: what the full kernels are fed."""
        if self.full:
            return _prec_chol(self.scale_tril)
        return torch.diag_embed(torch.exp(-0.5 * self.log_var.detach().double()).float())

    def _shift(self, shift):
        if shift is None:
            return None
        shift = torch.as_tensor(shift).to(self.log_pi.device, torch.float32).contiguous()
        if shift.shape != (self.dim,):
            raise ValueError(f"GaussianHMM: shift must have shape ({self.dim},)")
        return shift

    def _weights(self, weights, B):
        if weights is None:
            return None
        weights = torch.as_tensor(weights).to(self.log_pi.device, torch.float32).contiguous()
        if weights.shape != (B,):
            raise ValueError(f"GaussianHMM: weights must have shape ({B},)")
        return weights

    # ------------------------------------------------------- emissions, E-step
    def emission_log_prob(self, x, lengths=None):
        """em (B,T,S) fp32: log N(x[b,t]; mean[s], diag exp(log_var[s])), -inf at t >= length
        (vqhmm_gauss_emission_f32); "full": log N(x[b,t]; mean[s], Sigma[s]) (vqhmm_gauss_full_emission_f32)."""
        x, lengths, B, T = self._inputs(x, lengths)
        S, D = self.num_states, self.dim
        em = torch.empty((B, T, S), dtype=torch.float32, device=x.device)
        _, _, mean, log_var = self._params()
        lib = _ext.load()
        entry = lib.vqhmm_gauss_full_emission_f32 if self.full else lib.vqhmm_gauss_emission_f32
        with torch.no_grad():
            _ext.check(entry(
                _ext.ptr(mean), _ext.ptr(log_var), _ext.ptr(x), _ext.ptr(lengths), B, T, S, D, _ext.ptr(em),
                _ext.stream_ptr(x.device)), "GaussianHMM.emission_log_prob")
        return em

    def e_step(self, x, lengths=None, weights=None, return_gamma=False, shift=None):
        """x (B,T,D), lengths (B,), weights (B,) -> dict(pi_cnt (S,), trans_cnt (S,S), occ (S,), m1 (S,D), m2
        (S,D) fp64, loglik (B,) fp32 [, gamma (B,T,S) fp32], shift).  m1 and m2 are the posterior-weighted sums
        of x - shift and (x - shift)^2 (shift (D,), None = 0).  `flat` is the one buffer the counts are views of
        (all-reduce it across ranks before m_step for data-parallel EM).  "full": m2 is (S,D,D), the sums of (x -
        shift)(x - shift)^T, exactly symmetric."""
        x, lengths, B, T = self._inputs(x, lengths)
        return self._run("GaussianHMM.e_step", *self._params(), x, lengths, self._shift(shift),
                         self._weights(weights, B), True, return_gamma)

    def log_prob(self, x, lengths=None):
        """log p(x[b, :lengths[b]]) (B,) fp32; NaN for length 0 or a non-finite x, -inf if impossible."""
        x, lengths, B, T = self._inputs(x, lengths)
        return self._run("GaussianHMM.log_prob", *self._params(), x, lengths, None, None, True, False)["loglik"]

    def posterior(self, x, lengths=None):
        """gamma (B,T,S) fp32: p(z_t = s | x[b, :lengths[b]]), rows at t >= length are 0."""
        x, lengths, B, T = self._inputs(x, lengths)
        return self._run("GaussianHMM.posterior", *self._params(), x, lengths, None, None, False, True)["gamma"]

    def predict(self, x, lengths=None):
        """The most probable state per position (argmax of gamma) (B,T) int64, -1 at t >= length."""
        x, lengths, B, T = self._inputs(x, lengths)
        g = self._run("GaussianHMM.predict", *self._params(), x, lengths, None, None, False, True)["gamma"]
        pad = torch.arange(T, device=x.device).unsqueeze(0) >= lengths.clamp(0, T).unsqueeze(1)
        return g.argmax(-1).masked_fill(pad, -1)

    # ------------------------------------------------------- decode and filter
    def decode(self, x, lengths=None):
        """MAP state path (Viterbi on x, vqhmm_gauss_viterbi_f32 / vqhmm_gauss_full_viterbi_f32) -> (path (B,T)
        int32 with -1 at t >= length, score (B,) fp32 = the path's log weight).  Length 0: score -inf; a
        non-finite x or emission inside the length: path all -1 and score NaN."""
        x, lengths, B, T = self._inputs(x, lengths)
        S, D = self.num_states, self.dim
        dev = x.device
        path = torch.empty((B, T), dtype=torch.int32, device=dev)
        score = torch.empty((B,), dtype=torch.float32, device=dev)
        lib = _ext.load()
        size, entry = ((lib.vqhmm_gauss_full_viterbi_workspace_size, lib.vqhmm_gauss_full_viterbi_f32) if self.full
                       else (lib.vqhmm_gauss_viterbi_workspace_size, lib.vqhmm_gauss_viterbi_f32))
        nb = size(B, T, S, D)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        with torch.no_grad():
            _ext.check(entry(*(_ext.ptr(p) for p in self._params()), _ext.ptr(x), _ext.ptr(lengths), B, T, S, D,
                             _ext.ptr(path), _ext.ptr(score), _ext.ptr(ws), nb, _ext.stream_ptr(dev)),
                       "GaussianHMM.decode")
        return path, score

    def backtest(self, x, returns, weights, lengths=None, causal=True, **kw):
        """Label the history with this model and run `weights` through it: vqhmm.backtest(returns, probs, weights,
        lengths, **kw) with probs = filter(x, lengths)[0] (causal=True: step t's row has seen x up to t only) or
        posterior(x, lengths) (causal=False: the smoother, which has seen the whole window, for attribution rather
        than for a tradable result).  x (B,T,dim) are the model's observations, returns (B,T,D) the assets' step
        returns; they may be the same tensor.  The equal-weight buy-and-hold benchmark is weights = 1 / D in every
        row with tx_cost = 0.  -> Backtest."""
        from .backtest import backtest
        with torch.no_grad():
            probs = self.filter(x, lengths)[0] if causal else self.posterior(x, lengths)
        return backtest(returns, probs, weights, lengths=lengths, **kw)

    def _filter(self, x, lengths, state, want_filt):
        x, lengths, B, T = self._inputs(x, lengths)
        S, D = self.num_states, self.dim
        dev = x.device
        if state is not None:
            if not torch.is_tensor(state) or state.shape != (B, S) or state.dtype != torch.float32:
                raise ValueError(f"GaussianHMM: state must be a ({B}, {S}) float32 tensor")
            _ext.require_device(state)
            state = state.contiguous()
        filt = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_filt else None
        last = torch.empty((B, S), dtype=torch.float32, device=dev)
        loglik = torch.empty((B,), dtype=torch.float32, device=dev)
        lib = _ext.load()
        entry = lib.vqhmm_gauss_full_filter_f32 if self.full else lib.vqhmm_gauss_filter_f32
        with torch.no_grad():
            _ext.check(entry(*(_ext.ptr(p) for p in self._params()), _ext.ptr(x), _ext.ptr(lengths), _ext.ptr(state),
                             B, T, S, D, _ext.ptr(filt), _ext.ptr(last), _ext.ptr(loglik), _ext.stream_ptr(dev)),
                       "GaussianHMM.filter")
        return filt, last, loglik

    def filter(self, x, lengths=None, state=None, return_state=False):
        """Causal filter (vqhmm_gauss_filter_f32 / vqhmm_gauss_full_filter_f32): filt (B,T,S) fp32 with filt[b,t] =
        p(z_t | x[b, :t+1]) (no look-ahead; rows at t >= length are 0) and loglik (B,) = log p(x[b, :length] |
        state).  `state` (B,S) fp32 is the carry of the previous chunk (None: the sequence starts from log_pi);
        with return_state the new carry filt[b, length-1] is returned too, and feeding it back gives what one
        call on the concatenated observations gives.  loglik is NaN for length 0 (the carry then passes
        through)."""
        filt, last, loglik = self._filter(x, lengths, state, True)
        return (filt, loglik, last) if return_state else (filt, loglik)

    def update(self, x, lengths=None, state=None):
        """The streaming form of `filter`: -> (state (B,S), loglik (B,)) without writing filt."""
        _, last, loglik = self._filter(x, lengths, state, False)
        return last, loglik

    @torch.no_grad()
    def predict_next(self, state):
        """The next observation's predictive regime distribution, mean and covariance from a filtered state (B,S)
        -> (probs (B,S), mean (B,D), cov (B,D,D)) fp32: probs = normalise(state exp(log_A)), mean = probs . mu,
        cov = sum_s probs_s (Sigma_s + mu_s mu_s^T) - mean mean^T, in fp64 on the device."""
        S = self.num_states
        if not torch.is_tensor(state) or state.dim() != 2 or state.shape[1] != S or state.dtype != torch.float32:
            raise ValueError(f"GaussianHMM: state must be a (B, {S}) float32 tensor")
        _ext.require_device(self.log_pi, state)
        nxt = state.double() @ torch.exp(self.log_A.detach().double())
        probs = nxt / nxt.sum(-1, keepdim=True)
        mu = self.mean.detach().double()
        if self.full:
            L = self.scale_tril.detach().double().tril()
            sigma = L @ L.transpose(1, 2)
        else:
            sigma = torch.diag_embed(torch.exp(self.log_var.detach().double()))
        mean = probs @ mu
        second = (sigma + mu[:, :, None] * mu[:, None, :]).reshape(S, -1)
        cov = (probs @ second).view(-1, self.dim, self.dim) - mean[:, :, None] * mean[:, None, :]
        return probs.float(), mean.float(), cov.float()

    # ----------------------------------------------------------------- M-step
    @torch.no_grad()
    def as_mixture(self):
        """Tie every row of A to pi: the model becomes a diagonal Gaussian mixture over positions, and m_step
        keeps it one (pi from the occupancies).  Returns self."""
        self.mixture = True
        self.log_A.copy_(self.log_pi.unsqueeze(0).expand_as(self.log_A))
        return self

    @torch.no_grad()
    def m_step(self, counts, prior_count=0.0, var_floor=None, reg_covar=None):
        """Parameters <- the counts' maximiser, in fp64 on the device.  pi and A: row-normalised (counts +
        prior_count), structural zeros kept, a row nothing was counted into keeps its parameters (as CodeHMM).
        mean = shift + m1 / occ, var = max(m2 / occ - (m1 / occ)^2, var_floor); a state with occ = 0 keeps its
        mean and log_var.  counts["shift"] (None = 0) is the shift its m1 and m2 were taken about.
        "full": Sigma = m2 / occ - mu mu^T + reg_covar I with mu = m1 / occ (sklearn's regulariser; the third
        argument is reg_covar), scale_tril = its Cholesky factor; a state with occ = 0, or whose factorisation
        fails, keeps its mean and scale_tril.  Both default to 1e-6."""
        if self.full:
            reg = reg_covar if reg_covar is not None else (1e-6 if var_floor is None else var_floor)
            return self._m_step_full(counts, prior_count, float(reg))
        var_floor = 1e-6 if var_floor is None else var_floor
        occ = counts["occ"].to(torch.float64)
        if self.mixture:
            self.log_pi.copy_(CodeHMM._m_rows(occ, self.log_pi, prior_count))
            self.log_A.copy_(self.log_pi.unsqueeze(0).expand_as(self.log_A))
        else:
            self.log_pi.copy_(CodeHMM._m_rows(counts["pi_cnt"], self.log_pi, prior_count))
            self.log_A.copy_(CodeHMM._m_rows(counts["trans_cnt"], self.log_A, prior_count))
        live = (occ > 0).unsqueeze(1)
        o = torch.where(occ > 0, occ, torch.ones_like(occ)).unsqueeze(1)
        mu = counts["m1"].to(torch.float64) / o
        var = (counts["m2"].to(torch.float64) / o - mu * mu).clamp_min(float(var_floor))
        shift = counts.get("shift")
        if shift is not None:
            mu = mu + torch.as_tensor(shift).to(mu.device, torch.float64)
        self.mean.copy_(torch.where(live, mu, self.mean.double()).float())
        self.log_var.copy_(torch.where(live, torch.log(var), self.log_var.double()).float())

    def _m_step_full(self, counts, prior_count, reg_covar):
        occ = counts["occ"].to(torch.float64)
        if self.mixture:
            self.log_pi.copy_(CodeHMM._m_rows(occ, self.log_pi, prior_count))
            self.log_A.copy_(self.log_pi.unsqueeze(0).expand_as(self.log_A))
        else:
            self.log_pi.copy_(CodeHMM._m_rows(counts["pi_cnt"], self.log_pi, prior_count))
            self.log_A.copy_(CodeHMM._m_rows(counts["trans_cnt"], self.log_A, prior_count))
        D = self.dim
        o = torch.where(occ > 0, occ, torch.ones_like(occ))
        mu = counts["m1"].to(torch.float64) / o[:, None]
        cov = counts["m2"].to(torch.float64) / o[:, None, None] - mu[:, :, None] * mu[:, None, :]
        cov = cov + reg_covar * torch.eye(D, dtype=torch.float64, device=cov.device)
        old = self.scale_tril.double().tril()
        # a state that keeps its parameters is factored from its own covariance (always possible)
        safe = torch.where((occ > 0)[:, None, None], cov, old @ old.transpose(1, 2))
        L, ok = _cholesky(torch.where(torch.isfinite(safe), safe, torch.zeros_like(safe)))
        ok = ok & (occ > 0) & torch.isfinite(cov).all((-1, -2))
        shift = counts.get("shift")
        if shift is not None:
            mu = mu + torch.as_tensor(shift).to(mu.device, torch.float64)
        self.mean.copy_(torch.where(ok[:, None], mu, self.mean.double()).float())
        self.scale_tril.copy_(torch.where(ok[:, None, None], L.tril(), old).float())

    @torch.no_grad()
    def init_kmeans(self, x, lengths=None, n_iter=10, generator=None):
        """Means from Lloyd's algorithm on the counted positions (Codebook.fit_kmeans), one shared variance from
        the final distortion (Codebook.stats' squared error / (D * counted positions)); pi and A are not
        touched."""
        x, lengths, B, T = self._inputs(x, lengths)
        S, D = self.num_states, self.dim
        cb = Codebook(S, D).to(x.device)   # its rows are seeded from the data by fit_kmeans
        z = x.transpose(1, 2).contiguous()
        cb.fit_kmeans(z, lengths, n_iter=n_iter, generator=generator)
        st = cb.stats(z, None, lengths)
        n = lengths.clamp(0, T).sum().clamp_min(1).double()
        var = (st["sse"] / (D * n)).clamp_min(1e-6)
        self.mean.copy_(cb.weight.detach().float())
        if self.full:   # the same shared spherical covariance
            self.scale_tril.copy_((torch.sqrt(var) * torch.eye(D, dtype=torch.float64, device=x.device))
                                  .float().expand(S, D, D))
        else:
            self.log_var.copy_(torch.log(var).float().expand(S, D))

    @torch.no_grad()
    def _restart_ensemble(self, n_init, x, lengths, generator=None):
        """The starts of fit(n_init=R): member 0 = the current parameters; members 1..R-1 = pi and A as
        GaussianHMM(S, D, covariance_type, generator) draws them, in that order, with this model's structural zeros
        imposed and the rows renormalised (a mixture's rows of A tied to its pi), means at S distinct counted
        positions of x (Codebook's draw with `generator`) and one shared per-dimension variance, the data's."""
        from .gauss_hmm_ensemble import GaussianHMMEnsemble
        S, D = self.num_states, self.dim
        dev = x.device
        T = x.shape[1]
        mask = (torch.arange(T, device=dev).unsqueeze(0) < lengths.clamp(0, T).unsqueeze(1)).unsqueeze(2)
        n = mask.sum().clamp_min(1)
        xd = x.double()
        mu = torch.where(mask, xd, 0.0).sum((0, 1)) / n
        var = (torch.where(mask, (xd - mu) ** 2, 0.0).sum((0, 1)) / n).clamp_min(1e-6)
        z = x.transpose(1, 2).contiguous()
        starts = [self]
        for _ in range(int(n_init) - 1):
            h = GaussianHMM(S, D, self.covariance_type, generator=generator).to(dev)
            h.mixture = self.mixture
            for k in ("log_pi", "log_A"):
                new = torch.where(getattr(self, k) != float("-inf"), getattr(h, k).double(), float("-inf"))
                lse = torch.logsumexp(new, -1, keepdim=True)
                getattr(h, k).copy_(torch.where(lse != float("-inf"), new - lse, new).float())
            if self.mixture:
                h.log_A.copy_(h.log_pi.unsqueeze(0).expand_as(h.log_A))
            h.mean.copy_(Codebook(S, D).to(dev)._pick(z, lengths, S, generator))
            if self.full:
                h.scale_tril.copy_(torch.diag(torch.sqrt(var)).float().expand(S, D, D))
            else:
                h.log_var.copy_(torch.log(var).float().expand(S, D))
            starts.append(h)
        return GaussianHMMEnsemble.from_models(starts)

    def fit(self, x, lengths=None, n_iter=20, tol=None, prior_count=0.0, var_floor=None, init="kmeans",
            mixture=False, generator=None, reg_covar=None, n_init=1):
        """Baum-Welch: alternate e_step and m_step.  Returns the total log-likelihoods, one per iteration, each
        under the parameters before that iteration's M-step (0-dim device tensors with tol=None, so the loop has
        no host sync; floats with tol, which stops once the improvement per observed position is < tol).
        init="kmeans" first runs init_kmeans, init=None starts from the current parameters.  The moments are
        taken about the data mean (computed once).  mixture=True fits the Gaussian mixture (as_mixture).
        var_floor ("diag") and reg_covar ("full") are m_step's, 1e-6 by default.

        n_init = R > 1: R chains in one batched E-step per iteration (GaussianHMMEnsemble): member 0 starts where
        the plain fit would (after init_kmeans, or from the current parameters with init=None), members 1..R-1
        from the random starts of _restart_ensemble, drawn from `generator`.  The member with the largest total
        log-likelihood under its final parameters (one more batched E-step) is copied into this model, selected
        on the device; the history returned is that member's.  No host sync; `tol` cannot be combined with it."""
        if init not in ("kmeans", None):
            raise ValueError("GaussianHMM.fit: init is 'kmeans' or None")
        n_init = int(n_init)
        if n_init < 1:
            raise ValueError("GaussianHMM.fit: n_init >= 1")
        if n_init > 1 and tol is not None:
            raise ValueError("GaussianHMM.fit: tol needs a host sync per iteration and cannot be combined with "
                             "n_init > 1")
        x, lengths, B, T = self._inputs(x, lengths)
        if mixture:
            self.as_mixture()
        if init == "kmeans":
            self.init_kmeans(x, lengths, generator=generator)
        if n_init > 1:
            ens = self._restart_ensemble(n_init, x, lengths, generator)
            hist = ens.fit(x, lengths, n_iter=n_iter, prior_count=prior_count, var_floor=var_floor,
                           reg_covar=reg_covar)
            best = ens.best_index(x, lengths)
            with torch.no_grad():
                for k in ("log_pi", "log_A", "mean", "scale_tril" if self.full else "log_var"):
                    getattr(self, k).copy_(getattr(ens, k).index_select(0, best)[0])
            return list(hist.index_select(1, best)[:, 0].unbind(0))
        mask = (torch.arange(T, device=x.device).unsqueeze(0) < lengths.clamp(0, T).unsqueeze(1)).unsqueeze(2)
        npos_t = mask.sum().clamp_min(1)
        shift = (torch.where(mask, x.double(), 0.0).sum((0, 1)) / npos_t).float().contiguous()
        npos = None
        history = []
        for _ in range(int(n_iter)):
            st = self._run("GaussianHMM.fit", *self._params(), x, lengths, shift, None, True, False)
            total = st["loglik"].double().nansum()
            self.m_step(st, prior_count, var_floor, reg_covar)
            if tol is None:
                history.append(total)
                continue
            if npos is None:
                npos = max(int(npos_t.item()), 1)
            total = float(total.item())
            if history and (total - history[-1]) / npos < tol:
                history.append(total)
                break
            history.append(total)
        return history

    # ------------------------------------------------------ moments and samples
    @torch.no_grad()
    def mean_path(self, T):
        """E[x_t] for t < T, (T, D) fp64 on the host: (pi A^t) mean of the row-normalised model."""
        pi = torch.exp(self.log_pi.detach().double().cpu())
        A = torch.exp(self.log_A.detach().double().cpu())
        pi, A = pi / pi.sum(), A / A.sum(1, keepdim=True)
        ps = torch.empty((int(T), self.num_states), dtype=torch.float64)
        for t in range(int(T)):
            ps[t] = pi if t == 0 else ps[t - 1] @ A
        return ps @ self.mean.detach().double().cpu()

    def sample(self, n, seq_len, generator=None):
        """Ancestral samples -> (states (n, seq_len) int64, x (n, seq_len, D) fp32): the states by inverse CDF from
        torch.rand((n, seq_len), generator=generator), x = mean + exp(log_var / 2) * torch.randn((n, seq_len, D),
        generator=generator), both drawn on the model's device.  "full": the same state draw, then x = mean[z] +
        scale_tril[z] . normal in torch (one masked matmul per state)."""
        _ext.require_device(self.log_pi)
        n, seq_len = int(n), int(seq_len)
        S, D = self.num_states, self.dim
        dev = self.log_pi.device
        u = torch.rand((n, seq_len), generator=generator, device=dev, dtype=torch.float32)
        nr = torch.randn((n, seq_len, D), generator=generator, device=dev, dtype=torch.float32)
        states = torch.empty((n, seq_len), dtype=torch.int32, device=dev)
        x = torch.empty((n, seq_len, D), dtype=torch.float32, device=dev)
        params = self._params()
        if self.full:   # the kernel draws the states (its unit-variance x is replaced below)
            params = params[:3] + (torch.zeros((S, D), dtype=torch.float32, device=dev),)
        with torch.no_grad():
            _ext.check(_ext.load().vqhmm_gauss_sample_f32(
                *(_ext.ptr(p) for p in params), _ext.ptr(u), _ext.ptr(nr), n, seq_len, S, D,
                _ext.ptr(states), _ext.ptr(x), _ext.stream_ptr(dev)), "GaussianHMM.sample")
            if self.full:
                L = self.scale_tril.detach().tril()
                x = self.mean.detach()[states.long()]
                for s in range(S):
                    x = x + (states == s).unsqueeze(-1) * (nr @ L[s].T)
        return states.long(), x

    @torch.no_grad()
    def simulate(self, horizon, n_paths, state=None, seed=0, weights=None, rebalance=1, tx_cost=0.0, return_x=False,
                 return_states=False, return_wealth=False, start_offset=0, path_offset=0):
        """Monte Carlo scenarios (vqhmm_gauss_scenario_f32, random numbers generated on chip): n_paths paths of
        `horizon` steps from each of B starts -> Scenarios(final (B,N), drawdown (B,N), wealth (B,N,H), states
        (B,N,H) int32, x (B,N,H,D)); what was not asked for is None.  `state` (B,S) fp32 is a filtered carry of
        `filter` / `update`: simulated step 0 is the next observation, its regime drawn from predict_next(state)'s
        probs; state=None: one start from exp(log_pi).  `weights` (S,D): the holdings taken when a rebalance (every
        `rebalance` steps, from step 0) finds the path in that regime, at a cost of tx_cost per unit of turnover;
        with weights, final wealth (start 1) and the maximum drawdown are returned, and with return_wealth the
        whole wealth path.  Path (b, n) is path (start_offset + b, path_offset + n) of the seed's stream, so a
        call on a slice of the starts or paths returns the full call's rows bit for bit.  Raises if nothing is
        requested (no weights and neither return_x nor return_states)."""
        _ext.require_device(self.log_pi)
        H, N = int(horizon), int(n_paths)
        S, D = self.num_states, self.dim
        dev = self.log_pi.device
        if H < 0 or N < 0:
            raise ValueError("GaussianHMM.simulate: horizon and n_paths must be >= 0")
        if weights is None and (return_wealth or not (return_x or return_states)):
            raise ValueError("GaussianHMM.simulate: nothing to compute: pass weights (S, D) for final / drawdown / "
                             "wealth, or ask for return_x / return_states")
        if state is None:
            start = torch.exp(self.log_pi.detach().double()).float().unsqueeze(0).contiguous()
        else:
            start = self.predict_next(state)[0].contiguous()
        B = int(start.shape[0])
        port = None
        if weights is not None:
            port = torch.as_tensor(weights).to(dev, torch.float32).contiguous()
            if port.shape != (S, D):
                raise ValueError(f"GaussianHMM.simulate: weights must have shape ({S}, {D})")
        if self.full:
            scale = self.scale_tril.detach().contiguous()
        else:   # as the sampler: exp(log_var / 2) in fp64, rounded once
            scale = torch.exp(0.5 * self.log_var.detach().double()).float().contiguous()

        def buf(want, shape, dtype=torch.float32):
            return torch.empty(shape, dtype=dtype, device=dev) if want else None

        res = Scenarios(final=buf(port is not None, (B, N)), drawdown=buf(port is not None, (B, N)),
                        wealth=buf(return_wealth, (B, N, H)), states=buf(return_states, (B, N, H), torch.int32),
                        x=buf(return_x, (B, N, H, D)))
        _ext.check(_ext.load().vqhmm_gauss_scenario_f32(
            _ext.ptr(start), _ext.ptr(self.log_A.detach().contiguous()), _ext.ptr(self.mean.detach().contiguous()),
            _ext.ptr(scale), int(self.full), _ext.ptr(port), int(rebalance), float(tx_cost),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(start_offset), int(path_offset), B, N, H, S, D, _ext.ptr(res.states),
            _ext.ptr(res.x), _ext.ptr(res.wealth), _ext.ptr(res.final), _ext.ptr(res.drawdown),
            _ext.stream_ptr(dev)), "GaussianHMM.simulate")
        return res
