"""Stationary HMM with diagonal-Gaussian emissions on continuous observations (returns, the `u` features,
encoder latents): Baum-Welch EM, scoring, posteriors and ancestral sampling.  HIP only: the emission
log-densities, the fused E-step and the sampler are the kernels of hmm_gauss.hip (vqhmm_gauss_emission_f32 /
vqhmm_gauss_estep_f32 / vqhmm_gauss_sample_f32, contracts in include/vqhmm.h); the M-step is S*S + 2*S*D numbers
of torch arithmetic in fp64 on the device.  With every row of A tied to pi (`as_mixture`, `fit(mixture=True)`)
the model is a diagonal Gaussian mixture.  `gauss_log_prob` is the differentiable log-likelihood (its backward
is one weighted E-step).
"""
import torch

from . import _ext
from .codebook import Codebook
from .codehmm import CodeHMM

MAX_STATES = 32   # the kernels' limits (hmm_gauss.hip)
MAX_DIM = 64


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


class GaussianHMM(torch.nn.Module):
    """HMM with `num_states` hidden states emitting `dim`-dimensional diagonal Gaussians.

    Parameters (fp32): log_pi (S,), log_A (S,S) with log_A[i,j] = log p(z_t=j | z_{t-1}=i) (natural logs; -inf
    entries are structural zeros that EM keeps), mean (S,D), log_var (S,D).  They start random (from
    `generator`): pi and A row-normalised, means standard normal, unit variances."""

    def __init__(self, num_states, dim, generator=None):
        super().__init__()
        S, D = int(num_states), int(dim)
        if not (1 <= S <= MAX_STATES and 1 <= D <= MAX_DIM):
            raise ValueError(f"GaussianHMM: 1 <= num_states <= {MAX_STATES} and 1 <= dim <= {MAX_DIM} "
                             f"(got {S}, {D})")
        self.num_states, self.dim = S, D
        self.mixture = False

        def rows(*shape):
            w = torch.rand(*shape, generator=generator, dtype=torch.float64) + 0.5
            return torch.log(w / w.sum(-1, keepdim=True)).float()

        P = torch.nn.Parameter
        self.log_pi = P(rows(S), requires_grad=False)
        self.log_A = P(rows(S, S), requires_grad=False)
        self.mean = P(torch.randn(S, D, generator=generator, dtype=torch.float64).float(), requires_grad=False)
        self.log_var = P(torch.zeros(S, D), requires_grad=False)

    # ------------------------------------------------------------------ inputs
    def _inputs(self, x, lengths):
        return _check_x("GaussianHMM", self.log_pi, x, lengths, self.dim)

    def _params(self):
        return (self.log_pi.detach().contiguous(), self.log_A.detach().contiguous(),
                self.mean.detach().contiguous(), self.log_var.detach().contiguous())

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
        (vqhmm_gauss_emission_f32)."""
        x, lengths, B, T = self._inputs(x, lengths)
        S, D = self.num_states, self.dim
        em = torch.empty((B, T, S), dtype=torch.float32, device=x.device)
        _, _, mean, log_var = self._params()
        with torch.no_grad():
            _ext.check(_ext.load().vqhmm_gauss_emission_f32(
                _ext.ptr(mean), _ext.ptr(log_var), _ext.ptr(x), _ext.ptr(lengths), B, T, S, D, _ext.ptr(em),
                _ext.stream_ptr(x.device)), "GaussianHMM.emission_log_prob")
        return em

    def e_step(self, x, lengths=None, weights=None, return_gamma=False, shift=None):
        """x (B,T,D), lengths (B,), weights (B,) -> dict(pi_cnt (S,), trans_cnt (S,S), occ (S,), m1 (S,D), m2
        (S,D) fp64, loglik (B,) fp32 [, gamma (B,T,S) fp32], shift).  m1 and m2 are the posterior-weighted sums
        of x - shift and (x - shift)^2 (shift (D,), None = 0).  `flat` is the one buffer the counts are views of
        (all-reduce it across ranks before m_step for data-parallel EM)."""
        x, lengths, B, T = self._inputs(x, lengths)
        return _estep("GaussianHMM.e_step", *self._params(), x, lengths, self._shift(shift),
                      self._weights(weights, B), True, return_gamma)

    def log_prob(self, x, lengths=None):
        """log p(x[b, :lengths[b]]) (B,) fp32; NaN for length 0 or a non-finite x, -inf if impossible."""
        x, lengths, B, T = self._inputs(x, lengths)
        return _estep("GaussianHMM.log_prob", *self._params(), x, lengths, None, None, True, False)["loglik"]

    def posterior(self, x, lengths=None):
        """gamma (B,T,S) fp32: p(z_t = s | x[b, :lengths[b]]), rows at t >= length are 0."""
        x, lengths, B, T = self._inputs(x, lengths)
        return _estep("GaussianHMM.posterior", *self._params(), x, lengths, None, None, False, True)["gamma"]

    def predict(self, x, lengths=None):
        """The most probable state per position (argmax of gamma) (B,T) int64, -1 at t >= length."""
        x, lengths, B, T = self._inputs(x, lengths)
        g = _estep("GaussianHMM.predict", *self._params(), x, lengths, None, None, False, True)["gamma"]
        pad = torch.arange(T, device=x.device).unsqueeze(0) >= lengths.clamp(0, T).unsqueeze(1)
        return g.argmax(-1).masked_fill(pad, -1)

    # ----------------------------------------------------------------- M-step
    @torch.no_grad()
    def as_mixture(self):
        """Tie every row of A to pi: the model becomes a diagonal Gaussian mixture over positions, and m_step
        keeps it one (pi from the occupancies).  Returns self."""
        self.mixture = True
        self.log_A.copy_(self.log_pi.unsqueeze(0).expand_as(self.log_A))
        return self

    @torch.no_grad()
    def m_step(self, counts, prior_count=0.0, var_floor=1e-6):
        """Parameters <- the counts' maximiser, in fp64 on the device.  pi and A: row-normalised (counts +
        prior_count), structural zeros kept, a row nothing was counted into keeps its parameters (as CodeHMM).
        mean = shift + m1 / occ, var = max(m2 / occ - (m1 / occ)^2, var_floor); a state with occ = 0 keeps its
        mean and log_var.  counts["shift"] (None = 0) is the shift its m1 and m2 were taken about."""
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
        self.log_var.copy_(torch.log(var).float().expand(S, D))

    def fit(self, x, lengths=None, n_iter=20, tol=None, prior_count=0.0, var_floor=1e-6, init="kmeans",
            mixture=False, generator=None):
        """Baum-Welch: alternate e_step and m_step.  Returns the total log-likelihoods, one per iteration, each
        under the parameters before that iteration's M-step (0-dim device tensors with tol=None, so the loop has
        no host sync; floats with tol, which stops once the improvement per observed position is < tol).
        init="kmeans" first runs init_kmeans, init=None starts from the current parameters.  The moments are
        taken about the data mean (computed once).  mixture=True fits the Gaussian mixture (as_mixture)."""
        if init not in ("kmeans", None):
            raise ValueError("GaussianHMM.fit: init is 'kmeans' or None")
        x, lengths, B, T = self._inputs(x, lengths)
        if mixture:
            self.as_mixture()
        if init == "kmeans":
            self.init_kmeans(x, lengths, generator=generator)
        mask = (torch.arange(T, device=x.device).unsqueeze(0) < lengths.clamp(0, T).unsqueeze(1)).unsqueeze(2)
        npos_t = mask.sum().clamp_min(1)
        shift = (torch.where(mask, x.double(), 0.0).sum((0, 1)) / npos_t).float().contiguous()
        npos = None
        history = []
        for _ in range(int(n_iter)):
            st = _estep("GaussianHMM.fit", *self._params(), x, lengths, shift, None, True, False)
            total = st["loglik"].double().nansum()
            self.m_step(st, prior_count, var_floor)
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
        generator=generator), both drawn on the model's device."""
        _ext.require_device(self.log_pi)
        n, seq_len = int(n), int(seq_len)
        S, D = self.num_states, self.dim
        dev = self.log_pi.device
        u = torch.rand((n, seq_len), generator=generator, device=dev, dtype=torch.float32)
        nr = torch.randn((n, seq_len, D), generator=generator, device=dev, dtype=torch.float32)
        states = torch.empty((n, seq_len), dtype=torch.int32, device=dev)
        x = torch.empty((n, seq_len, D), dtype=torch.float32, device=dev)
        with torch.no_grad():
            _ext.check(_ext.load().vqhmm_gauss_sample_f32(
                *(_ext.ptr(p) for p in self._params()), _ext.ptr(u), _ext.ptr(nr), n, seq_len, S, D,
                _ext.ptr(states), _ext.ptr(x), _ext.stream_ptr(dev)), "GaussianHMM.sample")
        return states.long(), x
