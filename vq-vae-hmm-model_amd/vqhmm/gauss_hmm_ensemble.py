"""A stack of M Gaussian HMMs on the same continuous observations fitted together: EM restarts, members of
different state counts (model selection by BIC), and a mixture of Gaussian HMMs over sequences.  Every E-step is
one call of vqhmm_gauss_estep_batched_f32 / vqhmm_gauss_full_estep_batched_f32 (hmm_gauss.hip,
hmm_gauss_full.hip): the member is a grid dimension of GaussianHMM's fused kernel, so M models cost two launches,
and member m's counts, loglik and gamma are bit-identical to `GaussianHMM.e_step` on member m.  The M-step is
GaussianHMM's applied along the stacked tensors in fp64 on the device ("full": one batched Cholesky).  decode /
filter / sample stay on GaussianHMM: `member(m)` or `best()` hands one over.
"""
import math

import torch

from . import _ext
from .codehmm import CodeHMM
from .gauss_hmm import GaussianHMM, _check_x, _cholesky, _estep_members, _prec_chol

NEG_INF = float("-inf")


class GaussianHMMEnsemble(torch.nn.Module):
    """M Gaussian HMMs over the same `dim`-dimensional observations, all "diag" or all "full".

    Buffers (fp32): log_pi (M,S), log_A (M,S,S), mean (M,S,D), log_var (M,S,D) ("diag") or scale_tril (M,S,D,D)
    ("full"), and log_mix (M,), the mixture weights `fit_mixture` learns (uniform at the start).  `mixture` (every
    row of A tied to pi: Gaussian mixtures over positions) is shared by the members.  `num_states` is an int (every
    member has S states; `num_models` of them) or a sequence with one entry per member; S is the largest.  A member
    with S_m < S is the padded larger model: log_pi[m, S_m:] = -inf and log_A[m] = -inf wherever the row or the
    column is >= S_m, which EM keeps.  The chain shifts every step by the largest emission over all S states and a
    non-finite emission voids the sequence, so a padded state always carries a copy of the member's state 0 (mean
    and log_var / scale_tril): valid, and never above the live maximum.  `m_step` re-copies it.  The padded state
    is unreachable: its gamma and occupancy are exactly 0.  Each member starts as GaussianHMM(S_m, D,
    covariance_type, generator) does, in member order.

    `max_workspace_bytes` (default 1 GiB, an engineering default) caps the E-step's workspace, which is M
    single-model workspaces (4 S bytes per position and member): the members then run in groups that fit, with
    the same bits."""

    def __init__(self, num_models=None, num_states=None, dim=None, covariance_type="diag", generator=None,
                 max_workspace_bytes=1 << 30):
        super().__init__()
        if num_states is None or dim is None:
            raise ValueError("GaussianHMMEnsemble: num_states and dim are required")
        if isinstance(num_states, (list, tuple)):
            sizes = [int(s) for s in num_states]
            if num_models is not None and int(num_models) != len(sizes):
                raise ValueError("GaussianHMMEnsemble: num_models does not match len(num_states)")
        else:
            if num_models is None:
                raise ValueError("GaussianHMMEnsemble: num_models is required with an integer num_states")
            sizes = [int(num_states)] * int(num_models)
        if not 1 <= len(sizes) <= 65535:
            raise ValueError(f"GaussianHMMEnsemble: 1 <= num_models <= 65535 (got {len(sizes)})")
        self._setup([GaussianHMM(s, dim, covariance_type, generator=generator) for s in sizes], max_workspace_bytes)

    def _setup(self, models, max_workspace_bytes):
        D, full, mixture = models[0].dim, models[0].full, models[0].mixture
        if any(h.dim != D or h.full != full or h.mixture != mixture for h in models):
            raise ValueError("GaussianHMMEnsemble: the members must share dim, covariance_type and mixture")
        self.member_states = [h.num_states for h in models]
        M, S = len(models), max(self.member_states)
        if full and S * D * D > 8192:
            raise ValueError(f"GaussianHMMEnsemble: full covariances need S * D * D <= 8192 (got {S}, {D})")
        self.num_models, self.num_states, self.dim = M, S, D
        self.full, self.covariance_type, self.mixture = full, models[0].covariance_type, mixture
        self.max_workspace_bytes = int(max_workspace_bytes)
        dev = models[0].log_pi.device
        log_pi = torch.full((M, S), NEG_INF, dtype=torch.float32, device=dev)
        log_A = torch.full((M, S, S), NEG_INF, dtype=torch.float32, device=dev)
        mean = torch.zeros((M, S, D), dtype=torch.float32, device=dev)
        last = torch.zeros((M, S, D, D) if full else (M, S, D), dtype=torch.float32, device=dev)
        for m, h in enumerate(models):
            s = h.num_states
            log_pi[m, :s] = h.log_pi.detach().to(dev)
            log_A[m, :s, :s] = h.log_A.detach().to(dev)
            mean[m, :s] = h.mean.detach().to(dev)
            last[m, :s] = (h.scale_tril.detach().tril() if full else h.log_var.detach()).to(dev)
        pad = torch.tensor([[s >= sm for s in range(S)] for sm in self.member_states], dtype=torch.bool, device=dev)
        self.register_buffer("log_pi", log_pi)
        self.register_buffer("log_A", log_A)
        self.register_buffer("mean", mean)
        self.register_buffer("scale_tril" if full else "log_var", last)
        self.register_buffer("log_mix", torch.full((M,), -math.log(M), dtype=torch.float32, device=dev))
        self.register_buffer("pad", pad)
        self._copy_padding()

    @classmethod
    def from_models(cls, models, max_workspace_bytes=1 << 30):
        """An ensemble of copies of the given GaussianHMMs (same dim, covariance_type and mixture flag; S padded
        to the largest), on the first one's device."""
        models = list(models)
        if not 1 <= len(models) <= 65535 or not all(isinstance(h, GaussianHMM) for h in models):
            raise ValueError("GaussianHMMEnsemble.from_models: a non-empty sequence of GaussianHMM")
        self = cls.__new__(cls)
        torch.nn.Module.__init__(self)
        self._setup(models, max_workspace_bytes)
        return self

    @property
    def _last(self):
        return self.scale_tril if self.full else self.log_var

    @torch.no_grad()
    def _copy_padding(self):
        """A padded state's emission parameters <- the member's state 0."""
        pad = self.pad
        self.mean.copy_(torch.where(pad[:, :, None], self.mean[:, :1], self.mean))
        last = self._last
        p = pad[:, :, None, None] if self.full else pad[:, :, None]
        last.copy_(torch.where(p, last[:, :1], last))

    # ----------------------------------------------------------------- E-step
    def _inputs(self, x, lengths):
        return _check_x("GaussianHMMEnsemble", self.log_pi, x, lengths, self.dim)

    def _params(self):
        """The four stacked tensors the kernels take: the last is log_var ("diag") or W = L^-1 ("full")."""
        if self.full:
            M, S, D = self.num_models, self.num_states, self.dim
            last = _prec_chol(self.scale_tril.view(M * S, D, D)).view(M, S, D, D)
        else:
            last = self.log_var
        return self.log_pi, self.log_A, self.mean, last

    def _shift(self, shift):
        if shift is None:
            return None
        shift = torch.as_tensor(shift).to(self.log_pi.device, torch.float32).contiguous()
        if shift.shape != (self.dim,):
            raise ValueError(f"GaussianHMMEnsemble: shift must have shape ({self.dim},)")
        return shift

    def _weights(self, weights, B):
        if weights is None:
            return None
        M = self.num_models
        if not torch.is_tensor(weights) or weights.dtype != torch.float32 or tuple(weights.shape) not in ((M, B), (B,)):
            raise ValueError(f"GaussianHMMEnsemble: weights must be a float32 tensor of shape ({M}, {B}) or ({B},)")
        _ext.require_device(weights)
        return (weights.expand(M, B) if weights.dim() == 1 else weights).contiguous()

    def _loglik(self, what, x, lengths):
        return _estep_members(what, self.full, *self._params(), x, lengths, None, None, True, False,
                              self.max_workspace_bytes)[5]

    def _estep(self, x, lengths, shift, weights, want_loglik, want_gamma):
        M, S, D = self.num_models, self.num_states, self.dim
        pi, tr, occ, m1, m2, ll, gm = _estep_members("GaussianHMMEnsemble.e_step", self.full, *self._params(), x,
                                                     lengths, shift, weights, want_loglik, want_gamma,
                                                     self.max_workspace_bytes)
        # one (M, 2 S + S*S + S*D + |m2|) buffer the five counts are views of: what data-parallel EM all-reduces
        flat = torch.cat((pi, tr.view(M, S * S), occ, m1.view(M, S * D), m2.view(M, -1)), 1)
        o = [0, S, S + S * S, 2 * S + S * S, 2 * S + S * S + S * D]
        out = {"pi_cnt": flat[:, o[0]:o[1]], "trans_cnt": flat[:, o[1]:o[2]].view(M, S, S), "occ": flat[:, o[2]:o[3]],
               "m1": flat[:, o[3]:o[4]].view(M, S, D),
               "m2": flat[:, o[4]:].view((M, S, D, D) if self.full else (M, S, D)), "flat": flat, "shift": shift}
        if want_loglik:
            out["loglik"] = ll
        if want_gamma:
            out["gamma"] = gm
        return out

    def e_step(self, x, lengths=None, weights=None, return_gamma=False, shift=None):
        """x (B,T,D) and lengths (B,), shared by all members; weights (M,B) or (B,) (broadcast) float32 device
        tensor, None = all 1; shift (D,), None = 0 -> dict(pi_cnt (M,S), trans_cnt (M,S,S), occ (M,S), m1 (M,S,D), m2
        (M,S,D) or (M,S,D,D) fp64 views of `flat`, loglik (M,B) fp32 [, gamma (M,B,T,S) fp32], shift).  Member m's
        counts are sum_b weights[m,b] x (sequence b's counts under member m); loglik and gamma do not depend on the
        weights."""
        x, lengths, B, T = self._inputs(x, lengths)
        return self._estep(x, lengths, self._shift(shift), self._weights(weights, B), True, return_gamma)

    def log_prob(self, x, lengths=None):
        """(M,B) fp32: log p(x[b, :lengths[b]]) under each member (NaN / -inf as GaussianHMM.log_prob)."""
        x, lengths, B, T = self._inputs(x, lengths)
        return self._loglik("GaussianHMMEnsemble.log_prob", x, lengths)

    # ----------------------------------------------------------------- M-step
    @torch.no_grad()
    def m_step(self, counts, prior_count=0.0, var_floor=None, reg_covar=None):
        """GaussianHMM.m_step per member, in fp64 on the device: structural zeros (the padding included) stay, a row
        nothing was counted into keeps its parameters, and so does a state with occ = 0 or ("full", one batched
        Cholesky) a failed factorisation.  The padded states then take their member's state 0 again."""
        occ = counts["occ"].to(torch.float64)
        if self.mixture:
            self.log_pi.copy_(CodeHMM._m_rows(occ, self.log_pi, prior_count))
            rows = self.log_pi.unsqueeze(1).expand_as(self.log_A)
            self.log_A.copy_(torch.where(self.pad[:, :, None], torch.full_like(rows, NEG_INF), rows))
        else:
            self.log_pi.copy_(CodeHMM._m_rows(counts["pi_cnt"], self.log_pi, prior_count))
            self.log_A.copy_(CodeHMM._m_rows(counts["trans_cnt"], self.log_A, prior_count))
        shift = counts.get("shift")
        if shift is not None:
            shift = torch.as_tensor(shift).to(occ.device, torch.float64)
        if self.full:
            reg = reg_covar if reg_covar is not None else (1e-6 if var_floor is None else var_floor)
            D = self.dim
            o = torch.where(occ > 0, occ, torch.ones_like(occ))
            mu = counts["m1"].to(torch.float64) / o[..., None]
            cov = counts["m2"].to(torch.float64) / o[..., None, None] - mu[..., :, None] * mu[..., None, :]
            cov = cov + float(reg) * torch.eye(D, dtype=torch.float64, device=cov.device)
            old = self.scale_tril.double().tril()
            # a state that keeps its parameters is factored from its own covariance (always possible)
            safe = torch.where((occ > 0)[..., None, None], cov, old @ old.transpose(-1, -2))
            L, ok = _cholesky(torch.where(torch.isfinite(safe), safe, torch.zeros_like(safe)))
            ok = ok & (occ > 0) & torch.isfinite(cov).all((-1, -2))
            if shift is not None:
                mu = mu + shift
            self.mean.copy_(torch.where(ok[..., None], mu, self.mean.double()).float())
            self.scale_tril.copy_(torch.where(ok[..., None, None], L.tril(), old).float())
        else:
            var_floor = 1e-6 if var_floor is None else var_floor
            live = (occ > 0).unsqueeze(-1)
            o = torch.where(occ > 0, occ, torch.ones_like(occ)).unsqueeze(-1)
            mu = counts["m1"].to(torch.float64) / o
            var = (counts["m2"].to(torch.float64) / o - mu * mu).clamp_min(float(var_floor))
            if shift is not None:
                mu = mu + shift
            self.mean.copy_(torch.where(live, mu, self.mean.double()).float())
            self.log_var.copy_(torch.where(live, torch.log(var), self.log_var.double()).float())
        self._copy_padding()

    @staticmethod
    def _data_shift(x, lengths):
        """The data mean over the counted positions (D,) fp32, as GaussianHMM.fit takes it."""
        T = x.shape[1]
        mask = (torch.arange(T, device=x.device).unsqueeze(0) < lengths.clamp(0, T).unsqueeze(1)).unsqueeze(2)
        npos_t = mask.sum().clamp_min(1)
        return (torch.where(mask, x.double(), 0.0).sum((0, 1)) / npos_t).float().contiguous()

    def fit(self, x, lengths=None, n_iter=20, prior_count=0.0, var_floor=None, reg_covar=None):
        """n_iter Baum-Welch iterations of every member independently -> (n_iter, M) fp64 device tensor of the
        total log-likelihoods, each under the parameters before that iteration's M-step.  The moments are taken
        about the data mean (computed once).  No host sync."""
        x, lengths, B, T = self._inputs(x, lengths)
        shift = self._data_shift(x, lengths)
        hist = torch.empty((int(n_iter), self.num_models), dtype=torch.float64, device=x.device)
        for it in range(int(n_iter)):
            st = self._estep(x, lengths, shift, None, True, False)
            hist[it] = st["loglik"].double().nansum(1)
            self.m_step(st, prior_count, var_floor, reg_covar)
        return hist

    # -------------------------------------------------------------- selection
    def best_index(self, x, lengths=None):
        """(1,) int64 device tensor: argmax_m of the nansum over sequences of log_prob, under the current
        parameters (no host sync)."""
        return self.log_prob(x, lengths).double().nansum(1).argmax(0, keepdim=True)

    def _model(self, S):
        hmm = GaussianHMM(S, self.dim, self.covariance_type).to(self.log_pi.device)
        hmm.mixture = self.mixture
        return hmm

    def best(self, x, lengths=None):
        """The best member as a GaussianHMM (selected on the device by index_select, no host sync, so it keeps the
        ensemble's S: a smaller member stays padded)."""
        idx = self.best_index(x, lengths)
        hmm = self._model(self.num_states)
        with torch.no_grad():
            for k in ("log_pi", "log_A", "mean", "scale_tril" if self.full else "log_var"):
                getattr(hmm, k).copy_(getattr(self, k).index_select(0, idx)[0])
        return hmm

    def member(self, m):
        """Member m as a GaussianHMM copy with the padding stripped."""
        m = int(m)
        s = self.member_states[m]
        hmm = self._model(s)
        with torch.no_grad():
            hmm.log_pi.copy_(self.log_pi[m, :s])
            hmm.log_A.copy_(self.log_A[m, :s, :s])
            hmm.mean.copy_(self.mean[m, :s])
            (hmm.scale_tril if self.full else hmm.log_var).copy_(self._last[m, :s])
        return hmm

    def num_free_parameters(self):
        """(M,) fp64: the live (not -inf) entries of log_pi and of log_A's rows minus one per live row (`mixture`:
        the rows of A are pi, so the transitions count as pi's entries again, S_m - 1 for a dense member), plus the
        emission parameters of the S_m states of the member: 2 D each ("diag"), D + D (D + 1) / 2 each ("full")."""
        live_pi, live_A = self.log_pi != NEG_INF, self.log_A != NEG_INF

        def free(live):  # entries minus one per live row, over the last axis
            return (live.sum(-1) - live.any(-1).long()).reshape(live.shape[0], -1).sum(1)

        D = self.dim
        per_state = D + D * (D + 1) // 2 if self.full else 2 * D
        sm = (~self.pad).sum(1)
        trans = free(live_pi[:, None, :]) if self.mixture else free(live_A)
        return (free(live_pi[:, None, :]) + trans + sm * per_state).double()

    def bic(self, x, lengths=None):
        """(M,) fp64: -2 sum_b loglik + p_m ln(n_positions), p_m = num_free_parameters()."""
        x, lengths, B, T = self._inputs(x, lengths)
        ll = self._loglik("GaussianHMMEnsemble.bic", x, lengths).double().nansum(1)
        npos = lengths.clamp(0, T).sum().double().clamp(min=1.0)
        return -2.0 * ll + self.num_free_parameters() * torch.log(npos)

    # ---------------------------------------------------------------- mixture
    def _resp(self, loglik):
        """loglik (M,B) -> (r (M,B) fp64, ok (B,) bool, total): r = softmax_m(log_mix + loglik) with NaN read
        as -inf and a column without a finite entry all zero; total = sum over the ok columns of the logsumexp."""
        z = self.log_mix.double()[:, None] + torch.nan_to_num(loglik.double(), nan=NEG_INF, posinf=NEG_INF,
                                                              neginf=NEG_INF)
        ok = (z != NEG_INF).any(0)
        z = torch.where(ok[None, :], z, torch.zeros_like(z))
        lse = torch.logsumexp(z, 0)
        r = torch.where(ok[None, :], torch.exp(z - lse[None, :]), torch.zeros_like(z))
        return r, ok, torch.where(ok, lse, torch.zeros_like(lse)).sum()

    def responsibilities(self, x, lengths=None):
        """(M,B) fp64: p(component m | x_b) = softmax_m(log_mix + log_prob); a sequence no component can score
        (length 0, a non-finite x, impossible everywhere) gets zeros."""
        return self._resp(self.log_prob(x, lengths))[0]

    def fit_mixture(self, x, lengths=None, n_iter=20, prior_count=0.0, var_floor=None, reg_covar=None):
        """EM for the mixture sum_m mix_m HMM_m over sequences -> (n_iter,) fp64 device tensor of the mixture
        log-likelihood sum_b logsumexp_m(log_mix + loglik) under the parameters before each iteration's M-step.
        An iteration is the exact EM and therefore two batched E-steps: one for loglik (M,B), from which the
        responsibilities r follow, and one with weights = r for the expected counts; then m_step and log_mix <-
        log(mean_b r) over the sequences some component can score.  The moments are taken about the data mean.
        No host sync."""
        x, lengths, B, T = self._inputs(x, lengths)
        shift = self._data_shift(x, lengths)
        hist = torch.empty((int(n_iter),), dtype=torch.float64, device=x.device)
        for it in range(int(n_iter)):
            ll = self._loglik("GaussianHMMEnsemble.fit_mixture", x, lengths)
            r, ok, hist[it] = self._resp(ll)
            st = self._estep(x, lengths, shift, r.float().contiguous(), False, False)
            self.m_step(st, prior_count, var_floor, reg_covar)
            with torch.no_grad():
                mix = r.sum(1) / ok.sum().clamp(min=1)
                self.log_mix.copy_(torch.where(ok.any(), torch.log(mix), self.log_mix.double()).float())
        return hist
