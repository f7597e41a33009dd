"""A stack of M stationary HMMs on VQ code indices fitted together: EM restarts, members of different state
counts (model selection), and a mixture of HMMs.  Every E-step is one call of vqhmm_code_estep_batched_f32
(hmm_code.hip): the member is a grid dimension of CodeHMM's fused kernel, so M models cost three launches,
and member m's counts, loglik and gamma are bit-identical to `CodeHMM.e_step` on member m.  The M-step is
CodeHMM's row normalisation applied along the last axis of the stacked tensors, in fp64 on the device.
decode / filter / sample stay on CodeHMM: `member(m)` or `best()` hands one over.
"""
import math

import torch

from . import _ext
from .codehmm import CodeHMM, _check_codes, _estep_batched

NEG_INF = float("-inf")


class CodeHMMEnsemble(torch.nn.Module):
    """M HMMs over the same `num_codes` codes.

    Buffers (fp32 natural logs): log_pi (M,S), log_A (M,S,S), log_B (M,S,V) and log_mix (M,), the mixture
    weights `fit_mixture` learns (uniform at the start).  `num_states` is an int (every member has S states;
    `num_models` of them) or a sequence with one entry per member; S is the largest.  A member with S_m < S is
    the padded larger model: log_pi[m, S_m:] = -inf, log_A[m] = -inf wherever the row or the column is >= S_m
    and log_B[m, S_m:] uniform (those states are unreachable).  -inf is a structural zero that EM keeps, so
    the padding survives every M-step.  Each member starts as CodeHMM(S_m, V, generator) does, in member order.

    `max_workspace_bytes` (default 1 GiB, an engineering default) caps the E-step's workspace, which is M
    single-model workspaces (4 S bytes per position and member): the members then run in groups that fit,
    with the same bits."""

    def __init__(self, num_models=None, num_states=None, num_codes=None, generator=None,
                 max_workspace_bytes=1 << 30):
        super().__init__()
        if num_states is None or num_codes is None:
            raise ValueError("CodeHMMEnsemble: num_states and num_codes are required")
        if isinstance(num_states, (list, tuple)):
            sizes = [int(s) for s in num_states]
            if num_models is not None and int(num_models) != len(sizes):
                raise ValueError("CodeHMMEnsemble: num_models does not match len(num_states)")
        else:
            if num_models is None:
                raise ValueError("CodeHMMEnsemble: num_models is required with an integer num_states")
            sizes = [int(num_states)] * int(num_models)
        if not 1 <= len(sizes) <= 65535:
            raise ValueError(f"CodeHMMEnsemble: 1 <= num_models <= 65535 (got {len(sizes)})")
        self._setup([CodeHMM(s, num_codes, generator=generator) for s in sizes], max_workspace_bytes)

    def _setup(self, models, max_workspace_bytes):
        V = models[0].num_codes
        if any(h.num_codes != V for h in models):
            raise ValueError("CodeHMMEnsemble: the members must share num_codes")
        self.member_states = [h.num_states for h in models]
        M, S = len(models), max(self.member_states)
        self.num_models, self.num_states, self.num_codes = M, S, V
        self.max_workspace_bytes = int(max_workspace_bytes)
        dev = models[0].log_pi.device
        log_pi = torch.full((M, S), NEG_INF, dtype=torch.float32, device=dev)
        log_A = torch.full((M, S, S), NEG_INF, dtype=torch.float32, device=dev)
        log_B = torch.full((M, S, V), -math.log(V), dtype=torch.float32, device=dev)
        for m, h in enumerate(models):
            s = h.num_states
            log_pi[m, :s] = h.log_pi.detach().to(dev)
            log_A[m, :s, :s] = h.log_A.detach().to(dev)
            log_B[m, :s] = h.log_B.detach().to(dev)
        self.register_buffer("log_pi", log_pi)
        self.register_buffer("log_A", log_A)
        self.register_buffer("log_B", log_B)
        self.register_buffer("log_mix", torch.full((M,), -math.log(M), dtype=torch.float32, device=dev))

    @classmethod
    def from_models(cls, models, max_workspace_bytes=1 << 30):
        """An ensemble of copies of the given CodeHMMs (same num_codes; S padded to the largest), on the
        first one's device."""
        models = list(models)
        if not 1 <= len(models) <= 65535 or not all(isinstance(h, CodeHMM) for h in models):
            raise ValueError("CodeHMMEnsemble.from_models: a non-empty sequence of CodeHMM")
        self = cls.__new__(cls)
        torch.nn.Module.__init__(self)
        self._setup(models, max_workspace_bytes)
        return self

    # ----------------------------------------------------------------- E-step
    def _inputs(self, codes, lengths):
        return _check_codes("CodeHMMEnsemble", self.log_pi, codes, lengths)

    def _weights(self, weights, B):
        if weights is None:
            return None
        M = self.num_models
        if not torch.is_tensor(weights) or weights.dtype != torch.float32 or tuple(weights.shape) not in ((M, B), (B,)):
            raise ValueError(f"CodeHMMEnsemble: weights must be a float32 tensor of shape ({M}, {B}) or ({B},)")
        _ext.require_device(weights)
        return (weights.expand(M, B) if weights.dim() == 1 else weights).contiguous()

    def _estep(self, codes, lengths, weights, want_loglik, want_gamma):
        M, S, V = self.num_models, self.num_states, self.num_codes
        pi, tr, em, ll, gm = _estep_batched("CodeHMMEnsemble.e_step", self.log_pi, self.log_A, self.log_B, codes,
                                            lengths, weights, want_loglik, want_gamma, self.max_workspace_bytes)
        # one (M, S + S*S + S*V) buffer the three counts are views of: what data-parallel EM all-reduces
        flat = torch.cat((pi, tr.view(M, S * S), em.view(M, S * V)), 1)
        out = {"pi_cnt": flat[:, :S], "trans_cnt": flat[:, S:S + S * S].view(M, S, S),
               "emit_cnt": flat[:, S + S * S:].view(M, S, V), "flat": flat}
        if want_loglik:
            out["loglik"] = ll
        if want_gamma:
            out["gamma"] = gm
        return out

    def e_step(self, codes, lengths=None, weights=None, return_gamma=False):
        """codes (B,T) int32/int64 and lengths (B,), shared by all members; weights (M,B) or (B,) (broadcast)
        float32 device tensor, None = all 1 -> dict(pi_cnt (M,S), trans_cnt (M,S,S), emit_cnt (M,S,V) fp64 views
        of flat (M, S+S*S+S*V), loglik (M,B) fp32 [, gamma (M,B,T,S) fp32]).  Member m's counts are
        sum_b weights[m,b] x (sequence b's counts under member m); loglik and gamma do not depend on the weights."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        return self._estep(codes, lengths, self._weights(weights, B), True, return_gamma)

    def log_prob(self, codes, lengths=None):
        """(M,B) fp32: log p(codes[b, :lengths[b]]) under each member (NaN / -inf as CodeHMM.log_prob)."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        return _estep_batched("CodeHMMEnsemble.log_prob", self.log_pi, self.log_A, self.log_B, codes, lengths, None,
                              True, False, self.max_workspace_bytes)[3]

    # ----------------------------------------------------------------- M-step
    @torch.no_grad()
    def m_step(self, counts, prior_count=0.0):
        """CodeHMM.m_step per member: structural zeros (the padding included) stay, a row nothing was counted
        into keeps its parameters."""
        self.log_pi.copy_(CodeHMM._m_rows(counts["pi_cnt"], self.log_pi, prior_count))
        self.log_A.copy_(CodeHMM._m_rows(counts["trans_cnt"], self.log_A, prior_count))
        self.log_B.copy_(CodeHMM._m_rows(counts["emit_cnt"], self.log_B, prior_count))

    def fit(self, codes, lengths=None, n_iter=20, prior_count=0.0):
        """n_iter Baum-Welch iterations of every member independently -> (n_iter, M) fp64 device tensor of the
        total log-likelihoods, each under the parameters before that iteration's M-step.  No host sync."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        hist = torch.empty((int(n_iter), self.num_models), dtype=torch.float64, device=codes.device)
        for it in range(int(n_iter)):
            st = self._estep(codes, lengths, None, True, False)
            hist[it] = st["loglik"].double().nansum(1)
            self.m_step(st, prior_count)
        return hist

    # -------------------------------------------------------------- selection
    def best_index(self, codes, lengths=None):
        """(1,) int64 device tensor: argmax_m of the nansum over sequences of log_prob, under the current
        parameters (no host sync)."""
        return self.log_prob(codes, lengths).double().nansum(1).argmax(0, keepdim=True)

    def best(self, codes, lengths=None):
        """The best member as a CodeHMM (selected on the device by index_select, no host sync, so it keeps
        the ensemble's S: a smaller member stays padded with -inf)."""
        idx = self.best_index(codes, lengths)
        hmm = CodeHMM(self.num_states, self.num_codes).to(self.log_pi.device)
        with torch.no_grad():
            for k in ("log_pi", "log_A", "log_B"):
                getattr(hmm, k).copy_(getattr(self, k).index_select(0, idx)[0])
        return hmm

    def member(self, m):
        """Member m as a CodeHMM copy with the padding stripped."""
        m = int(m)
        s = self.member_states[m]
        hmm = CodeHMM(s, self.num_codes).to(self.log_pi.device)
        with torch.no_grad():
            hmm.log_pi.copy_(self.log_pi[m, :s])
            hmm.log_A.copy_(self.log_A[m, :s, :s])
            hmm.log_B.copy_(self.log_B[m, :s])
        return hmm

    def num_free_parameters(self):
        """(M,) fp64: the live (not -inf) entries of log_pi, log_A and of log_B's rows at states that can be
        reached, minus one per row that has a live entry."""
        live_pi, live_A = self.log_pi != NEG_INF, self.log_A != NEG_INF
        reach = live_pi | live_A.any(1)                        # (M,S): some way into the state
        live_B = (self.log_B != NEG_INF) & reach[:, :, None]

        def free(live):  # entries minus one per live row, over the last axis
            return (live.sum(-1) - live.any(-1).long()).reshape(live.shape[0], -1).sum(1)

        return (free(live_pi[:, None, :]) + free(live_A) + free(live_B)).double()

    def bic(self, codes, lengths=None):
        """(M,) fp64: -2 sum_b loglik + p_m ln(n_positions), p_m = num_free_parameters()."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        ll = self.log_prob(codes, lengths).double().nansum(1)
        npos = lengths.clamp(0, T).sum().double().clamp(min=1.0)
        return -2.0 * ll + self.num_free_parameters() * torch.log(npos)

    # ---------------------------------------------------------------- mixture
    def _resp(self, loglik):
        """loglik (M,B) -> (r (M,B) fp64, ok (B,) bool, total): r = softmax_m(log_mix + loglik) with NaN read
        as -inf and a column without a finite entry all zero; total = sum over the ok columns of the logsumexp."""
        z = self.log_mix.double()[:, None] + torch.nan_to_num(loglik.double(), nan=NEG_INF, posinf=NEG_INF, neginf=NEG_INF)
        ok = (z != NEG_INF).any(0)
        z = torch.where(ok[None, :], z, torch.zeros_like(z))
        lse = torch.logsumexp(z, 0)
        r = torch.where(ok[None, :], torch.exp(z - lse[None, :]), torch.zeros_like(z))
        return r, ok, torch.where(ok, lse, torch.zeros_like(lse)).sum()

    def responsibilities(self, codes, lengths=None):
        """(M,B) fp64: p(component m | codes_b) = softmax_m(log_mix + log_prob); a sequence no component can
        score (length 0, a bad code, impossible everywhere) gets zeros."""
        return self._resp(self.log_prob(codes, lengths))[0]

    def fit_mixture(self, codes, lengths=None, n_iter=20, prior_count=0.0):
        """EM for the mixture sum_m mix_m HMM_m -> (n_iter,) fp64 device tensor of the mixture log-likelihood
        sum_b logsumexp_m(log_mix + loglik) under the parameters before each iteration's M-step.  An iteration
        is the exact EM and therefore two batched E-steps: one for loglik (M,B), from which the
        responsibilities r follow, and one with weights = r for the expected counts (the counts cannot be
        weighted before r is known, and r needs every member's loglik); then m_step and
        log_mix <- log(mean_b r) over the sequences some component can score.  No host sync."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        hist = torch.empty((int(n_iter),), dtype=torch.float64, device=codes.device)
        for it in range(int(n_iter)):
            ll = _estep_batched("CodeHMMEnsemble.fit_mixture", self.log_pi, self.log_A, self.log_B, codes, lengths,
                                None, True, False, self.max_workspace_bytes)[3]
            r, ok, hist[it] = self._resp(ll)
            st = self._estep(codes, lengths, r.float().contiguous(), False, False)
            self.m_step(st, prior_count)
            with torch.no_grad():
                mix = r.sum(1) / ok.sum().clamp(min=1)
                self.log_mix.copy_(torch.where(ok.any(), torch.log(mix), self.log_mix.double()).float())
        return hist
