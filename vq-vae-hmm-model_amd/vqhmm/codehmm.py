"""Stationary HMM on VQ code indices: Baum-Welch EM, ancestral sampling, Viterbi decode and the
streaming causal filter (pseudocode.txt:25-32: `hmm.train_em(all_code_indices)`, `hmm.sample(seq_len)`;
math.md:23-62 with M_t = M).  HIP only: the E-step and the sampler are the fused kernels of hmm_code.hip
(vqhmm_code_estep_f32 / vqhmm_code_sample_f32), decode and filter those of hmm_code_decode.hip
(vqhmm_code_viterbi_f32 / vqhmm_code_filter_f32), contracts in include/vqhmm.h; the M-step is
S*S + S*V numbers of torch arithmetic in fp64 on the device.  `code_log_prob` is the differentiable
log-likelihood (its backward is one weighted E-step); restarts (`fit(n_init=R)`) run on
codehmm_ensemble.CodeHMMEnsemble, R models in one launch (vqhmm_code_estep_batched_f32).
"""
import torch

from . import _ext

MAX_STATES = 32      # the kernels' limits (hmm_code.hip)
MAX_CODES = 65536


def _row_log_normalise(w):
    return torch.log(w / w.sum(-1, keepdim=True)).float()


def _check_codes(what, ref, codes, lengths):
    """codes (B,T) int32/int64 and lengths (B,) or None on ref's device -> (int32 codes, int64 lengths, B, T)."""
    _ext.require_device(ref, codes)
    if codes.dim() != 2 or codes.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: expected codes (B, T) int32 or int64, got {tuple(codes.shape)} {codes.dtype}")
    codes = codes.to(torch.int32).contiguous()
    B, T = codes.shape
    if lengths is None:
        lengths = torch.full((B,), T, dtype=torch.int64, device=codes.device)
    lengths = torch.as_tensor(lengths).to(codes.device, torch.int64).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f"{what}: lengths must have shape ({B},)")
    return codes, lengths, B, T


def _estep_batched(what, log_pi, log_A, log_B, codes, lengths, weights, want_loglik, want_gamma,
                   max_workspace_bytes=None):
    """vqhmm_code_estep_batched_f32 on stacked contiguous fp32 parameters (M,S) / (M,S,S) / (M,S,V), int32
    codes (B,T), int64 lengths (B) and weights (M,B) fp32 or None -> (pi_cnt (M,S), trans_cnt (M,S,S), emit_cnt
    (M,S,V) fp64, loglik (M,B) or None, gamma (M,B,T,S) or None).  The members run in groups whose workspace fits
    max_workspace_bytes (None: one group); a member's bits do not depend on its group."""
    M, S = log_pi.shape
    V = log_B.shape[-1]
    B, T = codes.shape
    dev = codes.device
    pi = torch.empty((M, S), dtype=torch.float64, device=dev)
    tr = torch.empty((M, S, S), dtype=torch.float64, device=dev)
    em = torch.empty((M, S, V), dtype=torch.float64, device=dev)
    ll = torch.empty((M, B), dtype=torch.float32, device=dev) if want_loglik else None
    gm = torch.empty((M, B, T, S), dtype=torch.float32, device=dev) if want_gamma else None
    lib = _ext.load()
    G = min(M, 65535)
    if max_workspace_bytes is not None:
        per = lib.vqhmm_code_estep_batched_workspace_size(B, T, S, V, 1)
        G = max(1, min(G, int(max_workspace_bytes) // max(per, 1)))
    nb = lib.vqhmm_code_estep_batched_workspace_size(B, T, S, V, G)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    st = _ext.stream_ptr(dev)

    def at(t, m0):
        return _ext.ptr(t[m0:]) if t is not None else _ext.ptr(None)

    with torch.no_grad():
        for m0 in range(0, M, G):
            _ext.check(lib.vqhmm_code_estep_batched_f32(
                at(log_pi, m0), at(log_A, m0), at(log_B, m0), _ext.ptr(codes), _ext.ptr(lengths), at(weights, m0),
                B, T, S, V, min(G, M - m0), at(pi, m0), at(tr, m0), at(em, m0), at(ll, m0), at(gm, m0),
                _ext.ptr(ws), nb, st), what)
    return pi, tr, em, ll, gm


class _CodeLogProb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_pi, log_A, log_B, codes, lengths):
        ll = _estep_batched("code_log_prob", log_pi[None], log_A[None], log_B[None], codes, lengths, None, True,
                            False)[3][0]
        ctx.save_for_backward(log_pi, log_A, log_B, codes, lengths)
        return ll

    @staticmethod
    def backward(ctx, g):
        log_pi, log_A, log_B, codes, lengths = ctx.saved_tensors
        w = g.detach().to(torch.float32).reshape(1, -1).contiguous()
        pi, tr, em, _, _ = _estep_batched("code_log_prob backward", log_pi[None], log_A[None], log_B[None], codes,
                                          lengths, w, False, False)
        return pi[0].float(), tr[0].float(), em[0].float(), None, None


def code_log_prob(log_pi, log_A, log_B, codes, lengths=None):
    """log p(codes[b, :lengths[b]]) (B,) fp32 under the HMM (log_pi (S,), log_A (S,S), log_B (S,V), fp32 device
    tensors), differentiable with respect to the three log-parameter tensors treated as free variables: train
    logits through log_softmax and autograd chains it.  The forward is the fused E-step's loglik; the backward is
    one weighted E-step with weights = grad_output, whose counts (fp64, cast to fp32) are the gradients:
    d loglik_b / d log_pi = gamma_{b,0}, / d log_A = sum_t xi_{b,t}, / d log_B[s,v] = sum_{codes=v} gamma_{b,t}(s).
    A sequence whose loglik is not finite (length 0 -> NaN, a code outside [0, V) -> NaN, impossible -> -inf)
    contributes exactly zero gradient, not the NaN a logsumexp recursion in torch would give.  grad_output must be
    finite."""
    S, V = int(log_B.shape[0]), int(log_B.shape[-1])
    for name, t, shape in (("log_pi", log_pi, (S,)), ("log_A", log_A, (S, S)), ("log_B", log_B, (S, V))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError(f"code_log_prob: {name} must be a float32 tensor of shape {shape}")
    if not (1 <= S <= MAX_STATES and 1 <= V <= MAX_CODES):
        raise ValueError(f"code_log_prob: 1 <= S <= {MAX_STATES} and 1 <= V <= {MAX_CODES} (got {S}, {V})")
    _ext.require_device(log_pi, log_A, log_B)
    codes, lengths, _, _ = _check_codes("code_log_prob", log_pi, codes, lengths)
    return _CodeLogProb.apply(log_pi.contiguous(), log_A.contiguous(), log_B.contiguous(), codes, lengths)


class CodeHMM(torch.nn.Module):
    """HMM with `num_states` hidden states emitting one of `num_codes` VQ code indices.

    Buffers (fp32 natural logs): log_pi (S,), log_A (S,S) with log_A[i,j] = log p(z_t=j | z_{t-1}=i),
    log_B (S,V) with log_B[s,v] = log p(code=v | z=s).  They start random (from `generator`) and
    row-normalised; -inf entries are structural zeros that EM keeps."""

    def __init__(self, num_states, num_codes, generator=None):
        super().__init__()
        S, V = int(num_states), int(num_codes)
        if not (1 <= S <= MAX_STATES and 1 <= V <= MAX_CODES):
            raise ValueError(f"CodeHMM: 1 <= num_states <= {MAX_STATES} and 1 <= num_codes <= {MAX_CODES} "
                             f"(got {S}, {V})")
        self.num_states, self.num_codes = S, V

        def init(*shape):
            return _row_log_normalise(torch.rand(*shape, generator=generator, dtype=torch.float64) + 0.5)

        self.register_buffer("log_pi", init(S))
        self.register_buffer("log_A", init(S, S))
        self.register_buffer("log_B", init(S, V))

    # ------------------------------------------------------------------ inputs
    def _inputs(self, codes, lengths):
        return _check_codes("CodeHMM", self.log_pi, codes, lengths)

    def _estep(self, codes, lengths, B, T, want_loglik, want_gamma):
        S, V = self.num_states, self.num_codes
        dev = codes.device
        counts = torch.empty(S + S * S + S * V, dtype=torch.float64, device=dev)
        pi_cnt, trans_cnt, emit_cnt = counts[:S], counts[S:S + S * S].view(S, S), counts[S + S * S:].view(S, V)
        loglik = torch.empty((B,), dtype=torch.float32, device=dev) if want_loglik else None
        gamma = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_gamma else None
        lib = _ext.load()
        nb = lib.vqhmm_code_estep_workspace_size(B, T, S, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        with torch.no_grad():
            _ext.check(lib.vqhmm_code_estep_f32(
                _ext.ptr(self.log_pi), _ext.ptr(self.log_A), _ext.ptr(self.log_B), _ext.ptr(codes), _ext.ptr(lengths),
                B, T, S, V, _ext.ptr(pi_cnt), _ext.ptr(trans_cnt), _ext.ptr(emit_cnt), _ext.ptr(loglik),
                _ext.ptr(gamma), _ext.ptr(ws), nb, _ext.stream_ptr(dev)), "CodeHMM.e_step")
        out = {"pi_cnt": pi_cnt, "trans_cnt": trans_cnt, "emit_cnt": emit_cnt, "flat": counts}
        if want_loglik:
            out["loglik"] = loglik
        if want_gamma:
            out["gamma"] = gamma
        return out

    # ----------------------------------------------------------------- E-step
    def e_step(self, codes, lengths=None, return_gamma=False):
        """codes (B,T) int32/int64, lengths (B,) -> dict(pi_cnt (S,), trans_cnt (S,S), emit_cnt (S,V) fp64,
        loglik (B,) fp32 [, gamma (B,T,S) fp32]); `flat` is the one buffer the three counts are views of
        (all-reduce it across ranks before m_step for data-parallel EM)."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        return self._estep(codes, lengths, B, T, True, return_gamma)

    def log_prob(self, codes, lengths=None):
        """log p(codes[b, :lengths[b]]) (B,) fp32; NaN for length 0 or a code outside [0, V), -inf if impossible."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        return self._estep(codes, lengths, B, T, True, False)["loglik"]

    def posterior(self, codes, lengths=None):
        """gamma (B,T,S) fp32: p(z_t = s | codes[b, :lengths[b]]), rows at t >= length are 0."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        return self._estep(codes, lengths, B, T, False, True)["gamma"]

    # ------------------------------------------------------- decode and filter
    def decode(self, codes, lengths=None):
        """MAP state path (Viterbi, vqhmm_code_viterbi_f32) -> (path (B,T) int32 with -1 at t >= length,
        score (B,) fp32 = the path's log weight).  Length 0: score -inf; a code outside [0, V) inside the
        length: path all -1 and score NaN."""
        codes, lengths, B, T = self._inputs(codes, lengths)
        S, V = self.num_states, self.num_codes
        dev = codes.device
        path = torch.empty((B, T), dtype=torch.int32, device=dev)
        score = torch.empty((B,), dtype=torch.float32, device=dev)
        lib = _ext.load()
        nb = lib.vqhmm_code_viterbi_workspace_size(B, T, S, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        with torch.no_grad():
            _ext.check(lib.vqhmm_code_viterbi_f32(
                _ext.ptr(self.log_pi), _ext.ptr(self.log_A), _ext.ptr(self.log_B), _ext.ptr(codes), _ext.ptr(lengths),
                B, T, S, V, _ext.ptr(path), _ext.ptr(score), _ext.ptr(ws), nb, _ext.stream_ptr(dev)),
                "CodeHMM.decode")
        return path, score

    def _filter(self, codes, lengths, state, want_filt):
        codes, lengths, B, T = self._inputs(codes, lengths)
        S, V = self.num_states, self.num_codes
        dev = codes.device
        if state is not None:
            if not torch.is_tensor(state) or state.shape != (B, S) or state.dtype != torch.float32:
                raise ValueError(f"CodeHMM: state must be a ({B}, {S}) float32 tensor")
            _ext.require_device(state)
            state = state.contiguous()
        filt = torch.empty((B, T, S), dtype=torch.float32, device=dev) if want_filt else None
        last = torch.empty((B, S), dtype=torch.float32, device=dev)
        loglik = torch.empty((B,), dtype=torch.float32, device=dev)
        lib = _ext.load()
        nb = lib.vqhmm_code_filter_workspace_size(B, T, S, V)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        with torch.no_grad():
            _ext.check(lib.vqhmm_code_filter_f32(
                _ext.ptr(self.log_pi), _ext.ptr(self.log_A), _ext.ptr(self.log_B), _ext.ptr(codes), _ext.ptr(lengths),
                _ext.ptr(state), B, T, S, V, _ext.ptr(filt), _ext.ptr(last), _ext.ptr(loglik), _ext.ptr(ws), nb,
                _ext.stream_ptr(dev)), "CodeHMM.filter")
        return filt, last, loglik

    def filter(self, codes, lengths=None, state=None, return_state=False):
        """Causal filter (vqhmm_code_filter_f32): filt (B,T,S) fp32 with filt[b,t] = p(z_t | codes[b, :t+1]) (no
        look-ahead; rows at t >= length are 0) and loglik (B,) = log p(codes[b, :length] | state).  `state`
        (B,S) fp32 is the carry of the previous chunk (None: the sequence starts from log_pi); with
        return_state the new carry filt[b, length-1] is returned too, and feeding it back gives what one call
        on the concatenated codes gives.  loglik is NaN for length 0 (the carry then passes through)."""
        filt, last, loglik = self._filter(codes, lengths, state, True)
        return (filt, loglik, last) if return_state else (filt, loglik)

    def update(self, codes, lengths=None, state=None):
        """The streaming form of `filter`: -> (state (B,S), loglik (B,)) without writing filt."""
        _, last, loglik = self._filter(codes, lengths, state, False)
        return last, loglik

    @torch.no_grad()
    def predict_next(self, state):
        """The next code's predictive distribution (B,V) fp32 from a filtered state (B,S): normalise(state A) B."""
        S = self.num_states
        if not torch.is_tensor(state) or state.dim() != 2 or state.shape[1] != S or state.dtype != torch.float32:
            raise ValueError(f"CodeHMM: state must be a (B, {S}) float32 tensor")
        _ext.require_device(self.log_pi, state)
        nxt = state @ torch.exp(self.log_A)
        nxt = nxt / nxt.sum(-1, keepdim=True)
        return nxt @ torch.exp(self.log_B)

    # ----------------------------------------------------------------- M-step
    @staticmethod
    def _m_rows(cnt, old, prior_count):
        cnt = cnt.to(torch.float64).reshape(old.shape)
        live = old != float("-inf")                      # structural zeros stay zeros
        w = torch.where(live, cnt + prior_count, torch.zeros_like(cnt))
        tot = w.sum(-1, keepdim=True)
        new = torch.log(w / tot).float()
        new = torch.where(live, new, torch.full_like(new, float("-inf")))
        return torch.where(tot > 0, new, old)            # a row nothing was counted into keeps its parameters

    @torch.no_grad()
    def m_step(self, counts, prior_count=0.0):
        """Parameters <- row-normalised (counts + prior_count), in fp64 on the device.  prior_count is added to
        every count that is not a structural zero; a row whose total is 0 keeps its previous parameters; an
        -inf parameter stays -inf."""
        self.log_pi.copy_(self._m_rows(counts["pi_cnt"], self.log_pi, prior_count))
        self.log_A.copy_(self._m_rows(counts["trans_cnt"], self.log_A, prior_count))
        self.log_B.copy_(self._m_rows(counts["emit_cnt"], self.log_B, prior_count))

    def _restart_ensemble(self, n_init, generator=None):
        """The starts of fit(n_init=R): member 0 = the current parameters, members 1..R-1 = CodeHMM(S, V, generator)
        drawn in that order, each with this model's structural zeros imposed and its rows renormalised."""
        from .codehmm_ensemble import CodeHMMEnsemble
        S, V = self.num_states, self.num_codes
        dev = self.log_pi.device
        starts = [self]
        for _ in range(int(n_init) - 1):
            h = CodeHMM(S, V, generator=generator).to(dev)
            for k in ("log_pi", "log_A", "log_B"):
                new = torch.where(getattr(self, k) != float("-inf"), getattr(h, k).double(), float("-inf"))
                lse = torch.logsumexp(new, -1, keepdim=True)
                getattr(h, k).copy_(torch.where(lse != float("-inf"), new - lse, new).float())
            starts.append(h)
        return CodeHMMEnsemble.from_models(starts)

    def fit(self, codes, lengths=None, n_iter=20, tol=None, prior_count=0.0, n_init=1, generator=None):
        """Baum-Welch: alternate e_step and m_step.  Returns the total log-likelihoods, one per iteration, each
        under the parameters before that iteration's M-step (0-dim device tensors with tol=None, so the loop
        has no host sync; floats with tol, which stops once the improvement per observed position is < tol).

        n_init = R > 1: R chains in one batched E-step per iteration (CodeHMMEnsemble): member 0 starts from the
        current parameters, members 1..R-1 from fresh random starts drawn from `generator`, all with the current
        structural zeros.  The member with the largest total log-likelihood under its final parameters (one
        more batched E-step) is copied into this model, selected on the device; the history returned is that
        member's.  No host sync; `tol` cannot be combined with it."""
        n_init = int(n_init)
        if n_init < 1:
            raise ValueError("CodeHMM.fit: n_init >= 1")
        if n_init > 1:
            if tol is not None:
                raise ValueError("CodeHMM.fit: tol needs a host sync per iteration and cannot be combined with n_init > 1")
            codes, lengths, B, T = self._inputs(codes, lengths)
            ens = self._restart_ensemble(n_init, generator)
            hist = ens.fit(codes, lengths, n_iter=n_iter, prior_count=prior_count)
            best = ens.best_index(codes, lengths)
            with torch.no_grad():
                for k in ("log_pi", "log_A", "log_B"):
                    getattr(self, k).copy_(getattr(ens, k).index_select(0, best)[0])
            return list(hist.index_select(1, best)[:, 0].unbind(0))
        codes, lengths, B, T = self._inputs(codes, lengths)
        npos = None
        history = []
        for _ in range(int(n_iter)):
            st = self._estep(codes, lengths, B, T, True, False)
            total = st["loglik"].double().nansum()
            self.m_step(st, prior_count)
            if tol is None:
                history.append(total)
                continue
            if npos is None:
                npos = max(int(lengths.clamp(0, T).sum().item()), 1)
            total = float(total.item())
            if history and (total - history[-1]) / npos < tol:
                history.append(total)
                break
            history.append(total)
        return history

    # ---------------------------------------------------------------- sampling
    def sample(self, n, seq_len, generator=None):
        """Ancestral samples -> (states (n, seq_len), codes (n, seq_len)) int64, drawn by inverse CDF from
        torch.rand((n, seq_len, 2), generator=generator, device=...).  The code indices are those of the VQ
        codebook, so `z_q_seq = codebook[codes]` is the `codebook.lookup(z_idx_seq)` of pseudocode.txt:31."""
        _ext.require_device(self.log_pi)
        n, seq_len = int(n), int(seq_len)
        dev = self.log_pi.device
        u = torch.rand((n, seq_len, 2), generator=generator, device=dev, dtype=torch.float32)
        states = torch.empty((n, seq_len), dtype=torch.int32, device=dev)
        codes = torch.empty((n, seq_len), dtype=torch.int32, device=dev)
        with torch.no_grad():
            _ext.check(_ext.load().vqhmm_code_sample_f32(
                _ext.ptr(self.log_pi), _ext.ptr(self.log_A), _ext.ptr(self.log_B), _ext.ptr(u), n, seq_len,
                self.num_states, self.num_codes, _ext.ptr(states), _ext.ptr(codes), _ext.stream_ptr(dev)),
                "CodeHMM.sample")
        return states.long(), codes.long()
