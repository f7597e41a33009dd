"""The VQ codebook as a module: quantize with a fused deterministic backward, per-code statistics, the EMA and
k-means updates, dead-code resets and the channels-first lookup (pseudocode.txt:8-32: `codebook`,
`quantize(z_e, codebook)`, `codebook.lookup(z_idx_seq)`).  HIP only: the statistics, the backward and the
lookup are the kernels of vq_codebook.hip (vqhmm_vq_stats_f32 / vqhmm_vq_quantize_bwd_f32 /
vqhmm_vq_lookup_f32, contracts in include/vqhmm.h); the updates are K*Dv numbers of torch arithmetic in fp64
on the device, rounded to fp32 once.
"""
import torch

from . import _ext
from .hmm import vq_argmin

MAX_CODES = 65536        # the kernels' limits (vq_codebook.hip)
MAX_DIM = 512
MAX_ELEMS = 1 << 21


def _lengths(lengths, B, dev):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths).to(dev, torch.int64).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f"Codebook: lengths must have shape ({B},)")
    return lengths


def _stats_launch(z, idx, lengths, weight):
    """-> flat fp64 (K + K*Dv + 1): count, rsum, sse."""
    B, Dv, T = z.shape
    K = weight.shape[0]
    flat = torch.empty(K + K * Dv + 1, dtype=torch.float64, device=z.device)
    lib = _ext.load()
    nb = lib.vqhmm_vq_stats_workspace_size(B, Dv, T, K)
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=z.device)
    _ext.check(lib.vqhmm_vq_stats_f32(_ext.ptr(z), _ext.ptr(idx), _ext.ptr(lengths), B, Dv, T, _ext.ptr(weight), K,
                                      _ext.ptr(flat[:K]), _ext.ptr(flat[K:K + K * Dv]), _ext.ptr(flat[K + K * Dv:]),
                                      _ext.ptr(ws), ws.numel(), _ext.stream_ptr(z.device)), "Codebook.stats")
    return flat


class _CodebookQuantize(torch.autograd.Function):
    """Forward: vqhmm.quantize's launch (vqhmm_vq_quantize_f32), plus the statistics launch for the counted sse
    when there are lengths.  Backward: ONE vqhmm_vq_quantize_bwd_f32 call; z_q is never materialised and the
    incoming 0-dim gradients become the two device scalars it reads, so there is no host sync."""

    @staticmethod
    def forward(ctx, z, weight, beta, lengths):
        B, Dv, T = z.shape
        K = weight.shape[0]
        idx = torch.empty((B, T), dtype=torch.int32, device=z.device)
        zq_st = torch.empty_like(z)
        sse = torch.zeros((), dtype=torch.float64, device=z.device)
        lib = _ext.load()
        nb = lib.vqhmm_vq_quantize_workspace_size(B, Dv, T, K)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=z.device)
        _ext.check(lib.vqhmm_vq_quantize_f32(_ext.ptr(z), B, Dv, T, _ext.ptr(weight), K, _ext.ptr(idx),
                                             _ext.ptr(zq_st), _ext.ptr(sse), _ext.ptr(ws), ws.numel(),
                                             _ext.stream_ptr(z.device)), "Codebook.forward")
        if lengths is None:
            n = float(max(z.numel(), 1))
        else:
            sse = _stats_launch(z, idx, lengths, weight)[-1]
            n = (lengths.clamp(0, T).sum() * Dv).clamp_min(1).double()
        mse = (sse / n).float()
        ctx.save_for_backward(z, weight, idx)
        ctx.beta, ctx.n, ctx.lengths = float(beta), n, lengths
        ctx.mark_non_differentiable(idx)
        return zq_st, idx, beta * mse, mse

    @staticmethod
    def backward(ctx, g_zq, g_idx, g_commit, g_cb):
        z, weight, idx = ctx.saved_tensors
        need_dz = ctx.needs_input_grad[0]
        need_dcb = ctx.needs_input_grad[1] and g_cb is not None
        if not (need_dz or need_dcb):
            return None, None, None, None
        B, Dv, T = z.shape
        K = weight.shape[0]
        dev = z.device

        def scale(g, c):
            if g is None:
                return torch.zeros(1, dtype=torch.float32, device=dev)
            return (g.detach().double() * c / ctx.n).float().reshape(1)

        dz_scale, dcb_scale = scale(g_commit, 2.0 * ctx.beta), scale(g_cb, -2.0)
        g_zq = g_zq.contiguous().float() if g_zq is not None else None
        dz = torch.empty_like(z) if need_dz else None
        dcb = torch.empty_like(weight) if need_dcb else None
        lib = _ext.load()
        nb = lib.vqhmm_vq_quantize_bwd_workspace_size(B, Dv, T, K)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
        _ext.check(lib.vqhmm_vq_quantize_bwd_f32(
            _ext.ptr(z), _ext.ptr(idx), _ext.ptr(ctx.lengths), B, Dv, T, _ext.ptr(weight), K, _ext.ptr(g_zq),
            _ext.ptr(dz_scale), _ext.ptr(dcb_scale), _ext.ptr(dz), _ext.ptr(dcb), _ext.ptr(ws), ws.numel(),
            _ext.stream_ptr(dev)), "Codebook.backward")
        return dz, dcb, None, None


class Codebook(torch.nn.Module):
    """`num_codes` code vectors of `dim` channels.

    decay=None: `weight` (K,Dv) fp32 is a Parameter, trained by the optimizer through the codebook loss
    (pseudocode.txt:18).  With a decay in [0, 1) `weight` is a buffer updated by `ema_update` from the fp64
    buffers `ema_count` (K) and `ema_sum` (K,Dv), and `forward` in training mode applies the update itself."""

    def __init__(self, num_codes, dim, beta=0.25, decay=None, eps=1e-5, generator=None):
        super().__init__()
        K, Dv = int(num_codes), int(dim)
        if not (1 <= K <= MAX_CODES and 1 <= Dv <= MAX_DIM and K * Dv <= MAX_ELEMS):
            raise ValueError(f"Codebook: 1 <= num_codes <= {MAX_CODES}, 1 <= dim <= {MAX_DIM} and "
                             f"num_codes * dim <= {MAX_ELEMS} (got {K}, {Dv})")
        if decay is not None and not (0.0 <= float(decay) < 1.0):
            raise ValueError(f"Codebook: decay must be None or in [0, 1) (got {decay})")
        if not float(eps) >= 0.0:
            raise ValueError(f"Codebook: eps must be >= 0 (got {eps})")
        self.num_codes, self.dim = K, Dv
        self.beta, self.eps = float(beta), float(eps)
        self.decay = None if decay is None else float(decay)
        w = (torch.rand(K, Dv, generator=generator, dtype=torch.float32) * 2.0 - 1.0) / K
        if self.decay is None:
            self.weight = torch.nn.Parameter(w)
        else:
            self.register_buffer("weight", w)
            self.register_buffer("ema_count", torch.zeros(K, dtype=torch.float64))
            self.register_buffer("ema_sum", torch.zeros(K, Dv, dtype=torch.float64))

    # ------------------------------------------------------------------ inputs
    def _z(self, z):
        _ext.require_device(self.weight, z)
        if z.dim() != 3 or z.shape[1] != self.dim:
            raise ValueError(f"Codebook: expected z (B, {self.dim}, T), got {tuple(z.shape)}")
        return z.contiguous().float()

    def _idx(self, idx, B, T):
        _ext.require_device(idx)
        if idx.shape != (B, T) or idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"Codebook: expected idx ({B}, {T}) int32 or int64, got {tuple(idx.shape)} {idx.dtype}")
        return idx.to(torch.int32).contiguous()

    # ----------------------------------------------------------------- forward
    def forward(self, z, lengths=None):
        """z (B,Dv,T) -> (z_q_st, idx, commit, codebook_loss) as vqhmm.quantize(z, weight, beta) gives them (bit
        for bit without lengths).  With lengths both losses are sse_counted / (Dv * sum clamp(lengths, 0, T))
        and z receives the commit gradient at counted positions only; z_q_st and idx are written everywhere.
        In EMA mode codebook_loss is 0 and, in training mode, the call ends with the EMA update."""
        z = self._z(z)
        lengths = _lengths(lengths, z.shape[0], z.device)
        weight = self.weight.contiguous()
        zq_st, idx, commit, cb_loss = _CodebookQuantize.apply(z, weight, self.beta, lengths)
        if self.decay is not None:
            cb_loss = torch.zeros_like(cb_loss)
            if self.training:
                self.ema_update(self.stats(z.detach(), idx, lengths))
        return zq_st, idx, commit, cb_loss

    # -------------------------------------------------------------- statistics
    @torch.no_grad()
    def stats(self, z, idx=None, lengths=None):
        """-> dict(count (K,), rsum (K,Dv), sse () fp64, flat): over the positions with t < lengths[b] and
        0 <= idx < K, count[k] = how many chose code k, rsum[k] = the sum of their residuals z - weight[k],
        sse = the sum of the squared residuals.  `flat` is the one buffer the three are views of (all-reduce
        it across ranks before an update for data-parallel codebook learning).  idx=None: vq_argmin(z, weight)."""
        z = self._z(z)
        B, Dv, T = z.shape
        K = self.num_codes
        weight = self.weight.detach().contiguous()
        idx = vq_argmin(z, weight) if idx is None else self._idx(idx, B, T)
        flat = _stats_launch(z, idx, _lengths(lengths, B, z.device), weight)
        return {"count": flat[:K], "rsum": flat[K:K + K * Dv].view(K, Dv), "sse": flat[K + K * Dv], "flat": flat}

    # ----------------------------------------------------------------- updates
    @torch.no_grad()
    def kmeans_step(self, stats):
        """weight[k] += rsum[k] / count[k] (the mean of the vectors that chose k) where count[k] > 0, in fp64
        on the device; an empty code keeps its row."""
        count, rsum = stats["count"].unsqueeze(1), stats["rsum"]
        w = self.weight.double()
        self.weight.copy_(torch.where(count > 0, w + rsum / count.clamp_min(1.0), w).float())

    @torch.no_grad()
    def ema_update(self, stats):
        """ema_count <- g ema_count + (1 - g) count, ema_sum <- g ema_sum + (1 - g) (rsum + count weight),
        weight <- ema_sum / ((ema_count + eps) / (N + K eps) N) with N = sum ema_count, in fp64 on the device; a
        code whose smoothed count is 0 keeps its row."""
        if self.decay is None:
            raise RuntimeError("Codebook: ema_update needs a decay (this codebook is trained by gradient)")
        g, K = self.decay, self.num_codes
        count, rsum = stats["count"], stats["rsum"]
        w = self.weight.double()
        self.ema_count.mul_(g).add_(count, alpha=1.0 - g)
        self.ema_sum.mul_(g).add_(rsum + count.unsqueeze(1) * w, alpha=1.0 - g)
        N = self.ema_count.sum()
        smooth = (self.ema_count + self.eps) / (N + K * self.eps) * N
        live = (self.ema_count > 0).unsqueeze(1)
        new = self.ema_sum / torch.where(live, smooth.unsqueeze(1), torch.ones_like(w))
        self.weight.copy_(torch.where(live, new, w).float())

    def _pick(self, z, lengths, n, generator):
        """n rows (n, Dv) of z at randomly chosen counted positions (distinct while there are enough of them),
        without a host sync."""
        B, Dv, T = z.shape
        dev = z.device
        perm = torch.randperm(B * T, generator=generator, device=generator.device if generator is not None else dev)
        perm = perm.to(dev)
        if lengths is None:
            avail = torch.tensor(B * T, device=dev)
        else:
            ok = (torch.arange(T, device=dev).unsqueeze(0) < lengths.clamp(0, T).unsqueeze(1)).reshape(-1)[perm]
            perm = perm[torch.argsort((~ok).to(torch.uint8), stable=True)]   # counted positions first
            avail = ok.sum()
        sel = perm[torch.arange(n, device=dev) % avail.clamp_min(1)]
        return z[sel // T, :, sel % T]

    @torch.no_grad()
    def fit_kmeans(self, z, lengths=None, n_iter=10, init=True, generator=None):
        """Lloyd's algorithm: alternate stats (with its own argmin) and kmeans_step.  init=True first seeds weight
        from K distinct counted positions of z (torch.randperm with the generator).  Returns the per-iteration
        distortion sse / (Dv * n_counted), each under the codebook before that step, as 0-dim device tensors
        (the loop has no host sync)."""
        z = self._z(z)
        lengths = _lengths(lengths, z.shape[0], z.device)
        if z.shape[0] * z.shape[2] == 0:
            return []
        if init:
            self.weight.copy_(self._pick(z, lengths, self.num_codes, generator))
        history = []
        for _ in range(int(n_iter)):
            st = self.stats(z, None, lengths)
            history.append(st["sse"] / (st["count"].sum().clamp_min(1.0) * self.dim))
            self.kmeans_step(st)
        return history

    @torch.no_grad()
    def reset_dead_codes(self, z, lengths=None, min_count=1.0, generator=None):
        """Re-seed the dead rows (EMA mode: ema_count < min_count, whose EMA state restarts at min_count copies
        of the new row; gradient mode: no position of z chose them) from randomly chosen counted positions of z.
        Returns how many rows it replaced."""
        z = self._z(z)
        lengths = _lengths(lengths, z.shape[0], z.device)
        if z.shape[0] * z.shape[2] == 0:
            return 0
        if self.decay is not None:
            dead = self.ema_count < float(min_count)
        else:
            dead = self.stats(z, None, lengths)["count"] == 0
        rows = torch.nonzero(dead).reshape(-1)
        n = int(rows.numel())
        if n == 0:
            return 0
        new = self._pick(z, lengths, n, generator)
        self.weight[rows] = new
        if self.decay is not None:
            self.ema_count[rows] = float(min_count)
            self.ema_sum[rows] = new.double() * float(min_count)
        return n

    # --------------------------------------------------------------- read-outs
    @torch.no_grad()
    def lookup(self, idx):
        """idx (B,T) int32 or int64 -> (B,Dv,T) fp32 = weight[idx] channels-first, zeros where idx is outside
        [0, K) (CodeHMM's -1 padding): `cb.lookup(hmm.sample(n, L)[1])` is pseudocode.txt:30-31."""
        _ext.require_device(self.weight, idx)
        if idx.dim() != 2:
            raise ValueError(f"Codebook: expected idx (B, T), got {tuple(idx.shape)}")
        B, T = idx.shape
        idx = self._idx(idx, B, T)
        out = torch.empty((B, self.dim, T), dtype=torch.float32, device=idx.device)
        _ext.check(_ext.load().vqhmm_vq_lookup_f32(_ext.ptr(self.weight.detach().contiguous()), self.num_codes,
                                                   self.dim, _ext.ptr(idx), B, T, _ext.ptr(out),
                                                   _ext.stream_ptr(idx.device)), "Codebook.lookup")
        return out

    @staticmethod
    @torch.no_grad()
    def perplexity(count):
        """exp(-sum p ln p) with p = count / sum(count) and 0 ln 0 = 0: the effective number of codes in use."""
        p = count.double() / count.double().sum()
        return torch.exp(-torch.special.xlogy(p, p).sum())
