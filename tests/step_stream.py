"""Streams of differently shaped batches through one TrainState (a helper for tests/test_gpu_step_stream.py, not a
test): the case tables, their host-only geometry checks and the checker that drives a stream.

train_model() does not feed one shape again and again.  collate_fn and DeviceChunkLoader pad to the batch maximum,
so T changes from batch to batch; an epoch's last batch is smaller; beta changes every epoch; and TrainState keeps
one workspace per (B, T), to which it comes back many Adam updates later.  That workspace then still holds the
prologue's weight images and Ecopy / Wcopy of older parameters, slabs of a launch whose count another shape set,
the cnt and sync words, and the LDS slot rows a strip does not write hold what a launch of another shape left.

StreamChecker treats one step as a function of (parameters, both Adam moments, step counter, batch, beta): before
every step of the long-lived (streamed) state it snapshots flat, exp_avg, exp_avg_sq and step_dev, loads them
into a fresh model and TrainState whose workspace is NaN-filled (test_gpu_configs.poison_workspace), runs the same
step there, and requires loss, grad, flat, exp_avg, exp_avg_sq and step_dev to be equal bit for bit.

STRIP_STREAM, at cfg2's dims, sits on the strip kernels' row-count edges (test_gpu_bwdw_sched / _latency /
test_gpu_strip_own restate the launchers' arithmetic; check_strip_row holds each row of the table to it).
SHORT_STREAM runs on dims of the other kernel families, taken from width_cases by name, whose family assertions
(tests/test_width_cases.py) keep them on those kernels.
"""
from collections import namedtuple

import torch

import width_cases as W

FORMS = ("fused", "split", "clip", "overlap", "graph")
# the forms README.md documents as bit-identical to each other (clipping rescales the gradient)
SAME_BITS = ("fused", "split", "overlap", "graph")

STRIP_DIMS = (5, 64, 3, 32, 4, 128)
SF_OWN = 122  # rows a forward strip owns (strip.hip: window rows 3 .. 124)

# R = B (T + 2) PCL rows; own / bwd / most: the folded backward strip's owned rows, strip count and strips of the
# busiest workgroup; last: rows its last strip owns; fwd: forward strips; fused_only: run in the `fused` form alone;
# oracle: the `split` form also holds this step to the fp64 oracle at the streamed state's own parameters
Step = namedtuple("Step", "B T beta R own bwd most last fwd fused_only oracle why")

STRIP_STREAM = [
    Step(96, 150, 0.25, 14592, 60, 244, 1, 12, 120, False, False, "244 backward strips of 60 rows, 120 forward strips"),
    Step(5, 71, 0.5, 365, 4, 92, 1, 1, 3, False, False, "R = 365: 3 forward strips; a small launch after a large one"),
    Step(96, 150, 0.5, 14592, 60, 244, 1, 12, 120, False, True, "first revisit: its workspace two Adam updates stale"),
    Step(310, 198, 0.75, 62000, 84, 739, 3, 8, 509, True, False, "739 strips on 256 workgroups, three per workgroup"),
    Step(1, 5, 1.0, 7, 4, 2, 1, 3, 1, False, False, "R = 7: both clamps in one window"),
    Step(25, 39, 1.0, 1025, 8, 129, 1, 1, 9, False, False, "R = 1025: a last strip of one row"),
    Step(104, 57, 0.25, 6136, 24, 256, 1, 16, 51, False, True, "a 'last batch': exactly 256 backward strips of 24"),
    Step(96, 150, 0.5, 14592, 60, 244, 1, 12, 120, False, True, "second revisit"),
]

# (B, T, beta); the third step (the first revisit) also meets the oracle in the `split` form
SHORT_STREAM = [(7, 90, 0.5), (3, 40, 1.0), (7, 90, 0.25), (9, 130, 1.0), (7, 90, 0.5)]
SHORT_ORACLE_STEP = 3

CFG4_DIMS = (16, 64, 8, 32, 4, 128)  # BASELINE configs[4]; not a width_cases row
SHORT_CASES = ("w_h48", "h16", "d17_k8", "k32_wide_rows", "d6_h64")
SHORT_DIMS = dict([("cfg4", CFG4_DIMS)] + [(n, W.BY_NAME[n].dims) for n in SHORT_CASES])
# what each short-stream case is here for: (stage, family) pairs at the stream's most visited shape (7, 90)
SHORT_FAMILIES = {
    "cfg4": (("enc2", "fused_pair"), ("head", "coop"), ("w_enc1", "wgrad2_group")),
    "w_h48": (("enc2", "fused_pair"), ("w_enc1", "wgrad2_group")),
    "h16": (("enc2", "conv2"), ("w_enc1", "wgrad2"), ("reduce", "grad_tail")),
    "d17_k8": (("head", "staged:l1<16>;hid=conv_mm<64,128,16>;lgA=convbig;dhid=convbig;dW1=wgradbig;dW2=wgradbig"),),
    "k32_wide_rows": (("enc1", "convbig"), ("w_enc1", "wgradbig")),
    "d6_h64": (("enc2_dg", "strip_bwd"), ("w_enc1", "wgrad2_group")),
}

ORACLE_RTOL = 1e-5  # gradients, normwise: the value the strip tests use at ragged shapes


def stream_lengths(B, T, seed):
    """width_cases._lengths (T, 1, 2, the middle, ...), extended by a seeded draw from [1, T] for B > 9."""
    base = [n for n in W._lengths(B, T)]
    if B > len(base):
        gen = torch.Generator().manual_seed(seed)
        base += torch.randint(1, T + 1, (B - len(base),), generator=gen).tolist()
    L = torch.tensor(base, dtype=torch.int64)
    assert L.shape == (B,) and int(L.min()) >= 1 and int(L.max()) == T
    return L


def stream_batch(dims, B, T, k):
    """Step k's batch (CPU): new data for every step, seeded from the step index."""
    D, U = dims[0], dims[4]
    gen = torch.Generator().manual_seed(7000 + k)
    x = torch.randn(B, D, T, generator=gen)
    u = torch.randn(B, U, T, generator=gen)
    return x, u, stream_lengths(B, T, 7100 + k)


def strip_stream(form):
    """[(k, Step)] of STRIP_STREAM for a form, k counting from 1 over the whole table (so a step's data and beta
    do not depend on whether the fused-only step ran)."""
    return [(k, s) for k, s in enumerate(STRIP_STREAM, 1) if form == "fused" or not s.fused_only]


def short_stream():
    return [(k, Step(B, T, beta, B * (T + 2), 0, 0, 0, 0, 0, False, k == SHORT_ORACLE_STEP, ""))
            for k, (B, T, beta) in enumerate(SHORT_STREAM, 1)]


def check_strip_row(s):
    """A STRIP_STREAM row against the launchers' arithmetic (host-only)."""
    from test_gpu_bwdw_sched import bwdw_own, bwdw_strips
    assert s.R == s.B * (s.T + 2)
    assert bwdw_own(s.R) == s.own and s.own % 4 == 0 and 3 + s.own - 1 <= 124
    n, grid, hi, lo = bwdw_strips(s.R)
    assert (n, hi) == (s.bwd, s.most) and grid == min(n, 256)
    assert s.R - (n - 1) * s.own == s.last and 1 <= s.last <= s.own
    assert -(-s.R // SF_OWN) == s.fwd
    L = stream_lengths(s.B, s.T, 0)
    if s.B >= 3:
        assert {s.T, 1, 2} <= set(L.tolist())


def runs_the_strips(dims, B, T):
    """strip_fwd for the four forward convolutions and the folded strip_bwdw for the whole backward (host-only)."""
    from test_gpu_bwdw_wgpass import _runs_folded_strip
    D, H, K, H2, U, TH = dims
    assert U == 4
    fam = W.stage_families(dims, B, T)
    return all(fam[s] == "strip_fwd" for s in ("enc1", "enc2", "dec1", "dec2")) and \
        _runs_folded_strip((D, H, K, H2, TH), B, T)


def state_dict_of(st, flat):
    """A flat parameter buffer of TrainState st as a CPU state dict."""
    import vqhmm
    named = dict(st.model.named_parameters())
    return {n: flat[st.off[i]:st.off[i + 1]].view_as(named[n]).cpu().clone() for i, n in enumerate(vqhmm.PARAM_ORDER)}


def check_loss_vs_fp64(sd, x, u, L, beta, dims, loss):
    """The device's loss within LOSS_RTOL of the fp64 oracle's (its own ReLU branch) at the parameters sd."""
    from oracle import ref_model as RM
    from test_gpu_model import LOSS_RTOL
    with torch.no_grad():
        ref = RM.elbo({k: v.double() for k, v in sd.items()}, x.double(), u.double(), L, beta, dims[2], dims[4]).item()
    print(f"loss {loss!r} vs fp64 oracle {ref!r}: {abs(loss - ref) / abs(ref):.2e}")
    assert abs(loss - ref) <= LOSS_RTOL * abs(ref), (loss, ref)


COMPARED = ("loss", "grad", "flat", "exp_avg", "exp_avg_sq", "step_dev")
SNAPSHOT = ("flat", "exp_avg", "exp_avg_sq", "step_dev")


class StreamChecker:
    """One long-lived TrainState driven through a stream in one step form, every step repeated on a fresh state.

    form   fused    st.step(...): forward_backward_adam
           split    forward_backward + apply_adam (the data-parallel step's kernels without the all-reduce)
           clip     st.step(..., max_norm=1.0)
           overlap  TrainState(..., overlap_bwd=True)
           graph    one capture(x, u, lengths, beta, warmup=0) per distinct (B, T, beta), on device tensors that
                    prepare() returns unchanged, replayed after the step's batch was copied into them in place;
                    the fresh side stays eager."""

    def __init__(self, dims, form, lr=1e-3):
        assert form in FORMS
        self.dims, self.form, self.lr = dims, form, lr
        torch.manual_seed(0)
        self.st = self._state()
        self.losses = []    # the streamed state's per-step losses since the last take_epoch()
        self.nsteps = 0
        self._static = {}   # (B, T) -> the graph form's input tensors
        self._graphs = {}   # (B, T, beta) -> replay

    def _state(self):
        import vqhmm
        D, H, K, H2, U, TH = self.dims
        m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=U, trans_hidden=TH).cuda()
        return vqhmm.TrainState(m, lr=self.lr, overlap_bwd=self.form == "overlap")

    def _replay(self, x, u, L, beta):
        st = self.st
        B, _, T = x.shape
        if (B, T) not in self._static:
            dev = st.device
            self._static[B, T] = (torch.empty(x.shape, dtype=torch.float32, device=dev),
                                  torch.empty(u.shape, dtype=torch.float32, device=dev),
                                  torch.empty(B, dtype=torch.int64, device=dev))
            st.workspace(B, T)  # allocated outside the capture
        static = self._static[B, T]
        for dst, src in zip(static, (x, u, L)):
            dst.copy_(src)
        if (B, T, beta) not in self._graphs:
            assert all(a is b for a, b in zip(st.prepare(*static), static))
            self._graphs[B, T, beta] = st.capture(*static, beta, warmup=0)
            assert st.step_graphs == 1
        self._graphs[B, T, beta]()

    def _run(self, st, x, u, L, beta, between=None):
        if self.form == "split":
            xs, us, Ls = st.prepare(x, u, L)
            st.forward_backward(xs, us, Ls, beta)
            if between is not None:
                between()
            st.apply_adam()
        elif self.form == "clip":
            st.step(x, u, L, beta, max_norm=1.0)
        elif self.form == "graph" and st is self.st:
            self._replay(x, u, L, beta)
        else:
            st.step(x, u, L, beta)

    def step(self, x, u, L, beta, oracle=False):
        """One step of the stream.  oracle=True (split form): between the streamed state's forward_backward and
        its Adam update, the ReLU-mask rule and the gradients against the fp64 oracle on the device's branch
        (test_gpu_configs.check_state_vs_oracle, ORACLE_RTOL) and the loss against the fp64 oracle, all at the
        streamed state's own pre-step parameters."""
        from test_gpu_configs import check_state_vs_oracle, poison_workspace
        st = self.st
        B, _, T = x.shape
        self.nsteps += 1
        where = (self.nsteps, B, T, beta, self.form)
        snap = [getattr(st, n).clone() for n in SNAPSHOT]

        def against_oracle():
            torch.cuda.synchronize()
            sd = state_dict_of(st, snap[0])
            xc, uc, Lc = x.cpu(), u.cpu(), torch.as_tensor(L).cpu()
            check_loss_vs_fp64(sd, xc, uc, Lc, beta, self.dims, st.loss.item())
            check_state_vs_oracle(sd, xc, uc, Lc, beta, st, rtol_norm=ORACLE_RTOL)

        assert not oracle or self.form == "split"
        self._run(st, x, u, L, beta, against_oracle if oracle else None)
        fresh = self._state()
        for n, v in zip(SNAPSHOT, snap):
            getattr(fresh, n).copy_(v)
        poison_workspace(fresh, B, T)
        self._run(fresh, x, u, L, beta)
        torch.cuda.synchronize()
        for n in COMPARED:
            a, b = getattr(st, n), getattr(fresh, n)
            assert torch.equal(a, b), (where, n, "streamed != fresh",
                                       (a.double() - b.double()).abs().max().item() if a.numel() else None)
        assert int(st.step_dev.item()) == self.nsteps
        st.check_status()
        fresh.check_status()
        self.losses.append(st.loss.item())

    def take_epoch(self):
        """epoch_acc, which must be the fp64 sum, in order, of the per-step float losses exactly (Trainer's
        docstring: "same double-precision sum of the same per-step losses as loss.item()"); zeroes it as
        train_model does at the start of an epoch."""
        acc = 0.0
        for v in self.losses:
            acc += v
        got = self.st.epoch_acc.item()
        assert got == acc, (got, acc)
        self.st.epoch_acc.zero_()
        self.losses = []
        return got

    def final(self):
        torch.cuda.synchronize()
        return {n: getattr(self.st, n).cpu().clone() for n in ("flat", "exp_avg", "exp_avg_sq")}
