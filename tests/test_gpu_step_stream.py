"""The training step on streams of differently shaped batches (tests/step_stream.py has the tables and the checker).

1. test_*_stream_is_history_free: one long-lived TrainState goes through a table of (B, T, beta) with new data
   every step; every step is repeated from a snapshot of (flat, exp_avg, exp_avg_sq, step_dev) on a fresh
   TrainState whose workspace is NaN-filled, and loss, grad, flat, both moments and step_dev must be equal bit for
   bit, check_status() clean on both, and epoch_acc the exact in-order fp64 sum of the float losses.  The strip
   stream (cfg2's dims) sits on the strip kernels' row-count edges and revisits (96, 150) twice, the first
   time with another beta; the short streams run the other kernel families.  Five step forms; the ones
   README.md documents as bit-identical (fused, split, overlap, graph) must also end a stream on the same flat
   and moments.
2. In the split form, the revisits and the "last batch" of the strip stream and the first revisit of every short
   stream also meet the fp64 oracle at the streamed state's own pre-step parameters (ReLU-mask rule, gradients
   1e-5 normwise on the device's branch, loss 1e-5), and test_step_vs_oracle_at_beta does so on a fresh model
   at beta = 0, 0.25 and 0.5 (the single-step oracle tests elsewhere all pass beta = 1).
3. test_loader_epochs_replay: two epochs of train_model() through DeviceChunkLoader (T varying, a last batch of
   104), the recorded batches replayed through the checker: same final parameters bit for bit, same printed
   epoch losses.

The tests without the gpu mark hold every row of the tables to the launchers' arithmetic and to the dispatch
(host-only queries), so the streams cannot drift off the strip counts and kernel families they are there for.
"""
import contextlib
import io
import random

import pytest
import torch

import step_stream as S
import width_cases as W

_FUSED = {}  # (case name, the step numbers run) -> the fused form's final flat and moments


def _stream_of(name, form):
    return S.strip_stream(form) if name == "strip" else S.short_stream()


def _dims_of(name):
    return S.STRIP_DIMS if name == "strip" else S.SHORT_DIMS[name]


def _drive(name, form, steps):
    """The steps [(k, Step)] of a case's stream in a form, every step checked -> the final flat and moments."""
    dims = _dims_of(name)
    chk = S.StreamChecker(dims, form)
    for k, s in steps:
        x, u, L = S.stream_batch(dims, s.B, s.T, k)
        chk.step(x, u, L, s.beta, oracle=s.oracle and form == "split")
    chk.take_epoch()
    return chk.final()


def _check_stream(name, form):
    """The stream in a form; the forms README.md documents as bit-identical also end on the fused form's flat and
    moments (of the same steps: the strip stream's fused-only step is left out of that comparison's fused run)."""
    steps = _stream_of(name, form)
    key = (name, tuple(k for k, _ in steps))
    got = _drive(name, form, steps)
    if form == "fused":
        _FUSED[key] = got
    elif form in S.SAME_BITS:
        if key not in _FUSED:
            _FUSED[key] = _drive(name, "fused", steps)
        for n, v in _FUSED[key].items():
            assert torch.equal(got[n], v), (n, "differs from the fused form's")


# ------------------------------------------------------------------ host-only: the tables sit where they claim
@pytest.mark.parametrize("k", range(1, len(S.STRIP_STREAM) + 1))
def test_strip_stream_geometry(k):
    S.check_strip_row(S.STRIP_STREAM[k - 1])


def test_strip_stream_shape():
    """The table as a whole: two revisits of (96, 150), train_model's warm-up values for beta, one fused-only
    step, the oracle steps cheap enough for the fp64 CPU oracle."""
    bt = [(s.B, s.T) for s in S.STRIP_STREAM]
    assert bt == [(96, 150), (5, 71), (96, 150), (310, 198), (1, 5), (25, 39), (104, 57), (96, 150)]
    assert [s.beta for s in S.STRIP_STREAM] == [0.25, 0.5, 0.5, 0.75, 1.0, 1.0, 0.25, 0.5]
    # (96, 150) comes back with another beta, and once more with a beta it has already seen (the graph form
    # replays one captured graph for both of those visits)
    assert [s.beta for s in S.STRIP_STREAM if (s.B, s.T) == (96, 150)] == [0.25, 0.5, 0.5]
    assert [k for k, s in enumerate(S.STRIP_STREAM, 1) if s.fused_only] == [4]
    assert [k for k, s in enumerate(S.STRIP_STREAM, 1) if s.oracle] == [3, 7, 8]
    assert all(s.R <= 14592 for s in S.STRIP_STREAM if s.oracle)
    assert max(s.most for s in S.STRIP_STREAM) == 3 and any(s.bwd == 256 for s in S.STRIP_STREAM)
    assert [k for k, _ in S.strip_stream("split")] == [1, 2, 3, 5, 6, 7, 8]


@pytest.mark.parametrize("k", range(1, len(S.STRIP_STREAM) + 1))
def test_strip_stream_runs_the_strips(k):
    s = S.STRIP_STREAM[k - 1]
    assert S.runs_the_strips(S.STRIP_DIMS, s.B, s.T)


@pytest.mark.parametrize("name", list(S.SHORT_DIMS))
def test_short_stream_families(name):
    """The short streams' dims run the kernel families they are here for; the width_cases rows as a whole."""
    dims = S.SHORT_DIMS[name]
    got = W.stage_families(dims, 7, 90)
    for stage, fam in S.SHORT_FAMILIES[name]:
        assert got[stage] == fam, (stage, got[stage])
    if name in W.BY_NAME:
        c = W.BY_NAME[name]
        assert (c.B, c.T) == (7, 90) and got == c.families
    for B, T, _ in S.SHORT_STREAM:
        assert not any("unsupported" in f for f in W.stage_families(dims, B, T).values())
    assert len({(B, T) for B, T, _ in S.SHORT_STREAM}) == 3
    assert len({beta for B, T, beta in S.SHORT_STREAM if (B, T) == (7, 90)}) == 2


def test_stream_lengths_are_ragged():
    for B, T in [(s.B, s.T) for s in S.STRIP_STREAM] + [c[:2] for c in S.SHORT_STREAM] + [(40, 77)]:
        L = S.stream_lengths(B, T, 1).tolist()
        assert L[:min(B, 9)] == list(W._lengths(B, T)) and all(1 <= n <= T for n in L)
        if B >= 3:
            assert {T, 1, 2} <= set(L)
        if B > 9:
            assert len(set(L[9:])) > 1 and L != S.stream_lengths(B, T, 2).tolist()


# ------------------------------------------------------------------------------- 1. history-free, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("form", S.FORMS)
def test_strip_stream_is_history_free(form):
    for _, s in S.strip_stream(form):
        assert S.runs_the_strips(S.STRIP_DIMS, s.B, s.T)
    _check_stream("strip", form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("name", list(S.SHORT_DIMS))
def test_short_stream_is_history_free(name, form):
    _check_stream(name, form)


# ------------------------------------------------------------------------- 2. the oracle at beta != 1
@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("name,B,T", [("strip", 40, 77), ("d17_k8", 7, 90)])
def test_step_vs_oracle_at_beta(name, B, T, beta):
    """One forward_backward of a fresh model on a NaN-filled workspace at beta < 1: check_step_vs_oracle's
    ReLU-mask rule and gradients (1e-5 normwise of the fp64 oracle on the device's branch, 1e-4 elementwise of
    the largest), the loss within 1e-5 of the fp64 oracle, everything finite.  At beta = 0 the KL term is gone:
    the oracle's gradients of the Prior's five parameters are exactly zero and the device's must be too
    (assert_grad_close's rule for a zero reference)."""
    import vqhmm
    from test_gpu_configs import check_state_vs_oracle, poison_workspace
    dims = _dims_of(name)
    m, sd, x, u, L = W.step_inputs(dims, B, T, seed=900 + B, lengths=S.stream_lengths(B, T, 901 + B))
    st = vqhmm.TrainState(m.cuda(), lr=1e-3)
    xs, us, Ls = st.prepare(x, u, L)
    poison_workspace(st, B, T)
    st.forward_backward(xs, us, Ls, beta)
    torch.cuda.synchronize()
    st.check_status()
    assert torch.isfinite(st.loss).item() and torch.isfinite(st.grad).all().item()
    S.check_loss_vs_fp64(sd, x, u, L, beta, dims, st.loss.item())
    _, p64 = check_state_vs_oracle(sd, x, u, L, beta, st, rtol_norm=S.ORACLE_RTOL)
    if beta == 0.0:
        for n in vqhmm.PARAM_ORDER:
            assert (n.startswith("prior.") and not p64[n].grad.any()) or \
                (not n.startswith("prior.") and p64[n].grad.any()), n


# ------------------------------------------------------------------------- 3. one epoch through the real loader
class _Recording:
    """A loader that clones every batch as it goes by."""

    def __init__(self, loader):
        self.loader, self.seen = loader, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for x, u, L in self.loader:
            self.seen.append((x.clone(), u.clone(), L.clone()))
            yield x, u, L


@pytest.mark.gpu
def test_loader_epochs_replay():
    """train_model() for two epochs over DeviceChunkLoader(RandomChunkDataset, 128): 8 batches an epoch, T the
    batch's longest chunk, the last batch 104 sequences.  The 16 recorded batches replayed through the checker in
    the fused form with train_model's beta schedule: every step history-free, the final parameters train_model's
    bit for bit, each printed epoch loss the replay's epoch_acc / 8 in the same format."""
    import vqhmm
    from vqhmm.data import DeviceChunkLoader, RandomChunkDataset
    D, H, K, H2, U, TH = S.STRIP_DIMS
    gen = torch.Generator().manual_seed(17)
    xs = [torch.randn(D, 300, generator=gen) for _ in range(6)]
    us = [torch.randn(U, 300, generator=gen) for _ in range(6)]
    ds = RandomChunkDataset(xs, us, min_len=20, max_len=60)
    random.seed(253)  # 128 draws from 20..60 nearly always reach 60: a seed whose 16 batch maxima take three values
    rec = _Recording(DeviceChunkLoader(ds, 128))
    epochs = 2
    torch.manual_seed(0)  # StreamChecker's init
    m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=U, trans_hidden=TH).cuda()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        vqhmm.train_model(m, rec, num_epochs=epochs)
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Epoch")]
    assert len(rec) == 8 and len(rec.seen) == 8 * epochs and len(lines) == epochs
    assert [x.shape[0] for x, _, _ in rec.seen] == ([128] * 7 + [104]) * epochs
    assert all(x.shape[2] == int(L.max()) for x, _, L in rec.seen)
    assert len({x.shape[2] for x, _, _ in rec.seen}) >= 3, [x.shape[2] for x, _, _ in rec.seen]
    for x, _, _ in rec.seen:
        assert S.runs_the_strips(S.STRIP_DIMS, x.shape[0], x.shape[2])

    chk = S.StreamChecker(S.STRIP_DIMS, "fused")
    it = iter(rec.seen)
    for ep in range(epochs):
        beta = min(1.0, 2.0 * (ep + 1) / epochs)
        for _ in range(len(rec)):
            chk.step(*next(it), beta)
        acc = chk.take_epoch()
        assert lines[ep] == f"Epoch {ep+1}/{epochs}, Loss: {acc/len(rec):.4f}", (lines[ep], acc / len(rec))
    trained = torch.cat([p.detach().reshape(-1) for p in m.ordered_parameters()]).cpu()
    assert torch.equal(chk.final()["flat"], trained)
