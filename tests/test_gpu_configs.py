"""BASELINE configs beyond cfg2, at the shapes the bench and the DP split run them
(BASELINE.json configs[2..4], SURVEY.md §8 "cfg3/cfg4"):

  cfg4 shard   K=8, D=16, H=64, H2=32, one rank's 512 x T=512 of the 4096-sequence batch:
               the training step (loss vs the fp32 oracle, 18 grads vs the fp64 oracle on
               the device's own ReLU branch, see check_step_vs_oracle), and the forward-
               backward / Viterbi on the model's own tables at that shape.
  cfg3 dims    K=32, D=64, H=256, H2=128 (the 256-channel generic conv, the staged ELBO
               head) at a small B x T: loss + grads vs the oracle, and a train step.

Tolerances: loss rel 1e-5; grads normwise 2e-6 vs fp64 on the device's ReLU branch.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle, hmm_ref
from oracle import ref_model as RM
from test_gpu_model import LOSS_RTOL, assert_grad_close

pytestmark = pytest.mark.gpu


def relu_masks(st, B, T):
    """The device forward's own ReLU patterns (h1, h2, g1, g2) as CF bool tensors, read
    from its workspace (vqhmm_elbo_debug_buffers)."""
    import ctypes
    from vqhmm import _ext
    ws = st.workspace(B, T)
    ptrs = (ctypes.c_void_p * 16)()
    _ext.check(_ext.load().vqhmm_elbo_debug_buffers(ctypes.byref(st.dims), B, T, _ext.ptr(ws), ptrs), "debug")
    d = st.dims
    out = []
    for i, c in ((1, d.hidden_dim), (2, d.hidden_dim2), (5, d.hidden_dim), (6, d.hidden_dim)):
        ld = (c + 3) // 4 * 4
        off = ptrs[i] - ws.data_ptr()
        v = ws[off: off + B * (T + 2) * ld * 4].view(torch.float32).view(B, T + 2, ld)[:, 1:T + 1, :c]
        out.append((v > 0).permute(0, 2, 1).cpu())
    return out


def poison_workspace(st, B, T):
    """Fill the step's workspace with quiet-NaN floats (0x7fc00000 in every word) and zero the status word
    again.  Every field of the workspace (api.hip plan_elbo's carve list) is written by the step before the
    step reads it: the float buffers and slabs by the launches that produce them; the two integer fields are
    `cnt`, which the prologue writes (need_grad = 2, no norm) before the head and the tail's loss finalize read
    it and which no launch reads otherwise, and `sync`, of which no kernel reads or writes anything but the
    status word, whose bits are only ever set.  So nothing stays unpoisoned but that word."""
    ws = st.workspace(B, T)
    ws[: ws.numel() // 4 * 4].view(torch.int32).fill_(0x7FC00000)
    for word in st._status.values():
        word.zero_()
    return ws


def check_masks_vs_oracle(sd, x, masks):
    """check_step_vs_oracle's `masks` rule: a step's ReLU patterns (relu_masks' CF bool tensors, on the host)
    against the fp64 oracle's own decisions at the parameters sd (a CPU state dict)."""
    for name, mk, pre in zip(("enc conv1", "enc conv2", "dec conv1", "dec conv2"), masks,
                             RM.preactivations({k: v.detach().double() for k, v in sd.items()}, x.double())):
        diff = mk != (pre > 0)
        nd = int(diff.sum())
        assert nd <= max(4, int(1e-6 * pre.numel())), f"{name}: {nd} ReLU decisions differ from the oracle's"
        if nd:
            worst = pre[diff].abs().max().item() / max(pre.abs().max().item(), 1e-30)
            assert worst <= 1e-4, f"{name}: a flipped ReLU decision at |pre| = {worst:.2e} of the layer max"


def check_masks_grads_vs_oracle(sd, x, u, L, beta, K, U, masks, grad, rtol_norm=2e-6):
    """check_step_vs_oracle's `masks` and `grads` rules for a step's ReLU patterns `masks` (relu_masks' CF bool
    tensors) and flat gradient `grad` (vqhmm_param_layout order: the 18 tensors of PARAM_ORDER back to back), on
    the device or the host, e.g. as a child process saved them.  sd, x, u, L: CPU.  Returns the fp64 parameters,
    whose .grad is the oracle's gradient on the given branch."""
    import vqhmm
    p64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    sizes = [p64[name].numel() for name in vqhmm.PARAM_ORDER]
    assert grad.numel() == sum(sizes)
    check_masks_vs_oracle(sd, x, masks)
    RM.elbo(p64, x.double(), u.double(), L, beta, K, U, relu_masks=masks).backward()
    for name, g in zip(vqhmm.PARAM_ORDER, grad.split(sizes)):
        assert_grad_close(g.view_as(p64[name]).cpu().numpy(), p64[name].grad.numpy(), name, rtol_norm=rtol_norm,
                          rtol_max=10 * rtol_norm)
    return p64


def check_state_vs_oracle(sd, x, u, L, beta, st, rtol_norm=2e-6):
    """check_masks_grads_vs_oracle for a TrainState that has just run forward_backward on the batch (x, u, L: CPU
    tensors) with the KL weight beta, from the parameters sd (a CPU state dict: the state's parameters BEFORE
    the step, so an Adam update in the same launch does not matter).  Returns the device's ReLU patterns and the
    fp64 parameters, whose .grad is the oracle's gradient on the device's branch."""
    B, _, T = x.shape
    masks = relu_masks(st, B, T)
    assert st.off[-1] == st.grad.numel()
    return masks, check_masks_grads_vs_oracle(sd, x, u, L, beta, st.dims.K, st.dims.u_dim, masks, st.grad,
                                              rtol_norm=rtol_norm)


def check_step_vs_oracle(dims, B, T, seed, full_frac=0.5, rtol_norm=2e-6, independent=False, lengths=None,
                         poison=False):
    """The training step (loss + 18 grads) at (B, T) vs the oracle:
      loss   within 1e-5 relative of the fp32 CPU oracle (the reference's arithmetic);
      grads  within 2e-6 normwise of the fp64 oracle evaluated on the device forward's own
             ReLU branch (RM.elbo relu_masks).  Two correct fp32 forwards put a few of the
             ~1e7 pre-activations on different sides of 0, which alone moves the grads by
             ~1e-5 (tools/stage_accuracy.py: 1-2 flips per layer, cpu-fp32 has its own);
             on a fixed branch the device grads sit ~2e-7 from fp64 (64-channel layers;
             the 256-channel layers' 768-term fp32 chains are held to 1e-5).
      masks  the device's ReLU patterns against the fp64 oracle's OWN decisions: at most
             max(4, 1e-6 of the elements) differ per layer, each at a pre-activation within
             1e-4 of 0 relative to the layer's largest |pre-activation| (a forward bug that
             flips or zeroes activations cannot hide behind the branch-conditioned oracle).
      independent=True: also every gradient against the fp32 CPU oracle's autograd on ITS
             own branch (round 1's check, no device information used): 1e-5 normwise where the
             fp32 oracle's ReLU decisions equal the device's, 5e-5 where a few differ (counted and
             bounded like the fp64 masks: each flip sits at a pre-activation within fp32 rounding
             of 0 and moves a gradient by ~1e-5; the cfg4 shard's encoder.conv1 grad measured
             2.7e-5 with such flips).
    The autograd surface (compute_loss + backward) must give the same bits as TrainState.
      lengths=  the batch's lengths instead of the random draw;
      poison=True: TrainState's workspace is NaN-filled before its step (poison_workspace), so a kernel that
             reads a pad column, pad row or slab entry nobody wrote this step shows as a NaN."""
    import vqhmm
    from width_cases import step_inputs
    D, H, K, H2, U, TH = dims
    m, sd, x, u, L = step_inputs(dims, B, T, seed, full_frac, lengths)
    p32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = RM.elbo(p32, x, u, L, 1.0, K, U)
    ref_loss = ref.item()
    if independent:
        ref.backward()

    mg = m.cuda()
    loss = mg.compute_loss(x.cuda(), u.cuda(), L, 1.0)
    loss.backward()
    auto = {n: prm.grad.clone() for n, prm in mg.named_parameters()}
    st = vqhmm.TrainState(mg, lr=1e-3)
    xs, us, Ls = st.prepare(x, u, L)
    if poison:
        poison_workspace(st, B, T)
    st.forward_backward(xs, us, Ls, 1.0)
    torch.cuda.synchronize()
    if poison:
        st.check_status()
    assert abs(st.loss.item() - ref_loss) <= LOSS_RTOL * abs(ref_loss), (st.loss.item(), ref_loss)
    assert st.loss.item() == loss.item()
    masks, p64 = check_state_vs_oracle(sd, x, u, L, 1.0, st, rtol_norm=rtol_norm)
    rtol_ind = 1e-5
    if independent:  # the fp32 oracle's own ReLU decisions against the device's
        nflip = 0
        for name, mk, pre in zip(("enc conv1", "enc conv2", "dec conv1", "dec conv2"), masks,
                                 RM.preactivations({k: v.detach() for k, v in p32.items()}, x)):
            diff = mk != (pre > 0)
            nd = int(diff.sum())
            nflip += nd
            assert nd <= max(4, int(1e-6 * pre.numel())), f"{name}: {nd} ReLU decisions differ from the fp32 oracle's"
        rtol_ind = 1e-5 if nflip == 0 else 5e-5
    for i, name in enumerate(vqhmm.PARAM_ORDER):
        g = st.grad[st.off[i]:st.off[i + 1]].view_as(auto[name])
        assert torch.equal(g, auto[name]), name
        if independent:
            assert_grad_close(g.cpu().numpy(), p32[name].grad.numpy(), name + " (fp32 oracle, own branch)",
                              rtol_norm=rtol_ind, rtol_max=1.0)


def test_cfg4_shard_train_step_vs_oracle():
    """One rank's shard of cfg4 (4096 sequences over 8 GPUs = 512 x T=512, K=8, D=16)."""
    check_step_vs_oracle((16, 64, 8, 32, 4, 128), 512, 512, seed=4096, independent=True)


def test_cfg4_shard_hmm_on_model_tables():
    """Forward-backward and Viterbi at the cfg4 shard shape on the model's own tables:
    gamma within 1e-5 of the fp64 oracle and bit-exact paths on a slice of the batch
    (the kernels run on the whole 512 x 512 x K8 batch)."""
    import vqhmm
    torch.manual_seed(0)
    m = vqhmm.VAE_HMM(16, 64, 8, 32, u_dim=4, trans_hidden=128).cuda()
    gen = torch.Generator(device="cuda").manual_seed(8)
    B, T = 512, 512
    x = torch.randn(B, 16, T, device="cuda", generator=gen)
    u = torch.randn(B, 4, T, device="cuda", generator=gen)
    L = torch.full((B,), T, dtype=torch.int64)
    L[1::7] = torch.arange(1, T, 7)[: L[1::7].numel()]
    with torch.no_grad():
        em = torch.log_softmax(m.encode(x), dim=1).transpose(1, 2).contiguous()
        log_pi, log_A = m.prior(u)
    gamma, logZ = vqhmm.forward_backward(log_pi, log_A, em, L)
    path, score = vqhmm.viterbi(log_pi, log_A, em, L)
    sl = slice(0, 512, 37)
    lp, la, e = log_pi.cpu().numpy(), log_A[sl].cpu().numpy(), em[sl].cpu().numpy()
    rg, rz = hmm_ref.forward_backward_f64(lp, la, e, L[sl].numpy())
    assert np.abs(gamma[sl].cpu().numpy() - rg).max() <= 1e-5
    assert np.all(np.abs(logZ[sl].cpu().numpy() - rz) <= 1e-5 * np.maximum(1.0, np.abs(rz)))
    rp, rs = c_oracle.viterbi(lp, la, e, L[sl].numpy())
    assert np.array_equal(path[sl].cpu().numpy(), rp)
    assert np.array_equal(score[sl].cpu().numpy().view(np.uint32), rs.view(np.uint32))


def test_cfg3_dims_train_step_vs_oracle():
    """cfg3 model dims (K=32, D=64, H=256, H2=128, TH=128) at a small B x T."""
    check_step_vs_oracle((64, 256, 32, 128, 4, 128), 6, 64, seed=2048, rtol_norm=1e-5)


def test_cfg3_dims_train_step_b64_t200_vs_oracle():
    """cfg3 model dims at B = 64, T = 200 (25.6k rows: every wide-conv and wide-wgrad launch runs many
    row tiles and several row chunks, ragged lengths)."""
    check_step_vs_oracle((64, 256, 32, 128, 4, 128), 64, 200, seed=2049, rtol_norm=1e-5)


@pytest.mark.timeout(600)
def test_cfg3_full_size_train_step_vs_oracle():
    """cfg3 at its full per-GPU size (BASELINE configs[2]: B = 2048, T = 200, K = 32, D = 64, H = 256,
    H2 = 128; 414k PCL rows, so convbig's grid, wgradbig's row chunks and the staged head run exactly as the
    bench runs them), ragged lengths: the loss within 1e-5 of the fp32 CPU oracle and every gradient within
    5e-5 normwise of the oracle's own autograd (its own ReLU branch: a handful of the ~1e8 pre-activations
    sit within fp32 rounding of 0 on either side).  The oracle step takes ~15 s on the box's host."""
    import vqhmm
    D, H, K, H2, U, TH = 64, 256, 32, 128, 4, 128
    B, T = 2048, 200
    torch.manual_seed(0)
    m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=U, trans_hidden=TH)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, D, T, generator=gen)
    u = torch.randn(B, U, T, generator=gen)
    L = torch.randint(20, T + 1, (B,), generator=gen)
    L[: B // 2] = T
    mg = m.cuda()
    loss = mg.compute_loss(x.cuda(), u.cuda(), L, 1.0)
    loss.backward()
    got = {n: prm.grad.detach().cpu().double() for n, prm in mg.named_parameters()}
    dev_loss = loss.item()
    del mg, loss
    torch.cuda.empty_cache()
    p32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = RM.elbo(p32, x, u, L, 1.0, K, U)
    assert abs(dev_loss - ref.item()) <= LOSS_RTOL * abs(ref.item()), (dev_loss, ref.item())
    ref.backward()
    for name in vqhmm.PARAM_ORDER:
        r = p32[name].grad.double()
        err = ((got[name] - r).norm() / max(r.norm().item(), 1e-30)).item()
        assert err <= 5e-5, f"{name}: {err:.2e}"


def test_cfg3_dims_adam_steps_vs_oracle():
    """Three fused-Adam steps at cfg3 dims track torch.optim.Adam on the oracle."""
    import vqhmm
    D, H, K, H2, U, TH = 64, 256, 32, 128, 4, 128
    torch.manual_seed(0)
    m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=U, trans_hidden=TH)
    gen = torch.Generator().manual_seed(5)
    B, T = 4, 48
    x = torch.randn(B, D, T, generator=gen)
    u = torch.randn(B, U, T, generator=gen)
    L = torch.tensor([48, 48, 30, 17])
    p = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    opt = torch.optim.Adam([p[k] for k in RM.PARAM_ORDER], lr=1e-3)
    mg = m.cuda()
    st = vqhmm.TrainState(mg, lr=1e-3)
    for _ in range(3):
        opt.zero_grad()
        RM.elbo(p, x, u, L, 1.0, K, U).backward()
        opt.step()
        st.step(x.cuda(), u.cuda(), L, 1.0)
    sd = mg.state_dict()
    lr_steps = 3e-3
    for k in RM.PARAM_ORDER:
        ref = p[k].detach().numpy().astype(np.float64)
        diff = np.abs(sd[k].cpu().numpy() - ref) - 2e-7 * np.abs(ref)
        # Adam moves each element by <= ~lr per step whatever |g| is, so an element whose
        # gradient is within fp32 summation noise of 0 may step the other way: allow at
        # most 1e-4 of the elements past 1% of the cumulative step, and bound the mean
        assert (diff > 1e-2 * lr_steps).mean() <= 1e-4, (k, diff.max())
        assert diff.max() <= 2 * lr_steps, (k, diff.max())
        assert diff.mean() <= 1e-4 * lr_steps, (k, diff.mean())
