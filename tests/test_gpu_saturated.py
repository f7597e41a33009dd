"""The training step at saturated posteriors, saturated prior tables and clamped variances (tests/saturated_cases.py;
tests/test_saturated_ref.py proves on the host that the inputs are in the regime and the bounds reachable).

Every other test of the step runs a freshly initialised model or the briefly trained goldens: logvar near 0, no q
near 0 or 1, log_A above about -5.  Here, on every ELBO head (pipe, coop, mfma, scalar, two staged row kernels, the
head fused into the forward strip) and every softmax tail of the encoder's last convolution:

  a  default forms, LEVEL_MODERATE, with the variance edit alone and with all three edits: a poisoned TrainState's
     forward_backward at beta 1 against the fp64 oracle on the device's own ReLU masks
       loss, and recon / prior / entropy one by one (vqhmm_elbo_pieces; recon is ~1e7 here and would hide any
         error of the other two inside the total), within LOSS_RTOL;
       the ReLU masks and all 18 gradients by test_gpu_configs' rules at 1e-5 normwise;
       decoder.to_params' weight and bias gradient row by row (every mu row and every unclamped logvar row within
         1e-5 normwise, the weight row alone and joined with its bias entry, check_to_params_rows: over the whole
         tensor the 1e8-sized mu rows of the clamped channels swamp the rest);
       exactly: the logvar rows of the clamped channels (c % 5 < 2) have a zero bias gradient and an all-zero
         weight gradient (a clamped variance passes no gradient to logvar), and no gradient element is NaN or inf;
       compute_loss().backward() gives the same loss and gradient bits;
       on pipe_strip and coop_k8, two fused forward_backward_adam steps equal two forward_backward + apply_adam
         steps bit for bit.
  b  default forms, LEVEL_HARD, "logit" alone (more than 40 % of q exactly 0): loss, pieces and masks as in a.  The
     fp32 oracle itself is 1e-5 to 6e-5 from fp64 on the encoder gradients there (the cancellation in
     q ((lg - lse) - f)), so each gradient's bound is measured: e_ref is the fp32 oracle's normwise distance from
     the fp64 oracle, both on the device's masks, and the device must be within max(1e-5, 4 e_ref) of fp64.  The
     factor 4 is a judgement (another summation order, native exp / log against torch's), still far below the
     O(1) error of a mishandled zero q.  Both distances are printed per tensor (DESIGN.md records them).
  c  the switched forms (VQHMM_HEAD=coop / tile, VQHMM_STRIP_HEAD=1, VQHMM_STRIP=0, VQHMM_CONV_FUSE=0,
     VQHMM_STRIP_BWD=0 + VQHMM_STRIP_WGRAD=0), each in a fresh child process (the switches are read once per
     process) on pipe_strip at LEVEL_MODERATE with all three edits, held to the oracle by a's rules.  Two forms
     are not compared with each other: the oracle is the better judge where terms reach 1e8.
  d  inference at LEVEL_HARD: hard_regimes' regimes equal q.argmax(1) exactly, q.sum(1) is within 1e-6 of 1, and q
     is within 1e-6 of the fp64 softmax of the logits the same weights give on the device (model.encode).  From x,
     end to end, 1e-6 is out of fp32's reach at this level: logits of several hundred carry ~1e-4 of rounding,
     and the fp32 oracle's own q is 9e-6 (pipe_strip) and 1.8e-5 (coop_k8) from the fp64 oracle's.  That distance
     is held to the measured bound of b, max(1e-6, 4 e_ref), and printed.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model as RM
import saturated_cases as S
from test_gpu_configs import check_masks_grads_vs_oracle, check_masks_vs_oracle, poison_workspace, relu_masks
from test_gpu_model import LOSS_RTOL

pytestmark = pytest.mark.gpu

GRAD_RTOL = 1e-5
PIECES = ("recon", "prior", "entropy")
IDS = [c.name for c in S.CASES]
TP_W, TP_B = "decoder.to_params.weight", "decoder.to_params.bias"


def loss_pieces(st, B, T):
    """[recon, prior, entropy] of the TrainState's last step at (B, T), read from its workspace."""
    from vqhmm import _ext
    ws = st.workspace(B, T)
    p = ctypes.c_void_p()
    _ext.check(_ext.load().vqhmm_elbo_pieces(ctypes.byref(st.dims), B, T, _ext.ptr(ws), None, ctypes.byref(p)),
               "pieces")
    off = p.value - ws.data_ptr()
    return ws[off: off + 12].view(torch.float32).cpu().clone()


def model_of(dims, sd):
    import vqhmm
    D, H, K, H2, U, TH = dims
    m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=U, trans_hidden=TH)
    m.load_state_dict(sd)
    return m.cuda()


def run_step(dims, sd, x, u, L):
    """One forward_backward at beta 1 of a fresh TrainState on a NaN-filled workspace -> (the state, the prepared
    batch, dict(loss, pieces, grad, masks) on the host)."""
    import vqhmm
    B, _, T = x.shape
    st = vqhmm.TrainState(model_of(dims, sd), lr=1e-3)
    batch = st.prepare(x, u, L)
    poison_workspace(st, B, T)
    st.forward_backward(*batch, 1.0)
    torch.cuda.synchronize()
    st.check_status()
    out = dict(loss=st.loss.cpu().clone(), pieces=loss_pieces(st, B, T), grad=st.grad.cpu().clone(),
               masks=relu_masks(st, B, T))
    return st, batch, out


def oracle_terms(sd, x, u, L, dims, masks, dtype=torch.float64):
    with torch.no_grad():
        return RM.elbo_terms({k: v.to(dtype) for k, v in sd.items()}, x.to(dtype), u.to(dtype), L, dims[2], dims[4],
                             relu_masks=masks)


def check_loss_and_pieces(where, sd, x, u, L, dims, out):
    """The loss and its three pieces within LOSS_RTOL of the fp64 oracle on the device's masks."""
    t = oracle_terms(sd, x, u, L, dims, out["masks"])
    ref = {k: t[k].item() for k in PIECES}
    ref_loss = ref["recon"] + 1.0 * (ref["prior"] - ref["entropy"])
    loss = out["loss"].item()
    print(f"{where}: loss {loss!r} vs {ref_loss!r}: {abs(loss - ref_loss) / abs(ref_loss):.2e}")
    for k, got in zip(PIECES, out["pieces"].tolist()):
        print(f"{where}: {k} {got!r} vs {ref[k]!r}: {abs(got - ref[k]) / abs(ref[k]):.2e}")
    assert abs(loss - ref_loss) <= LOSS_RTOL * abs(ref_loss), (loss, ref_loss)
    for k, got in zip(PIECES, out["pieces"].tolist()):
        assert abs(got - ref[k]) <= LOSS_RTOL * abs(ref[k]), (k, got, ref[k])


def split_grad(grad, like):
    import vqhmm
    return {n: g.view_as(like[n]) for n, g in zip(vqhmm.PARAM_ORDER,
                                                  grad.split([like[n].numel() for n in vqhmm.PARAM_ORDER]))}


def check_to_params_rows(where, D, g, p64, what):
    """decoder.to_params' gradient row by row, and the clamped rows' exact zeros.  A row is an output channel's H
    weights and its bias entry, [dW[row] | db[row]], compared normwise as one vector: a lone bias entry is a sum
    of signed terms with no norm to be relative to (the fp32 oracle's own mu-row bias entries are up to 2.9e-5
    from fp64 as scalars); the weight row alone is held to the same bound."""
    gw, gb = g[TP_W].double().flatten(1), g[TP_B].double()
    rw, rb = p64[TP_W].grad.flatten(1), p64[TP_B].grad
    clamped = {D + c for c in S.clamped_channels(D)} if "var" in what else set()
    worst = 0.0
    for row in range(2 * D):
        if row in clamped:
            assert gb[row].item() == 0.0 and rb[row].item() == 0.0, (row, gb[row].item(), rb[row].item())
            assert not gw[row].any() and not rw[row].any(), row
            continue
        ew = ((gw[row] - rw[row]).norm() / max(rw[row].norm().item(), 1e-30)).item()
        got, ref = torch.cat([gw[row], gb[row:row + 1]]), torch.cat([rw[row], rb[row:row + 1]])
        er = ((got - ref).norm() / max(ref.norm().item(), 1e-30)).item()
        worst = max(worst, ew, er)
        assert ew <= GRAD_RTOL and er <= GRAD_RTOL, (row, ew, er)
    print(f"{where}: to_params rows, worst {worst:.2e}")


def print_grad_errors(where, sd, x, u, L, K, U, out):
    """Every gradient's normwise distance from the fp64 oracle on the device's masks, printed before any rule
    asserts (the figures DESIGN.md records)."""
    import vqhmm
    p64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    RM.elbo(p64, x.double(), u.double(), L, 1.0, K, U, relu_masks=out["masks"]).backward()
    g = split_grad(out["grad"], p64)
    errs = {n: ((g[n].double() - p64[n].grad).norm() / max(p64[n].grad.norm().item(), 1e-30)).item()
            for n in vqhmm.PARAM_ORDER}
    worst = max(errs, key=errs.get)
    print(f"{where}: gradients, worst {errs[worst]:.2e} ({worst}); " + " ".join(f"{e:.1e}" for e in errs.values()))


def check_against_oracle(where, case, sd, x, u, L, out, what):
    """a's rules for one step's saved outputs (host tensors) -> the fp64 parameters with the oracle's gradient."""
    D, K, U = case.dims[0], case.dims[2], case.dims[4]
    assert torch.isfinite(out["grad"]).all(), where
    check_loss_and_pieces(where, sd, x, u, L, case.dims, out)
    print_grad_errors(where, sd, x, u, L, K, U, out)
    p64 = check_masks_grads_vs_oracle(sd, x, u, L, 1.0, K, U, out["masks"], out["grad"], rtol_norm=GRAD_RTOL)
    check_to_params_rows(where, D, split_grad(out["grad"], p64), p64, what)
    return p64


# ----------------------------------------------------------------------------------------- a: default forms
@pytest.mark.parametrize("what", [("var",), ("var", "logit", "trans")], ids=["var", "all"])
@pytest.mark.parametrize("name", IDS)
def test_moderate_step_vs_oracle(name, what):
    case = S.BY_NAME[name]
    S.check_families(case)
    m, sd, x, u, L = S.saturated_inputs(case, S.LEVEL_MODERATE, what)
    st, _, out = run_step(case.dims, sd, x, u, L)
    check_against_oracle(f"{name}/{'+'.join(what)}", case, sd, x, u, L, out, what)
    # the autograd surface: same loss and gradient bits
    mg = m.cuda()
    loss = mg.compute_loss(x.cuda(), u.cuda(), L, 1.0)
    loss.backward()
    assert loss.item() == st.loss.item()
    for i, prm in enumerate(mg.ordered_parameters()):
        assert torch.equal(st.grad[st.off[i]:st.off[i + 1]].view_as(prm), prm.grad), i


@pytest.mark.parametrize("name", ["pipe_strip", "coop_k8"])
def test_moderate_fused_adam_bit_identical(name):
    """Two forward_backward_adam steps against two forward_backward + apply_adam steps from the same saturated
    state (test_fused_tail_adam_bit_identical's rule at default init)."""
    import vqhmm
    case = S.BY_NAME[name]
    _, sd, x, u, L = S.saturated_inputs(case, S.LEVEL_MODERATE, S.ALL)
    fused, split = (vqhmm.TrainState(model_of(case.dims, sd), lr=1e-3) for _ in range(2))
    batch = fused.prepare(x, u, L)
    for _ in range(2):
        fused.forward_backward_adam(*batch, 1.0)
        split.forward_backward(*batch, 1.0)
        split.apply_adam()
    torch.cuda.synchronize()
    fused.check_status()
    split.check_status()
    for n in ("flat", "exp_avg", "exp_avg_sq", "grad"):
        a, b = getattr(fused, n), getattr(split, n)
        assert torch.isfinite(a).all(), n
        assert torch.equal(a, b), n
    assert int(fused.step_dev.item()) == int(split.step_dev.item()) == 2


# ------------------------------------------------------------------------------------ b: LEVEL_HARD, logits
@pytest.mark.parametrize("name", ["pipe_strip", "coop_k8", "staged_k32", "scalar_u8"])
def test_hard_logits_step_vs_oracle(name):
    import vqhmm
    case = S.BY_NAME[name]
    K, U = case.dims[2], case.dims[4]
    S.check_families(case)
    _, sd, x, u, L = S.saturated_inputs(case, S.LEVEL_HARD, ("logit",))
    _, _, out = run_step(case.dims, sd, x, u, L)
    assert torch.isfinite(out["grad"]).all()
    check_loss_and_pieces(f"{name}/hard", sd, x, u, L, case.dims, out)
    check_masks_vs_oracle(sd, x, out["masks"])
    p64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    p32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    RM.elbo(p64, x.double(), u.double(), L, 1.0, K, U, relu_masks=out["masks"]).backward()
    RM.elbo(p32, x, u, L, 1.0, K, U, relu_masks=out["masks"]).backward()
    g = split_grad(out["grad"], p64)
    bad = []
    for n in vqhmm.PARAM_ORDER:
        r = p64[n].grad
        nr = max(r.norm().item(), 1e-30)
        e_ref = ((p32[n].grad.double() - r).norm() / nr).item()
        e_dev = ((g[n].double() - r).norm() / nr).item()
        print(f"{name}/hard: {n:32s} e_ref {e_ref:.2e}  device {e_dev:.2e}")
        if not e_dev <= max(GRAD_RTOL, 4 * e_ref):
            bad.append((n, e_dev, e_ref))
    assert not bad, bad


# --------------------------------------------------------------------------------------- c: switched forms
# form -> (environment, the (stage, family) pairs it must move pipe_strip to, as the child's library reports them).
# VQHMM_CONV_FUSE=0 alone moves no launch at these dims (the strips come before the fused pairs); with the strips
# off too (the last form) it reaches conv2's two-launch path and its fused softmax / to_params tails.
FORMS = {
    "head_coop": ({"VQHMM_HEAD": "coop"}, (("head", "coop"),)),
    "head_tile": ({"VQHMM_HEAD": "tile"}, (("head", "mfma"),)),
    "strip_head": ({"VQHMM_STRIP_HEAD": "1"}, (("head", "strip_fwd"),)),
    "no_strip": ({"VQHMM_STRIP": "0", "VQHMM_STRIP_HEAD": "0"}, (("enc2", "fused_pair"), ("dec2", "fused_pair"))),
    "no_conv_fuse": ({"VQHMM_CONV_FUSE": "0"}, (("enc2", "strip_fwd"), ("head", "pipe"))),
    "no_strip_bwd": ({"VQHMM_STRIP_BWD": "0", "VQHMM_STRIP_WGRAD": "0"},
                     (("par_dg", "fused_pair"), ("dec1_dg", "bwd_pair"), ("w_enc1", "wgrad2_group"))),
    "no_strips_no_conv_fuse": ({"VQHMM_STRIP": "0", "VQHMM_STRIP_HEAD": "0", "VQHMM_STRIP_BWD": "0",
                                "VQHMM_STRIP_WGRAD": "0", "VQHMM_CONV_FUSE": "0"},
                               (("enc2", "conv2"), ("dec2", "conv2"), ("dec1_dg", "conv2+logits_bwd+logits_dg"))),
}

_CHILD = r"""
import sys, torch
sys.path[:0] = sys.argv[1:4]
from test_gpu_saturated import run_step
from width_cases import stage_families
inp = torch.load(sys.argv[4], weights_only=True)
_, _, out = run_step(tuple(inp["dims"]), inp["sd"], inp["x"], inp["u"], inp["L"])
out["families"] = stage_families(tuple(inp["dims"]), *inp["x"].shape[::2])
torch.save(out, sys.argv[5])
"""


@pytest.fixture(scope="module")
def switched_inputs(tmp_path_factory):
    case = S.BY_NAME["pipe_strip"]
    _, sd, x, u, L = S.saturated_inputs(case, S.LEVEL_MODERATE, S.ALL)
    f = str(tmp_path_factory.mktemp("saturated") / "inputs.pt")
    torch.save(dict(dims=list(case.dims), sd=sd, x=x, u=u, L=L), f)
    return case, sd, x, u, L, f


@pytest.mark.parametrize("form", list(FORMS))
def test_switched_form_vs_oracle(tmp_path, switched_inputs, form):
    from conftest import PKG_DIR, ROOT
    case, sd, x, u, L, f_in = switched_inputs
    f_out = str(tmp_path / "out.pt")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, PKG_DIR, os.path.join(ROOT, "tests"), f_in, f_out],
                   check=True, timeout=300, env=dict(os.environ, **FORMS[form][0]))
    out = torch.load(f_out, weights_only=True)
    for stage, fam in FORMS[form][1]:
        assert out["families"][stage] == fam, (stage, out["families"][stage], fam)
    check_against_oracle(f"pipe_strip/{form}", case, sd, x, u, L, out, S.ALL)


# --------------------------------------------------------------------------------------------- d: inference
@pytest.mark.parametrize("name", ["pipe_strip", "coop_k8"])
def test_hard_inference(name):
    import vqhmm
    case = S.BY_NAME[name]
    m, sd, x, u, L = S.saturated_inputs(case, S.LEVEL_HARD, ("logit",))
    mg = m.cuda()
    reg, q = vqhmm.hard_regimes(mg, x.cuda())
    with torch.no_grad():
        logits = mg.encode(x.cuda())
    assert torch.equal(reg, q.argmax(dim=1))
    assert torch.isfinite(q).all() and (q == 0).float().mean().item() > 0.4
    assert (q.sum(dim=1).double() - 1).abs().max().item() <= 1e-6
    q_dev = F.softmax(logits.double(), dim=1).cpu()
    err = (q.cpu().double() - q_dev).abs().max().item()
    q64 = F.softmax(RM.encoder_logits({k: v.double() for k, v in sd.items()}, x.double()), dim=1)
    q32 = F.softmax(RM.encoder_logits(sd, x), dim=1)
    e_ref = (q32.double() - q64).abs().max().item()
    e_dev = (q.cpu().double() - q64).abs().max().item()
    print(f"{name}/hard: q vs fp64 softmax of the device's logits {err:.2e}; from x: fp32 oracle {e_ref:.2e}, "
          f"device {e_dev:.2e}")
    assert err <= 1e-6
    assert e_dev <= max(1e-6, 4 * e_ref)
