"""CPU checks of the width sweep's case table (tests/width_cases.py), no device needed.

For every row, that the draw is one the device can be held to the project's bounds on:
  loss   the fp32 CPU oracle's within 3e-6 of the fp64 oracle's, which leaves the device two thirds of the
         1e-5 loss budget (test_gpu_model.LOSS_RTOL) the sweep asserts against the fp32 oracle;
  grads  the fp32 oracle's own-branch gradients within 1e-5 normwise of the fp64 oracle's (no ReLU decision
         of the draw sits within fp32 rounding of 0);
and that the table says what the library does: vqhmm_elbo_stage_family gives, stage by stage, the families the
row claims (the query is host-only), every family the dispatch can reach is claimed by some row, and the shape of
every row is as the sweep needs it (>= 600 PCL rows, ragged against every tile, lengths T, 1, 2 and a middle one).
A draw that misses a bound gets another seed, never a wider bound.  The fp32 oracle's sums depend on the host
(its thread count splits them differently), so the seeds were picked to hold both bounds with a margin at 1, 2, 4,
8 and 16 threads.
"""
import numpy as np
import pytest
import torch

from oracle import ref_model as RM
import width_cases as W

LOSS_GAP = 3e-6
GRAD_GAP = 1e-5

# Every family vqhmm_elbo_stage_family can return for a supported shape (conv.hip conv_choice / wgrad_choice,
# api.hip head_kind and the stage switch), the staged head's string split into its parts.  conv_mm tiles that
# the step cannot reach are absent: without a tail a layer with N, Kc <= 64 runs on conv2, so the 16-channel
# slice tiles appear only with a tail conv2 refuses, and a tail is split off (+tail_kernel) only from the
# 256-row tiles (C2 > 139 beside 16 outputs, > 123 beside 32) or the widest one (N > 256).
ALL_FAMILIES = {
    "prologue", "(prologue)", "finalize_loss", "logits_bwd", "grad_tail", "compose_bwd", "tail",
    "conv2", "conv2+logits_bwd", "conv2+logits_bwd+logits_dg", "fused_pair", "bwd_pair",
    "strip_fwd", "strip_bwd", "strip_bwdw", "convbig", "convbig+tail",
    "conv_mm<256,16,16>+tail", "conv_mm<256,16,16>+tail_kernel", "conv_mm<256,16,32>", "conv_mm<256,16,32>+tail",
    "conv_mm<256,32,16>+tail", "conv_mm<256,32,32>", "conv_mm<256,32,32>+tail", "conv_mm<256,32,32>+tail_kernel",
    "conv_mm<128,64,16>+tail", "conv_mm<128,64,32>", "conv_mm<128,64,32>+tail",
    "conv_mm<64,128,16>", "conv_mm<64,128,16>+tail", "conv_mm<64,128,32>", "conv_mm<64,128,32>+tail",
    "conv_mm<64,256,16>", "conv_mm<64,256,16>+tail", "conv_mm<64,256,16>+tail_kernel",
    "wgrad2", "wgrad2_group", "wgradbig", "wgrad_generic",
    "pipe", "coop", "mfma", "scalar",
    "staged:l1<16>", "staged:l1_wide<1>", "staged:l1_wide<4>", "staged:l1_pow2<16>", "staged:l1_pow2<32>",
    "staged:l1<64>",
}


def family_parts(fam):
    """A stage's family string as its parts: 'staged:l1<16>;hid=conv2;...' -> {'staged:l1<16>', 'conv2', ...}."""
    return {part.split("=", 1)[-1] for part in fam.split(";")}


def oracle_gap(case):
    """-> (relative loss gap, worst normwise gradient gap and its parameter) of the fp32 oracle against fp64."""
    D, H, K, H2, U, TH = case.dims
    _, sd, x, u, L = W.step_inputs(case.dims, case.B, case.T, case.seed, lengths=case.lengths)
    p32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    p64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    l32 = RM.elbo(p32, x, u, L, 1.0, K, U)
    l64 = RM.elbo(p64, x.double(), u.double(), L, 1.0, K, U)
    l32.backward()
    l64.backward()
    worst = (0.0, "")
    for name in RM.PARAM_ORDER:
        r = p64[name].grad
        err = ((p32[name].grad.double() - r).norm() / max(r.norm().item(), 1e-30)).item()
        worst = max(worst, (err, name))
    return abs(l32.item() - l64.item()) / abs(l64.item()), worst


@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_fp32_oracle_close_to_fp64(case):
    loss_gap, (grad_gap, name) = oracle_gap(case)
    print(f"{case.name}: loss gap {loss_gap:.2e}, worst gradient gap {grad_gap:.2e} ({name})")
    assert np.isfinite(loss_gap) and loss_gap <= LOSS_GAP, loss_gap
    assert grad_gap <= GRAD_GAP, (name, grad_gap)


@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_row_shape(case):
    R = case.B * (case.T + 2)
    assert R >= 600 and all(R % m for m in (64, 128, 256))
    assert len(case.lengths) == case.B
    assert {case.T, 1, 2} <= set(case.lengths) and any(2 < n < case.T - 1 for n in case.lengths)
    assert case.why


@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_families_as_claimed(case):
    got = W.stage_families(case.dims, case.B, case.T)
    assert got == case.families, {s: (got[s], case.families[s]) for s in W.STAGES if got[s] != case.families[s]}


def test_every_family_claimed_by_a_row():
    claimed = set()
    for c in W.CASES:
        for fam in c.families.values():
            claimed |= family_parts(fam)
    assert "unsupported" not in claimed
    assert claimed == ALL_FAMILIES, (sorted(ALL_FAMILIES - claimed), sorted(claimed - ALL_FAMILIES))


def test_reachable_families_are_listed():
    """A grid of dims around every threshold of the dispatch reaches nothing outside ALL_FAMILIES (but
    'unsupported', which only the shapes of width_cases.UNSUPPORTED and tails wider than 159 channels give)."""
    seen = set()
    for D in (1, 5, 6, 16, 17, 21, 62, 63, 64):
        for H in (8, 16, 20, 32, 40, 64, 66, 128, 256, 272):
            for K in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64):
                for H2 in (1, 16, 20, 31, 32, 34, 64, 72, 128, 272):
                    for fam in W.stage_families((D, H, K, H2, 4, 128), 7, 90).values():
                        seen |= family_parts(fam)
    for U in (1, 4, 5, 8, 9):
        for TH in (16, 48, 64, 128, 256, 512):
            for K in (1, 4, 5, 8):
                seen |= family_parts(W.stage_families((5, 32, K, 16, U, TH), 7, 90)["head"])
    assert seen - {"unsupported"} <= ALL_FAMILIES, sorted(seen - ALL_FAMILIES)


@pytest.mark.parametrize("dims,B,T,why", W.UNSUPPORTED, ids=[str(u[0]) for u in W.UNSUPPORTED])
def test_unsupported_shapes_say_so(dims, B, T, why):
    fams = W.stage_families(dims, B, T)
    assert any("unsupported" in f for f in fams.values()), fams
