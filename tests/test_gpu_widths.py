"""The training step across the model widths that select its fallback kernels (tests/width_cases.py): the
generic implicit-GEMM conv (conv.hip conv_mm_kernel, every tile the step can reach, with and without the fused
1x1 tail, and the tail as conv_tail_kernel), the generic weight gradient (wgrad_kernel<2, 2>), wgrad2 as separate
launches and its grouped variants, the scalar, MFMA and staged heads at the edges of their ranges, and the strips
at their minimum sizes.  Every case has more than 600 PCL rows, ragged against every tile height, and sequence
lengths T, 1, 2 and a middle one.

Each case asserts, through check_step_vs_oracle:
  families  vqhmm_elbo_stage_family gives, stage by stage, the kernel families the row is there for;
  loss      within 1e-5 relative (LOSS_RTOL) of the fp32 CPU oracle;
  grads     all 18 within 1e-5 normwise of the fp64 oracle on the device forward's own ReLU branch (the
            contract's bound, as in test_gpu_head.py), with the helper's caps on the ReLU decisions;
  surface   compute_loss + backward give the same bits as TrainState;
  poison    TrainState's workspace is filled with quiet NaNs before the step (test_gpu_configs.poison_workspace),
            so a read of a pad column, pad row or slab entry that no launch of the step wrote is a NaN in the
            loss or a gradient, not a silent zero from a fresh allocation.
tests/test_width_cases.py holds each draw's fp32 oracle to 3e-6 (loss) and 1e-5 (gradients) of fp64 on the CPU.

Family -> rows that assert it (conv families by the stage that runs them):
  conv2 (+logits_bwd[+logits_dg])      h16, h20, scalar_*, mfma_u6, staged_*, d17_k8
  fused_pair / bwd_pair                w_h48, w_h40_k6, w_k5_h2_40, w_h2_48 / w_h2_64
  strip_fwd / strip_bwd / strip_bwdw   h2_31, h2_7, min_1, d1 / d6_h64 / h2_31, d1
  convbig, convbig+tail                k32_wide_rows, staged_d20, staged_k64, gen_h128 (dec_conv2 dgrad)
  conv_mm<64,128,16>[+tail]            gen_h128, gen_h66 (enc/dec conv1, to_params dgrad) [t_h8_h2_72]
  conv_mm<64,128,32>[+tail]            gen_h66, gen_h100_k18 [gen_h128, gen_h66 dec_conv2+to_params]
  conv_mm<64,256,16>[+tail]            gen_h256, h272 [gen_h256: the tail at N == BN]
  conv_mm<64,256,16>+tail_kernel       h272 (to_params), h2_272 (to_logits + softmax)
  conv_mm<128,64,32>[+tail]            h40_h2_72 [gen_h128, gen_h66 enc_conv2; d17_k8 dec_conv2]
  conv_mm<128,64,16>+tail              t_h16_h2_34
  conv_mm<256,16,16>+tail[_kernel]     t_h16_k18 [d70_h12]
  conv_mm<256,16,32>[+tail]            gen_h128, gen_h256, gen_h66 (dec_conv1 dgrad) [t_h20_k17]
  conv_mm<256,32,16>+tail              t_h12_k17
  conv_mm<256,32,32>[+tail[_kernel]]   gen_h100_k18 (dec_conv1 dgrad) [h272 enc_conv2] [d64_h20]
  logits_bwd (its own launch)          gen_*, staged_k9 .. staged_k64
  wgrad2 / wgrad2_group                h16, h20, scalar_* / w_*, d6_h64, d17_k8
  wgradbig / wgrad_generic             k32_wide_rows, gen_h128 / gen_h128, gen_h256, gen_h66, gen_h100_k18
  pipe / coop / mfma / scalar          gen_*, w_h48 / w_h40_k6, h16 / mfma_u6 / scalar_k5_u8, scalar_k8_u5, scalar_th48
  staged:l1<16>                        d17_k8, staged_d20
  staged:l1_wide<1> / l1_wide<4>       staged_k9, gen_h100_k18 / staged_k12
  staged:l1_pow2<16> / l1_pow2<32>     staged_k16 / k32_wide_rows
  staged:l1<64>                        staged_k33, staged_k64
tests/test_width_cases.py::test_every_family_claimed_by_a_row checks this table's claim on the CPU.
"""
import pytest
import torch

import width_cases as W
from test_gpu_configs import check_step_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_width_step_vs_oracle(case):
    got = W.stage_families(case.dims, case.B, case.T)
    assert got == case.families, {s: (got[s], case.families[s]) for s in W.STAGES if got[s] != case.families[s]}
    check_step_vs_oracle(case.dims, case.B, case.T, case.seed, rtol_norm=1e-5, lengths=case.lengths, poison=True)


@pytest.mark.parametrize("dims,B,T,why", W.UNSUPPORTED, ids=[str(u[0]) for u in W.UNSUPPORTED])
def test_unsupported_shape_raises(dims, B, T, why):
    """A shape past the step's limits (INTEGRATION.md "Limits") raises the "unsupported shape" error from
    compute_loss and hands back no number."""
    import vqhmm
    D, H, K, H2, U, TH = dims
    m, _, x, u, L = W.step_inputs(dims, B, T, seed=1)
    mg = m.cuda()
    loss = None
    with pytest.raises(RuntimeError, match="unsupported shape"):
        loss = mg.compute_loss(x.cuda(), u.cuda(), L, 1.0)
    torch.cuda.synchronize()
    assert loss is None
    st = vqhmm.TrainState(mg, lr=1e-3)
    xs, us, Ls = st.prepare(x, u, L)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        st.forward_backward(xs, us, Ls, 1.0)
    torch.cuda.synchronize()
