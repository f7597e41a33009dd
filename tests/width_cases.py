"""The width sweep's case table (a helper for tests/test_width_cases.py and tests/test_gpu_widths.py, not a
test): model dims (D, H, K, H2, U, TH) chosen from the step's kernel dispatch so that every conv, weight-gradient
and head family the training step can run meets the oracle at several row tiles.

Every case has >= 600 PCL rows B * (T + 2), not a multiple of 64, 128 or 256 (every conv tile configuration runs
several row tiles and a ragged last one), and lengths that include T, 1, 2 and a value in the middle.

`families` is what vqhmm_elbo_stage_family returns for the 23 stages of the step, in stage order (STAGES).  The
tests assert it, so a change of the dispatch that moves a case off the path it is here for fails loudly.
`python tests/width_cases.py` prints the table's families as the library gives them.
"""
import ctypes
from collections import namedtuple

import torch

STAGES = ("topcl", "compose", "enc1", "enc2", "dec1", "dec2", "head", "final",
          "par_dg", "dec2_dg", "dec1_dg", "logit_bwd", "logit_dg", "enc2_dg",
          "w_par", "w_dec2", "w_dec1", "w_logit", "w_enc2", "w_enc1", "reduce", "compose_bwd", "logprior")

Case = namedtuple("Case", "name dims B T lengths seed why families")


def _lengths(B, T):
    """T, 1, 2, the middle, then values spread over (2, T)."""
    base = [T, 1, 2, T // 2, T, T - 1, 3 + T // 3, T - 7, 17]
    return tuple(base[:B])


def _case(name, dims, B, T, seed, why, families):
    assert B * (T + 2) >= 600 and all(B * (T + 2) % m for m in (64, 128, 256))
    fam = dict(zip(STAGES, families.split()))
    assert len(fam) == len(STAGES), name
    return Case(name, dims, B, T, _lengths(B, T), seed, why, fam)


CASES = [
    _case("gen_h128", (5, 128, 3, 64, 4, 128), 7, 90, 101,
          "cfg2 with the hidden sizes doubled: every conv but to_logits' dgrad on conv_mm / convbig, "
          "wgrad_generic",
          "prologue (prologue) conv_mm<64,128,16> conv_mm<128,64,32>+tail conv_mm<64,128,16> "
          "conv_mm<64,128,32>+tail pipe finalize_loss conv_mm<64,128,16> convbig conv_mm<256,16,32> logits_bwd "
          "conv2 convbig wgrad_generic wgradbig wgrad_generic wgrad2 wgradbig wgrad_generic grad_tail "
          "compose_bwd grad_tail"),
    _case("gen_h256", (5, 256, 3, 128, 4, 128), 9, 130, 151,
          "the fused tail at N == BN = 256; to_logits' dgrad on conv_mm",
          "prologue (prologue) conv_mm<64,256,16> conv_mm<64,128,32>+tail conv_mm<64,256,16> "
          "conv_mm<64,256,16>+tail pipe finalize_loss conv_mm<64,256,16> convbig conv_mm<256,16,32> logits_bwd "
          "conv_mm<64,128,16> convbig wgrad_generic wgradbig wgrad_generic wgrad_generic wgradbig wgrad_generic "
          "grad_tail compose_bwd grad_tail"),
    _case("gen_h66", (6, 66, 4, 34, 4, 128), 7, 90, 200,
          "nothing on a 16 or 4 grid: partial K-slices, 2-wide edge tiles, wgrad_generic for every wide layer",
          "prologue (prologue) conv_mm<64,128,16> conv_mm<128,64,32>+tail conv_mm<64,128,16> "
          "conv_mm<64,128,32>+tail pipe finalize_loss conv_mm<64,128,16> conv_mm<64,128,32> conv_mm<256,16,32> "
          "logits_bwd conv2 conv_mm<64,128,32> wgrad_generic wgrad_generic wgrad_generic wgrad2 wgrad_generic "
          "wgrad_generic grad_tail compose_bwd grad_tail"),
    _case("gen_h100_k18", (21, 100, 18, 50, 6, 48), 7, 90, 254,
          "odd D > 16, softmax tail C2 = 18, staged head K = 18, the Prior's K^2 = 324 dgrad on conv_mm",
          "prologue (prologue) conv_mm<64,128,32> conv_mm<128,64,32>+tail conv_mm<64,128,32> "
          "conv_mm<64,128,32>+tail "
          "staged:l1_wide<1>;hid=conv2;lgA=convbig;dhid=conv_mm<128,64,32>;dW1=wgrad2;dW2=wgradbig "
          "finalize_loss conv_mm<64,128,32> conv_mm<64,128,32> conv_mm<256,32,32> logits_bwd conv2 "
          "conv_mm<64,128,32> wgrad_generic wgradbig wgrad_generic wgrad2 wgrad_generic wgrad_generic grad_tail "
          "compose_bwd grad_tail"),
    _case("k32_wide_rows", (64, 80, 32, 72, 4, 16), 7, 90, 306,
          "the k32_wide golden's dims at many row tiles",
          "prologue (prologue) convbig conv_mm<64,128,32>+tail convbig convbig+tail "
          "staged:l1_pow2<32>;hid=conv2;lgA=convbig;dhid=convbig;dW1=wgrad2;dW2=wgradbig finalize_loss convbig "
          "convbig convbig logits_bwd convbig conv_mm<64,128,32> wgradbig wgradbig wgradbig wgradbig wgradbig "
          "wgradbig grad_tail compose_bwd grad_tail"),
    _case("d17_k8", (17, 64, 8, 32, 4, 128), 7, 90, 350,
          "to_params tail C2 = 34 on conv_mm, staged head at K = 8 (D > 16)",
          "prologue (prologue) conv2 conv2 conv2 conv_mm<128,64,32>+tail "
          "staged:l1<16>;hid=conv_mm<64,128,16>;lgA=convbig;dhid=convbig;dW1=wgradbig;dW2=wgradbig "
          "finalize_loss conv2 conv2 conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg "
          "conv2+logits_bwd+logits_dg conv2 wgrad2_group wgrad2_group wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group tail tail tail"),
    _case("w_h48", (5, 48, 4, 40, 4, 128), 7, 90, 401,
          "wgrad2 3-block sides (the catch-all 64 x 64 body) in the grouped launch",
          "prologue (prologue) fused_pair fused_pair fused_pair fused_pair pipe finalize_loss fused_pair "
          "fused_pair conv2+logits_bwd conv2+logits_bwd conv2 conv2 wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group wgrad2_group wgrad2_group tail tail tail"),
    _case("w_h40_k6", (12, 40, 6, 24, 3, 64), 7, 90, 453,
          "wgrad2 3 x 2 block variants, coop head K = 6, U = 3",
          "prologue (prologue) fused_pair fused_pair fused_pair fused_pair coop finalize_loss fused_pair "
          "fused_pair conv2+logits_bwd conv2+logits_bwd conv2 conv2 wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group wgrad2_group wgrad2_group tail tail tail"),
    _case("w_h2_64", (5, 64, 3, 64, 4, 128), 7, 90, 500,
          "H2 = 64: the backward pair launch",
          "prologue (prologue) fused_pair fused_pair fused_pair fused_pair pipe finalize_loss fused_pair "
          "fused_pair bwd_pair bwd_pair bwd_pair bwd_pair wgrad2_group wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group wgrad2_group tail tail tail"),
    _case("w_h2_48", (5, 64, 3, 48, 4, 128), 7, 90, 552,
          "H2 = 48: to_logits' dgrad in dec_conv1's epilogue, 3-block wgrad2 side",
          "prologue (prologue) fused_pair fused_pair fused_pair fused_pair pipe finalize_loss fused_pair "
          "fused_pair conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2 "
          "wgrad2_group wgrad2_group wgrad2_group wgrad2_group wgrad2_group wgrad2_group tail tail tail"),
    _case("w_k5_h2_40", (5, 64, 5, 40, 4, 64), 7, 90, 613,
          "K = 5: ACT 4 epilogue, composed-layer variant in the grouped launch",
          "prologue (prologue) fused_pair fused_pair fused_pair fused_pair coop finalize_loss fused_pair "
          "fused_pair conv2+logits_bwd conv2+logits_bwd conv2 conv2 wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group wgrad2_group wgrad2_group tail tail tail"),
    _case("d6_h64", (6, 64, 3, 32, 4, 128), 7, 90, 651,
          "3D > 16: H = 64 without the forward strip, backward strip without the folded wgrads",
          "prologue (prologue) fused_pair fused_pair fused_pair fused_pair pipe finalize_loss strip_bwd "
          "strip_bwd strip_bwd strip_bwd strip_bwd strip_bwd wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group wgrad2_group wgrad2_group tail tail tail"),
    _case("h2_31", (5, 64, 4, 31, 4, 128), 7, 90, 700,
          "odd H2 in the strips",
          "prologue (prologue) strip_fwd strip_fwd strip_fwd strip_fwd pipe finalize_loss strip_bwdw strip_bwdw "
          "strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw "
          "strip_bwdw tail tail tail"),
    _case("h2_7", (3, 64, 2, 7, 2, 64), 7, 90, 750,
          "H2 <= 16: forward strip, pair launches backward",
          "prologue (prologue) strip_fwd strip_fwd strip_fwd strip_fwd coop finalize_loss fused_pair fused_pair "
          "conv2+logits_bwd conv2+logits_bwd conv2 conv2 wgrad2_group wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group wgrad2_group tail tail tail"),
    _case("h16", (5, 16, 3, 8, 4, 64), 7, 90, 800,
          "one-block layers: wgrad2 separately (composed-layer exclusion)",
          "prologue (prologue) conv2 conv2 conv2 conv2 coop finalize_loss conv2 conv2 conv2+logits_bwd "
          "conv2+logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd "
          "grad_tail"),
    _case("h20", (5, 20, 3, 12, 4, 128), 7, 90, 851,
          "two-block H: wgrad2 separately",
          "prologue (prologue) conv2 conv2 conv2 conv2 pipe finalize_loss conv2 conv2 conv2+logits_bwd "
          "conv2+logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd "
          "grad_tail"),
    _case("min_1", (1, 64, 1, 1, 1, 64), 7, 90, 900,
          "the strips at D = K = H2 = U = 1",
          "prologue (prologue) strip_fwd strip_fwd strip_fwd strip_fwd coop finalize_loss fused_pair fused_pair "
          "conv2+logits_bwd conv2+logits_bwd conv2 conv2 wgrad2_group wgrad2_group wgrad2_group wgrad2_group "
          "wgrad2_group wgrad2_group tail tail tail"),
    _case("d1", (1, 64, 4, 32, 4, 128), 7, 90, 950,
          "D = 1 in the strips with the folded weight gradients",
          "prologue (prologue) strip_fwd strip_fwd strip_fwd strip_fwd pipe finalize_loss strip_bwdw strip_bwdw "
          "strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw strip_bwdw "
          "strip_bwdw tail tail tail"),
    _case("scalar_k5_u8", (5, 32, 5, 16, 8, 96), 7, 90, 1000,
          "scalar head <8, 8>: U = 8, TH = 96",
          "prologue (prologue) conv2 conv2 conv2 conv2 scalar finalize_loss conv2 conv2 "
          "conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2 wgrad2 wgrad2 "
          "wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd grad_tail"),
    _case("scalar_k8_u5", (16, 32, 8, 16, 5, 256), 7, 90, 1060,
          "scalar head <8, 8>: K = 8, U = 5, TH = 256, D = 16",
          "prologue (prologue) conv2 conv2 conv2 conv2 scalar finalize_loss conv2 conv2 "
          "conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2 wgrad2 wgrad2 "
          "wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd grad_tail"),
    _case("scalar_th48", (5, 32, 3, 16, 4, 48), 7, 90, 1103,
          "scalar head <4, 8>: TH = 48",
          "prologue (prologue) conv2 conv2 conv2 conv2 scalar finalize_loss conv2 conv2 "
          "conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2 wgrad2 wgrad2 "
          "wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd grad_tail"),
    _case("mfma_u6", (5, 32, 3, 16, 6, 64), 7, 90, 1151,
          "the tile-barrier MFMA head (U in 5..7)",
          "prologue (prologue) conv2 conv2 conv2 conv2 mfma finalize_loss conv2 conv2 "
          "conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2 wgrad2 wgrad2 "
          "wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd grad_tail"),
    _case("staged_d20", (20, 32, 3, 16, 4, 64), 7, 90, 1201,
          "staged head l1<16> at K = 3 because D > 16; to_params on convbig+tail",
          "prologue (prologue) conv2 conv2 conv2 convbig+tail "
          "staged:l1<16>;hid=conv2;lgA=conv2;dhid=conv2;dW1=wgrad2;dW2=wgrad2 finalize_loss conv2 conv2 "
          "conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2+logits_bwd+logits_dg conv2 wgrad2 wgrad2 "
          "wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd grad_tail"),
    _case("staged_k9", (8, 32, 9, 16, 4, 64), 7, 90, 1250,
          "staged head l1_wide<1> at its lower edge K = 9; logits_bwd launch",
          "prologue (prologue) conv2 conv2 conv2 conv2 "
          "staged:l1_wide<1>;hid=conv2;lgA=conv_mm<64,128,32>;dhid=conv_mm<128,64,32>;dW1=wgrad2;dW2=wgrad_generic "
          "finalize_loss conv2 conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 "
          "grad_tail compose_bwd grad_tail"),
    _case("staged_k12", (8, 32, 12, 16, 4, 64), 7, 90, 1301,
          "staged head l1_wide<4>",
          "prologue (prologue) conv2 conv2 conv2 conv2 "
          "staged:l1_wide<4>;hid=conv2;lgA=convbig;dhid=convbig;dW1=wgrad2;dW2=wgradbig finalize_loss conv2 "
          "conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd "
          "grad_tail"),
    _case("staged_k16", (8, 32, 16, 16, 4, 64), 7, 90, 1352,
          "staged head l1_pow2<16>",
          "prologue (prologue) conv2 conv2 conv2 conv2 "
          "staged:l1_pow2<16>;hid=conv2;lgA=convbig;dhid=convbig;dW1=wgrad2;dW2=wgradbig finalize_loss conv2 "
          "conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd "
          "grad_tail"),
    _case("staged_k33", (8, 32, 33, 16, 4, 64), 7, 90, 1412,
          "staged head l1<64> at its lower edge K = 33; K^2 = 1089 logits on conv_mm<64,256,16>",
          "prologue (prologue) conv2 conv_mm<256,16,32>+tail conv2 conv2 "
          "staged:l1<64>;hid=conv2;lgA=conv_mm<64,256,16>;dhid=conv_mm<128,64,32>;dW1=wgrad2;dW2=wgrad_generic "
          "finalize_loss conv2 conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 "
          "grad_tail compose_bwd grad_tail"),
    _case("staged_k64", (8, 32, 64, 16, 2, 64), 7, 90, 1464,
          "staged head l1<64> at K = 64, the step's largest",
          "prologue (prologue) conv2 convbig+tail conv2 conv2 "
          "staged:l1<64>;hid=conv2;lgA=convbig;dhid=convbig;dW1=wgrad2;dW2=wgradbig finalize_loss conv2 conv2 "
          "conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 grad_tail compose_bwd "
          "grad_tail"),
    _case("h272", (5, 272, 3, 32, 4, 128), 7, 90, 1502,
          "H > 256: to_params' tail as conv_tail_kernel over the stored activation",
          "prologue (prologue) conv_mm<64,256,16> conv_mm<256,32,32>+tail conv_mm<64,256,16> "
          "conv_mm<64,256,16>+tail_kernel pipe finalize_loss conv_mm<64,256,16> convbig conv_mm<256,16,32> "
          "logits_bwd conv2 convbig wgrad_generic wgradbig wgrad_generic wgrad2 wgradbig wgrad_generic "
          "grad_tail compose_bwd grad_tail"),
    _case("h2_272", (5, 64, 3, 272, 4, 128), 7, 90, 1523,
          "H2 > 256: to_logits + softmax as conv_tail_kernel over the stored activation",
          "prologue (prologue) conv2 conv_mm<64,256,16>+tail_kernel fused_pair fused_pair pipe finalize_loss "
          "fused_pair fused_pair conv2+logits_bwd conv2+logits_bwd conv_mm<64,256,16> convbig wgrad2 wgrad2 "
          "wgrad2 wgrad_generic wgradbig wgrad2 grad_tail compose_bwd grad_tail"),
    _case("d70_h12", (70, 12, 3, 8, 4, 64), 7, 90, 1551,
          "to_params tail C2 = 140: too large for the LDS beside a 256 x 16 tile, so conv_tail_kernel",
          "prologue (prologue) conv_mm<256,16,32> conv2 conv2 conv_mm<256,16,16>+tail_kernel "
          "staged:l1<16>;hid=conv2;lgA=conv2;dhid=conv2;dW1=wgrad2;dW2=wgrad2 finalize_loss conv_mm<256,16,32> "
          "conv2 conv2+logits_bwd conv2+logits_bwd conv2 conv2 wgradbig wgrad2 wgrad2 wgrad2 wgrad2 "
          "wgrad_generic grad_tail compose_bwd grad_tail"),
    _case("d64_h20", (64, 20, 3, 12, 4, 64), 7, 90, 1600,
          "the same beside a 256 x 32 tile (C2 = 128)",
          "prologue (prologue) conv2 conv2 conv2 conv_mm<256,32,32>+tail_kernel "
          "staged:l1<16>;hid=conv2;lgA=conv2;dhid=conv2;dW1=wgrad2;dW2=wgrad2 finalize_loss convbig conv2 "
          "conv2+logits_bwd conv2+logits_bwd conv2 conv2 wgradbig wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 grad_tail "
          "compose_bwd grad_tail"),
    _case("t_h16_k18", (17, 16, 18, 12, 4, 64), 7, 90, 1654,
          "conv_mm<256,16,16>+tail: softmax tail K = 18 and to_params tail 34 on 16-wide layers",
          "prologue (prologue) conv2 conv_mm<256,16,16>+tail conv2 conv_mm<256,16,16>+tail "
          "staged:l1_wide<1>;hid=conv2;lgA=convbig;dhid=conv_mm<128,64,32>;dW1=wgrad2;dW2=wgradbig "
          "finalize_loss conv2 conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 "
          "grad_tail compose_bwd grad_tail"),
    _case("t_h12_k17", (5, 12, 17, 20, 4, 64), 7, 90, 1700,
          "conv_mm<256,32,16>+tail",
          "prologue (prologue) conv2 conv_mm<256,32,16>+tail conv2 conv2 "
          "staged:l1_wide<1>;hid=conv2;lgA=conv_mm<64,256,16>;dhid=conv_mm<128,64,32>;dW1=wgrad2;dW2=wgrad_generic "
          "finalize_loss conv2 conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 "
          "grad_tail compose_bwd grad_tail"),
    _case("t_h16_h2_34", (5, 16, 17, 34, 4, 64), 7, 90, 1752,
          "conv_mm<128,64,16>+tail",
          "prologue (prologue) conv2 conv_mm<128,64,16>+tail conv2 conv2 "
          "staged:l1_wide<1>;hid=conv2;lgA=conv_mm<64,256,16>;dhid=conv_mm<128,64,32>;dW1=wgrad2;dW2=wgrad_generic "
          "finalize_loss conv2 conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 "
          "grad_tail compose_bwd grad_tail"),
    _case("t_h20_k17", (5, 20, 17, 12, 4, 64), 7, 90, 1800,
          "conv_mm<256,16,32>+tail",
          "prologue (prologue) conv2 conv_mm<256,16,32>+tail conv2 conv2 "
          "staged:l1_wide<1>;hid=conv2;lgA=conv_mm<64,256,16>;dhid=conv_mm<128,64,32>;dW1=wgrad2;dW2=wgrad_generic "
          "finalize_loss conv2 conv2 conv2 logits_bwd conv2 conv2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 wgrad2 "
          "grad_tail compose_bwd grad_tail"),
    _case("t_h8_h2_72", (5, 8, 3, 72, 4, 128), 7, 90, 1850,
          "conv_mm<64,128,16>+tail",
          "prologue (prologue) conv2 conv_mm<64,128,16>+tail conv2 conv2 pipe finalize_loss conv2 conv2 "
          "conv2+logits_bwd conv2+logits_bwd conv_mm<64,128,16> conv_mm<256,16,32> wgrad2 wgrad2 wgrad2 "
          "wgrad_generic wgradbig wgrad2 grad_tail compose_bwd grad_tail"),
    _case("h40_h2_72", (5, 40, 3, 72, 4, 128), 7, 90, 1907,
          "conv_mm<128,64,32> without a tail (enc_conv2's dgrad)",
          "prologue (prologue) conv2 conv_mm<64,128,32>+tail fused_pair fused_pair pipe finalize_loss "
          "fused_pair fused_pair conv2+logits_bwd conv2+logits_bwd conv_mm<64,128,16> conv_mm<128,64,32> wgrad2 "
          "wgrad2 wgrad2 wgrad_generic wgradbig wgrad2 grad_tail compose_bwd grad_tail"),
]

BY_NAME = {c.name: c for c in CASES}

# shapes the step refuses (INTEGRATION.md "Limits"): (dims, B, T, why)
UNSUPPORTED = [
    ((8, 32, 65, 16, 4, 64), 7, 90, "K > 64: the staged head's row kernels hold one state per lane"),
    ((80, 20, 3, 12, 4, 64), 7, 90, "to_params with 2D = 160 channels on the generic conv: conv_tail_kernel's rows "
                                    "hold at most 159 tail channels in LDS"),
]


def step_inputs(dims, B, T, seed, full_frac=0.5, lengths=None):
    """The model (CPU, seeded init), its state dict and one batch, as check_step_vs_oracle draws them.
    lengths=None: random lengths with the first full_frac of the batch at T."""
    import vqhmm
    D, H, K, H2, U, TH = dims
    torch.manual_seed(0)
    m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=U, trans_hidden=TH)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, T, generator=gen)
    u = torch.randn(B, U, T, generator=gen)
    L = torch.randint(20 if T > 20 else 1, T + 1, (B,), generator=gen)
    L[:int(B * full_frac)] = T
    if lengths is not None:
        L = torch.as_tensor(lengths, dtype=torch.int64)
        assert L.shape == (B,)
    return m, sd, x, u, L


def stage_families(dims, B, T):
    """vqhmm_elbo_stage_family for every stage (host-only: needs the library, no device)."""
    from vqhmm import _ext
    lib = _ext.load()
    d = _ext.Dims(*dims)
    n = lib.vqhmm_elbo_num_stages()
    assert n == len(STAGES)
    out = {}
    buf = ctypes.create_string_buffer(256)
    for st in range(n):
        _ext.check(lib.vqhmm_elbo_stage_family(ctypes.byref(d), B, T, st, buf, len(buf)), "stage family")
        out[STAGES[st]] = buf.value.decode()
    return out


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "vq-vae-hmm-model_amd")]
    for c in CASES:
        print(c.name, c.dims, " ".join(stage_families(c.dims, c.B, c.T)[s] for s in STAGES))
