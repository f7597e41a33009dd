"""CPU checks of the saturated cases (tests/saturated_cases.py), the reference alone, no device needed: that the
inputs are in the regime they claim and that the tolerance tests/test_gpu_saturated.py holds the device to is one
the reference's own fp32 arithmetic reaches.

LEVEL_MODERATE, all three edits.  fp64 and fp32 oracle run on the same ReLU masks, the fp64 oracle's own decisions
(preactivations > 0 passed as relu_masks), so what separates them is rounding alone.
  regime     share of (b, c, t) with exp(logvar) < 1e-8 >= 0.3; share of positions with max_k q > 0.999 >= 0.5; at
             least one q exactly 0 in fp32; log_A.min() < -50; the constant channels' logvar equal their bias bit
             for bit; recon, prior and entropy finite.
  reference  each of the 18 fp32 gradients within 5e-6 normwise of the fp64 gradient, half of the 1e-5 the device is
             given; the three pieces within 1e-6 relative.
A case that misses a condition gets another seed or other lengths, never another condition.

LEVEL_HARD, "logit" alone.  The fp32 reference itself sits 1e-5 to 6e-5 from fp64 on the encoder gradients (the
cancellation in q ((lg - lse) - f)), so no fixed tolerance is honest there and the device test measures its own.
Here: more than 40 % of q exactly 0 in fp32, and every piece and gradient of the fp32 reference finite.
"""
import functools
import math

import pytest
import torch

from oracle import ref_model as RM
import saturated_cases as S

GRAD_GAP = 5e-6
PIECE_GAP = 1e-6
PIECES = ("recon", "prior", "entropy")

IDS = [c.name for c in S.CASES]


def oracle_run(sd, x, u, L, dims, dtype, masks):
    """elbo_terms and the gradient of recon + prior - entropy at dtype on the given masks:
    (terms (detached), {name: grad})."""
    K, U = dims[2], dims[4]
    p = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    t = RM.elbo_terms(p, x.to(dtype), u.to(dtype), L, K, U, relu_masks=masks)
    (t["recon"] + 1.0 * (t["prior"] - t["entropy"])).backward()
    return {k: v.detach() for k, v in t.items()}, {n: p[n].grad for n in RM.PARAM_ORDER}


@functools.lru_cache(maxsize=None)
def both(name, level, what):
    case = S.BY_NAME[name]
    _, sd, x, u, L = S.saturated_inputs(case, level, what)
    masks = [pre > 0 for pre in RM.preactivations({k: v.double() for k, v in sd.items()}, x.double())]
    t64, g64 = oracle_run(sd, x, u, L, case.dims, torch.float64, masks)
    t32, g32 = oracle_run(sd, x, u, L, case.dims, torch.float32, masks)
    return sd, t64, g64, t32, g32


@pytest.mark.parametrize("name", IDS)
def test_families_as_claimed(name):
    S.check_families(S.BY_NAME[name])


@pytest.mark.parametrize("name", IDS)
def test_row_shape(name):
    c = S.BY_NAME[name]
    R = c.B * (c.T + 2)
    assert (c.B, c.T) == (7, 90) and R == 644 and R % 64 and R % 128 and -(-R // 122) == 6
    assert {c.T, 1, 2} <= set(c.lengths) and len(c.lengths) == c.B


@pytest.mark.parametrize("name", IDS)
def test_moderate_inputs_are_in_the_regime(name):
    case = S.BY_NAME[name]
    D = case.dims[0]
    sd, t64, _, t32, _ = both(name, S.LEVEL_MODERATE, S.ALL)
    clamped = (t32["logvar"].exp() < S.VAR_FLOOR).float().mean().item()
    q = t32["q"]
    sat = (q.max(dim=1).values > 0.999).float().mean().item()
    zeros = (q == 0).float().mean().item()
    la_min = t32["log_A"].min().item()
    print(f"{name}: clamped {clamped:.3f}, saturated {sat:.3f}, q == 0 {zeros:.4f}, log_A.min {la_min:.1f}")
    assert clamped >= 0.3
    assert sat >= 0.5
    assert zeros > 0
    assert la_min < -50
    bias = sd["decoder.to_params.bias"]
    for c in S.constant_channels(D):
        assert bias[D + c].item() == S.LOGVAR_BIAS[c % 5]
        assert torch.equal(t32["logvar"][:, c, :], bias[D + c].expand(case.B, case.T)), c
        assert torch.equal(t64["logvar"][:, c, :], bias[D + c].double().expand(case.B, case.T)), c
    for t in (t32, t64):
        assert all(math.isfinite(t[k].item()) for k in PIECES), [t[k].item() for k in PIECES]


@pytest.mark.parametrize("name", IDS)
def test_moderate_fp32_reference_close_to_fp64(name):
    _, t64, g64, t32, g32 = both(name, S.LEVEL_MODERATE, S.ALL)
    for k in PIECES:
        gap = abs(t32[k].item() - t64[k].item()) / abs(t64[k].item())
        print(f"{name}: {k} {t64[k].item():.6e}, fp32 gap {gap:.2e}")
        assert gap <= PIECE_GAP, (k, gap)
    worst = (0.0, "")
    for n in RM.PARAM_ORDER:
        r = g64[n]
        assert torch.isfinite(g32[n]).all(), n
        err = ((g32[n].double() - r).norm() / max(r.norm().item(), 1e-30)).item()
        worst = max(worst, (err, n))
        assert err <= GRAD_GAP, (n, err)
    print(f"{name}: worst fp32 gradient gap {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("name", IDS)
def test_hard_logits_reference_is_finite(name):
    _, _, g64, t32, g32 = both(name, S.LEVEL_HARD, frozenset({"logit"}))
    zeros = (t32["q"] == 0).float().mean().item()
    worst = max((((g32[n].double() - g64[n]).norm() / max(g64[n].norm().item(), 1e-30)).item(), n)
                for n in RM.PARAM_ORDER)
    print(f"{name}: q == 0 {zeros:.3f}, worst fp32 gradient gap {worst[0]:.2e} ({worst[1]})")
    assert zeros > 0.4
    assert all(math.isfinite(t32[k].item()) for k in PIECES)
    assert all(torch.isfinite(g32[n]).all() for n in RM.PARAM_ORDER)
