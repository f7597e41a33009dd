"""The folded backward strip's asymmetric halo (strip_bwdw.hip).

The strip owns window rows 3 .. 3 + own - 1, own <= 120, and computes no to_params dgrad block for window rows -1
and 128: dg2 on rows 0..127 gives dg1 on 1..126, dh2 / dlog on 2..125 and dh1 on 3..124, which covers every owned
row.  The shapes below sit on the edges: window rows before 0 and past R, the cap of 120 with one and with two
strips per workgroup, workgroups of different strip counts side by side, three strips per workgroup, and a row
count that 124-row strips covered in one round and 120-row strips do not.  (The last four are also the shapes
at which a weight-gradient pass carried from one strip into the next would go wrong: DESIGN section 10 item 7.)

Each case: the folded strip (VQHMM_STRIP_WGRAD=1) against the grouped weight-gradient path (=0) in fresh processes
(equal losses, gradients within 1e-6 normwise), and the step against the oracle at 1e-5."""
import pytest
import torch

from test_gpu_configs import check_step_vs_oracle
from test_gpu_trainer import _run_both_tol

DIMS = (5, 64, 3, 32, 128)  # D, H, K, H2, TH


def _cdiv(a, b):
    return -(-a // b)


def bwdw_own(R):
    """strip_bwdw_own's arithmetic: as few rounds of 256 strips as 120 owned rows allow, a multiple of 4."""
    rounds = _cdiv(R, 256 * 120)
    own = _cdiv(_cdiv(R, 256 * rounds), 4) * 4
    return min(max(own, 4), 120)


def bwdw_strips(R):
    """(strips, workgroups, strips of the busiest workgroup, strips of the least busy one)"""
    n = _cdiv(R, bwdw_own(R))
    grid = min(max(n, 1), 256)
    return n, grid, _cdiv(n, grid), n // grid


# (B, T, R, own, strips, most strips per workgroup, fewest)
CASES = [
    (1, 5, 7, 4, 2, 1, 1),             # two 4-row strips; window rows before 0 and past R
    (150, 198, 30000, 120, 250, 1, 1),  # the cap; one strip per workgroup
    (300, 198, 60000, 120, 500, 2, 1),  # the cap; two strips per workgroup
    (270, 121, 33210, 68, 489, 2, 1),   # workgroups with two strips next to workgroups with one
    (310, 198, 62000, 84, 739, 3, 2),   # three strips per workgroup: a first, a middle and a last one
    (155, 200, 31310, 64, 490, 2, 1),   # 124 owned rows in one round before the cap; now two rounds
]


@pytest.mark.parametrize("B,T,R,own,strips,most,fewest", CASES)
def test_bwdw_case_geometry(B, T, R, own, strips, most, fewest):
    """The cases sit where the table says (the launcher's arithmetic restated; no device needed)."""
    assert R == B * (T + 2)
    assert bwdw_own(R) == own
    n, grid, hi, lo = bwdw_strips(R)
    assert (n, hi, lo) == (strips, most, fewest)
    assert 3 + own - 1 <= 124 and own % 4 == 0  # dh1 is exact on window rows 3 .. 124
    if R == 31310:  # with the cap at 124 this row count was one round of 124-row strips
        assert _cdiv(_cdiv(R, 256 * _cdiv(R, 256 * 124)), 4) * 4 == 124


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [c[:2] for c in CASES])
def test_bwdw_fold_matches_grouped(tmp_path, B, T):
    out = _run_both_tol(tmp_path, "VQHMM_STRIP_WGRAD", DIMS, (B, T))
    assert torch.equal(out["1"]["loss0"], out["0"]["loss0"])  # the forward is untouched


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [c[:2] for c in CASES])
def test_bwdw_step_vs_oracle(B, T):
    gen = torch.Generator().manual_seed(7)
    L = torch.randint(max(1, T // 3), T + 1, (B,), generator=gen)  # ragged, as the fold-vs-grouped runs draw them
    D, H, K, H2, TH = DIMS
    check_step_vs_oracle((D, H, K, H2, 4, TH), B, T, seed=1000 + B, rtol_norm=1e-5, lengths=L)
