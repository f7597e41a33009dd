"""The folded backward strip's load addressing and phase order (strip_bwdw.hip).

Every row-indexed load of a strip is a per-strip scalar base (the array's row s0 = strip * own - 3) plus a 32-bit
per-lane offset, the lane's window row clamped into [0, R) against two per-strip scalars (the first and the last
window row inside); the per-lane parts are computed once and kept across a workgroup's strips.  The h1e mask rows are
issued a phase ahead of their use, and to_logits' weight-gradient tile rides in enc_conv2's pass on waves 0-1.  The
shapes sit where that can break:

  (1, 5)      R = 7: both clamps active in one window (rows before 0 and past R in the same strip)
  (10, 198),  one strip per workgroup: the first strip's rows before 0, the last strip's rows past R
  (50, 198)
  (310, 198)  three strips per workgroup: the kept per-lane offsets survive the back edge, and a workgroup's last
              strip (its P7 overwrites DL's region with decoder.conv1's weight) still has DL read before it
  (25, 39)    R = 1025 = 1 (mod own = 8): the last strip owns a single row
  four dims at (50, 198) that move the structurally-zero lanes of the single-tile passes (K = 4, 2; D = 3, 4)

Each case: the folded strip against the grouped weight-gradient path in fresh processes (equal losses, gradients
within 1e-6 normwise, test_gpu_bwdw_wgpass's runner), and the step against the oracle at 1e-5, with ragged lengths."""
import pytest
import torch

from test_gpu_bwdw_sched import bwdw_own, bwdw_strips
from test_gpu_bwdw_wgpass import _fold_vs_grouped, _oracle_seed, _runs_folded_strip
from test_gpu_configs import check_step_vs_oracle

DIMS = (5, 64, 3, 32, 128)  # D, H, K, H2, TH
WIN, LO = 128, 3            # window rows; the first owned window row

# (B, T, R, own, strips, strips of the busiest workgroup, rows the last strip owns)
CASES = [
    (1, 5, 7, 4, 2, 1, 3),
    (10, 198, 2000, 8, 250, 1, 8),
    (50, 198, 10000, 40, 250, 1, 40),
    (310, 198, 62000, 84, 739, 3, 8),
    (25, 39, 1025, 8, 129, 1, 1),
]

MASK_DIMS = [
    (5, 64, 4, 32, 128),
    (5, 64, 2, 32, 128),
    (3, 64, 3, 32, 128),
    (4, 64, 3, 32, 128),
]
MASK_BT = (50, 198)

RUNS = [(DIMS, c[0], c[1]) for c in CASES] + [(d, *MASK_BT) for d in MASK_DIMS]


@pytest.mark.parametrize("B,T,R,own,strips,most,last_rows", CASES)
def test_latency_case_geometry(B, T, R, own, strips, most, last_rows):
    """The cases sit where the table says (the launcher's arithmetic as test_gpu_bwdw_sched restates it; no
    device needed)."""
    assert R == B * (T + 2)
    assert bwdw_own(R) == own and own % 4 == 0
    n, grid, hi, lo = bwdw_strips(R)
    assert (n, hi) == (strips, most)
    assert R - (n - 1) * own == last_rows
    # window row 0 of strip s is PCL row s * own - LO: the first strip starts before row 0, the last one ends past R
    assert 0 * own - LO < 0
    assert (n - 1) * own - LO + WIN - 1 >= R
    if R == 7:  # both in the first strip's window
        assert -LO + WIN - 1 >= R
    if R == 1025:
        assert R % own == 1


@pytest.mark.parametrize("dims,B,T", RUNS)
def test_latency_dims_run_the_folded_strip(dims, B, T):
    """Every case's backward is the folded strip (host-only query)."""
    assert _runs_folded_strip(dims, B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B,T", RUNS)
def test_latency_fold_matches_grouped(tmp_path, dims, B, T):
    assert _runs_folded_strip(dims, B, T)
    out = _fold_vs_grouped(tmp_path, dims, (B, T))
    assert torch.equal(out["1"]["loss0"], out["0"]["loss0"])  # the forward is untouched


@pytest.mark.gpu
@pytest.mark.parametrize("dims,B,T", RUNS)
def test_latency_step_vs_oracle(dims, B, T):
    assert _runs_folded_strip(dims, B, T)
    gen = torch.Generator().manual_seed(7)
    L = torch.randint(max(1, T // 3), T + 1, (B,), generator=gen)  # ragged, as the fold-vs-grouped runs draw them
    D, H, K, H2, TH = dims
    check_step_vs_oracle((D, H, K, H2, 4, TH), B, T, seed=_oracle_seed(dims, B), rtol_norm=1e-5, lengths=L)
