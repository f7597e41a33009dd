"""The forward strip owns window rows 3..124 (at most 122 rows) and computes no enc_conv1 block for its window's
outer rows -1 and 128: h1e is exact on window rows 0..127, h2e / logits / q on 1..126, g1 on 2..125, g2 and
mu | logvar on 3..124.  The two LDS slot rows that are no longer written (slot 0 row 0, slot 7 row 17) hold
whatever an earlier strip left there, and must never reach a stored row.

Checked as tests/test_gpu_strip_halo.py does, at row counts around a multiple of the 122 owned rows: every stored
activation of the forward (h1, h2, logits, q, g1, g2, mu | logvar) equals the pair launches' (VQHMM_STRIP=0) bit
for bit, and a sequence that is NaN throughout (so the slot rows next to its neighbours' strips hold NaN) stays
inside itself.  One case runs the one-block enc_conv2 instance (hidden_dim2 = 16), whose weight image ends in a
half-filled 1-KB DMA chunk, and one the head fused into the strip launch, whose row arithmetic follows the
owned rows."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_gpu_trainer import _run_both_tol

pytestmark = pytest.mark.gpu

_RUN = r"""
import ctypes, sys, torch
sys.path.insert(0, sys.argv[1])
import vqhmm
from vqhmm import _ext
B, T, bad = (int(v) for v in sys.argv[3].split(","))
D, H, K, H2 = (int(v) for v in sys.argv[4].split(","))
gen = torch.Generator().manual_seed(B + T)
x = torch.randn(B, D, T, generator=gen)
if bad >= 0:
    x[bad] = float("nan")
u = torch.randn(B, 4, T, generator=gen)
L = torch.randint(1, T + 1, (B,), generator=gen)
L[0] = T
torch.manual_seed(3)
m = vqhmm.VAE_HMM(D, H, K, H2, u_dim=4, trans_hidden=128).cuda()
st = vqhmm.TrainState(m, lr=1e-3)
xs, us, Ls = st.prepare(x, u, L)
st.forward_backward(xs, us, Ls, 0.5)
torch.cuda.synchronize()
ws = st.workspace(B, T)
ptr = (ctypes.c_void_p * 16)()
_ext.check(st.lib.vqhmm_elbo_debug_buffers(ctypes.byref(st.dims), B, T, _ext.ptr(ws), ptr), "buffers")
R = B * (T + 2)
ld4 = lambda c: (c + 3) // 4 * 4
out = {}
for name, i, ch in (("h1", 1, H), ("h2", 2, H2), ("logits", 3, K), ("q", 4, K), ("g1", 5, H), ("g2", 6, H),
                    ("par", 7, 2 * D)):
    off = ptr[i] - ws.data_ptr()
    out[name] = ws[off:off + R * ld4(ch) * 4].view(torch.float32).view(R, ld4(ch)).cpu().clone()
torch.save(out, sys.argv[2])
"""


def _strip_vs_pair(tmp_path, B, T, bad, dims):
    pkg = os.path.join(ROOT, "vq-vae-hmm-model_amd")
    out = {}
    for flag in ("1", "0"):
        f = str(tmp_path / f"strip{flag}.pt")
        subprocess.run([sys.executable, "-c", _RUN, pkg, f, f"{B},{T},{bad}", ",".join(map(str, dims))], check=True,
                       timeout=300, env=dict(os.environ, VQHMM_STRIP=flag, VQHMM_STRIP_HEAD="0"))
        out[flag] = torch.load(f, weights_only=True)
    rows = torch.arange(B * (T + 2))
    clean = (rows // (T + 2)) != bad
    assert set(out["1"]) == set(out["0"]) and len(out["1"]) == 7
    for name, a in out["1"].items():
        b = out["0"][name]
        assert a.shape == b.shape, name
        assert torch.equal(a[clean], b[clean]), name             # bit for bit (no NaN here: equal would fail)
        assert not torch.isnan(a[clean]).any(), name
        assert torch.equal(torch.isnan(a[~clean]), torch.isnan(b[~clean])), name
        same = ~torch.isnan(a[~clean])
        assert torch.equal(a[~clean][same], b[~clean][same]), name  # the NaN sequence's pad rows and channels


# R = B (T + 2); 122 owned rows per strip
@pytest.mark.parametrize("B,T,bad", [(1, 120, -1),    # R = 122: one full strip, its last owned row the batch's last
                                     (1, 121, -1),    # R = 123: a last strip of one row
                                     (5, 71, 2),      # R = 365 = 2 * 122 + 121: sequences cross strip edges, one NaN
                                     (2, 120, 0),     # R = 244: strips end on sequence ends, the first sequence NaN
                                     (270, 121, 135)])  # 33,210 rows = 273 strips on 256 workgroups; one NaN sequence
def test_strip_forward_owned_rows(tmp_path, B, T, bad):
    _strip_vs_pair(tmp_path, B, T, bad, (5, 64, 3, 32))


def test_strip_forward_owned_rows_one_block(tmp_path):
    """hidden_dim2 = 16: the one-block enc_conv2 instance, its 13.5-KB weight image copied in whole 1-KB chunks
    (the last one overlapping its predecessor); 365 rows, sequences across strip edges, one of them NaN."""
    _strip_vs_pair(tmp_path, 5, 71, 2, (4, 64, 4, 16))


def test_strip_head_owned_rows(tmp_path):
    """The ELBO head fused into the strip launch (VQHMM_STRIP_HEAD=1) takes its rows, its q rows in LDS and its
    slab count from the strip's owned rows: loss and gradient against the head's own launch at the tolerance of
    test_strip_head_matches_head_launch (1e-6: a summation order), 273 strips on 256 workgroups."""
    _run_both_tol(tmp_path, "VQHMM_STRIP_HEAD", (5, 64, 3, 32, 128), (270, 121))
