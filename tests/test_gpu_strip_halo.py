"""The forward strip computes no composed-dec_conv1 block for its window's outer rows -1 and 128: those g1
rows feed only dec_conv2's window rows 0 and 127, which no strip stores.  Whatever the two LDS slot rows still
hold (enc_conv1's halo rows of the same strip) must therefore never reach a stored row.

Checked where it could: row counts around a multiple of the 124 owned rows (last strip of 1, 123 and 124 rows),
more strips than workgroups, and one sequence that is NaN throughout, so the slot rows next to its neighbours'
strips hold NaN.  Every stored activation of the forward (h1, h2, logits, q, g1, g2, mu | logvar) equals the
pair launches' (VQHMM_STRIP=0) bit for bit, and the NaN stays inside its own sequence."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

_RUN = r"""
import ctypes, sys, torch
sys.path.insert(0, sys.argv[1])
import vqhmm
from vqhmm import _ext
B, T, bad = (int(v) for v in sys.argv[3].split(","))
D, H, K, H2 = 5, 64, 3, 32
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


# R = B (T + 2); 124 owned rows per strip
@pytest.mark.parametrize("B,T,bad", [(1, 122, -1),    # R = 124: one full strip, its last owned row the batch's last
                                     (1, 123, -1),    # R = 125: a last strip of one row
                                     (3, 121, 1),     # R = 369 = 2 * 124 + 121, the middle sequence NaN
                                     (2, 122, 0),     # R = 248: strips end on sequence ends, the first sequence NaN
                                     (270, 121, 135)])  # 33,210 rows = 268 strips: workgroups run two; one NaN sequence
def test_strip_forward_outer_rows(tmp_path, B, T, bad):
    pkg = os.path.join(ROOT, "vq-vae-hmm-model_amd")
    out = {}
    for flag in ("1", "0"):
        f = str(tmp_path / f"strip{flag}.pt")
        subprocess.run([sys.executable, "-c", _RUN, pkg, f, f"{B},{T},{bad}"], check=True, timeout=300,
                       env=dict(os.environ, VQHMM_STRIP=flag, VQHMM_STRIP_HEAD="0"))
        out[flag] = torch.load(f, weights_only=True)
    rows = torch.arange(B * (T + 2))
    clean = (rows // (T + 2)) != bad
    for name, a in out["1"].items():
        b = out["0"][name]
        assert torch.equal(a[clean], b[clean]), name             # bit for bit (no NaN here: equal would fail)
        assert not torch.isnan(a[clean]).any(), name
        assert torch.equal(torch.isnan(a[~clean]), torch.isnan(b[~clean])), name
        same = ~torch.isnan(a[~clean])
        assert torch.equal(a[~clean][same], b[~clean][same]), name  # the NaN sequence's pad rows and channels
