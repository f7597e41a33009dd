"""The memory contract of the core C-ABI entries (include/vqhmm.h), through ctypes on guarded buffers:
every output element is written, nothing is written outside an output or the workspace, and no result
depends on what the workspace held before the call.

Every output and the workspace is a gpu_buffers.guarded allocation: the payload 16 bytes past a 256-byte
boundary and of exactly its own size (a workspace of exactly *_workspace_size bytes, passed with that
ws_bytes), 8 KiB of sentinel on both sides, the payload itself sentinel (NaN words) before the call.
After each call, in this order: rc == 0; synchronize and check every guard; no output element is still
sentinel; the values against the reference the suite already uses for that entry, by its existing rule
(c_oracle bit for bit, hmm_ref.forward_backward_f64 through check_gamma and the logZ rule, hmm_pair_ref
with 2e-5 / 1e-5 / 1e-6, hmm_ref.quantize_f32 with 1e-6 relative on the losses); then the same call
with every workspace byte 0x3C (a small finite float) instead of the sentinel gives the same bits.

Workspace regions, which launch writes them and which reads them (read from the launchers and kernels
before the first run; the runs confirm it).  L = a sequence's clamped length, Lmax = the largest L of
the sequences that share a wave (or workgroup, where stated).

vqhmm_viterbi_f32, vqhmm_viterbi_workspace_size(B, T, K)
  K <= 8 (hmm.hip viterbi_kernel, one launch).  [waves = ceil(B / SPW)][Tr = 64 ceil(T / 64)] 8-byte
    lane ballots, SPW = 64 / KP^2 sequences per wave.
      written  the chain, after chunk c of HC in {16, 32} steps: entries [c HC, c HC + HC) of its own
               wave, c < ceil(Lmax / HC); HC divides 64, so the last entry is < Tr.
      read     the same wave's backtrace, per sequence: whole 64-entry blocks up to the one holding
               L - 1 are copied to LDS (in bounds: Tr is a multiple of 64); entries 1 .. L - 1 are
               used, all written since L <= Lmax.  Block entries past ceil(Lmax / HC) HC may be copied
               unwritten; they are never used, neither as a value nor as an index.
      a sequence of length 0 or 1 reads nothing; waves past the batch do not exist (grid = waves).
  8 < K <= 32 (hmm_wide.hip viterbi_wide_kernel, one launch, one wave per sequence).
    [B][ceil(T / 4)][32] words, byte t & 3 of word [t >> 2][j] = the backpointer of state j at step t.
      written  word [t >> 2][j], j < 16 (K <= 16) or j < 32, when t & 3 == 3 or t == L - 1, 1 <= t < L.
      read     the backtrace copies rows [w0 >> 2, (L - 1) >> 2] whole (32 words each, in bounds) to
               LDS and uses word [t >> 2][s] for 1 <= t < L, s < K the state reached: written.
               Columns j >= 16 at K <= 16, and the whole first row when L = 1, are copied unwritten
               and never used.
  32 < K (hmm_generic.hip viterbi_generic_kernel, one launch, one workgroup per sequence).
    [B][T][K] backpointers of 1 byte (K <= 256) or 2 bytes.
      written  [t][j], 1 <= t < L, all j < K.      read  [t][state], t = L - 1 .. 1, by thread 0 after
      a workgroup barrier.  Nothing else.

vqhmm_fwdbwd_f32, vqhmm_fwdbwd_workspace_size(B, T, K) = 2 B T K floats: al [B][T][K], be [B][T][K]
  K <= 8, resident kernel and both fused streaming forms (fwdbwd_resident_kernel, fwdbwd_kernel<.., FUSE
    = true, NSQ = 1 / 2>): the workspace is not touched (both histories live in LDS).
  K <= 8, streaming-unfused (fwdbwd_kernel<.., false>, one launch, two waves per SPW sequences).
      written  al rows [c HC, c HC + HC) below T by the alpha wave, be rows likewise by the beta wave
               (be[t + 1] holds beta_t), every chunk c < ceil(Lmax / HC), sequences inside the batch.
      read     after a workgroup barrier, the gamma pass: al[t] for t < L and be[t + 1] for t < L - 1,
               both inside the written chunks (L <= Lmax); rows at t >= L are not read (gamma = 0).
  K <= 8, segmented (hmm_seg.hip fwdbwd_seg_kernel, one launch, one workgroup per sequence).
      fast path: not touched.  Exact path (a sequence that left the linear range):
      written  al[t], t < L, by wave 0; be[t], t < L, by wave 1 (be[L - 1] = 0 first).
      read     after a workgroup barrier, al[t] + be[t] for t < L.
  8 < K <= 32 (hmm_wide.hip fwdbwd_wide_kernel, one launch, two waves per sequence).
      written  al[t], t < L, wave 0; be[t], t < L, wave 1.   read  al[t] + be[t], t < L, after the barrier.
  32 < K (hmm_generic.hip fwdbwd_generic_kernel, one launch): only the first B T K floats.
      written  al[t][j], t < L, in the forward sweep.   read  al[t][j], t = L - 1 .. 0, in the backward
      sweep of the same workgroup, after barriers.

vqhmm_filter_f32: no workspace.

vqhmm_fwdbwd_xi_f32, vqhmm_fwdbwd_xi_workspace_size(B, T, K) = the forward-backward workspace rounded
  up to 256 bytes, then filt [B][T][K], then loglik [B]
      launch 1 (launch_fwdbwd)      the first region, exactly as above.
      launch 2 (filter kernels)     writes every element of filt (rows t >= L zeroed, row 0 and rows
                                    1 .. L - 1 from the chain) and loglik[b]; reads none of them.
      launch 3 (xi_kernel)          reads filt rows p - 1 of its positions p (row -1 replaced by 0) and
                                    the gamma output; never loglik, never the first region.
      The padding between the first region and filt is neither written nor read.

vqhmm_vq_argmin_f32: no workspace.

vqhmm_vq_quantize_f32, vqhmm_vq_quantize_workspace_size = max(resident waves, ceil(B T / 256)) doubles
      launch 1  row-load kernel (vq_rows_kernel<.., QUANT>): every wave gw < resident waves writes
                part[gw] (a wave without tiles writes 0); or argmin + vq_quantize_gather_kernel:
                block i < ceil(B T / 256) writes part[i].  Neither reads the workspace.
      launch 2  vq_sse_finalize_kernel reads part[0, np), np = the count launch 1 wrote.

vqhmm_prior_viterbi_f32, vqhmm_prior_viterbi_workspace_size = 256 bytes + the Viterbi workspace
      launch 1  log_softmax of log_prior writes floats [0, K) of the first 256 bytes.
      launch 2  prior_viterbi_kernel reads those K floats; the ballots behind them are written and
                read exactly as viterbi_kernel's above (chunks up to the workgroup's longest length,
                which is still below Tr), by chain waves whose first sequence is inside the batch.

vqhmm_argmax_f32: no workspace.

No region is used before it is written, and no workspace word is ever used as an index except the
backpointers listed as written above.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import hmm_pair_ref as PR
from gpu_buffers import check_all, guarded
from oracle import c_oracle, hmm_ref
from test_gpu_dispatch_edges import bits, check_logZ
from test_gpu_hmm import FB_KERNELS, check_gamma, gpu, log_softmax, random_hmm, use_fb_kernel
from test_gpu_hmm_pair import rel_ok

pytestmark = pytest.mark.gpu

LANE_K = (1, 2, 3, 4, 5, 8)
LANE_BT = ((3, 1), (5, 33), (7, 70))
WIDE_K = (9, 16, 17, 32)
WIDE_BT = ((3, 1), (3, 45))
GENERIC = [(33, 2, 9), (64, 3, 12), (257, 2, 9), (300, 3, 7)]
SPANS = [(32, 1, 5), (8, 1, 65)]  # one workgroup's last, partly filled span of positions
LANE = [(K, B, T) for K in LANE_K for B, T in LANE_BT]
WIDE = [(K, B, T) for K in WIDE_K for B, T in WIDE_BT]
PAIR_SHAPES = LANE + WIDE + SPANS


def lengths_for(B, T):
    """T, 0 and 1 first, then one value each side of the 64-, 32- and 16-step chunk boundaries that fit
    below T (T itself is the far side of the boundary at T - 1)."""
    extra = [v for v in (63, 65, 31, 33, 15, 17) if 1 < v < T]
    return np.array(([T, 0, 1] + extra)[:B], np.int64)


@functools.lru_cache(maxsize=None)
def hmm_case(K, B, T):
    """Tables, lengths and every reference of one shape, computed once and shared; read-only."""
    log_pi, log_A, em = random_hmm(1000 * K + 10 * B + T, B, T, K)
    L = lengths_for(B, T)
    c = dict(log_pi=log_pi, log_A=log_A, em=em, L=L, vit=c_oracle.viterbi(log_pi, log_A, em, L),
             fb=hmm_ref.forward_backward_f64(log_pi, log_A, em, L))
    if K <= 32:
        c["pair"] = PR.pair_ref(log_pi, log_A, em, L)
    return c


def lib_and_ext():
    from vqhmm import _ext
    return _ext.load(), _ext


_dummy = []


def dptr(t):
    """Device pointer of an input tensor; an empty input still gets a valid, non-null one."""
    from vqhmm import _ext
    if t.numel():
        return _ext.ptr(t)
    if not _dummy:
        _dummy.append(guarded((4,), torch.float32))
    return _dummy[0].ptr


def run_guarded(call, out_specs, ws_bytes, expect_written=True):
    """call(outs, ws) -> rc with outs a dict of Guarded and ws a Guarded of exactly ws_bytes (or None),
    twice: on a sentinel-poisoned workspace, then on one whose bytes are all 0x3C.  Checks rc, every
    guard, that no output element is left as sentinel, and that both runs give the same bits.
    Returns the first run's outputs as numpy arrays."""
    runs = []
    for fill in (None, 0x3C):
        outs = {name: guarded(shape, dtype) for name, (shape, dtype) in out_specs.items()}
        ws = None if ws_bytes is None else guarded(int(ws_bytes), torch.uint8)
        if ws is not None and fill is not None:
            ws.poison(fill)
        rc = call(outs, ws)
        assert rc == 0, f"rc = {rc}"
        check_all(*outs.values(), ws)
        for name, g in outs.items():
            miss = g.unwritten()
            if expect_written:
                assert not bool(miss.any()), (f"{name}: {int(miss.sum())} of {miss.numel()} elements never written, "
                                              f"first at {miss.nonzero()[0].tolist()}")
            else:
                assert bool(miss.all()), f"{name}: written by a call that must not launch"
        runs.append({name: g.t.cpu().numpy() for name, g in outs.items()})
    for name in out_specs:
        assert np.array_equal(bits(runs[0][name]), bits(runs[1][name])), f"{name} depends on the workspace's contents"
    return runs[0]


def hmm_inputs(c):
    lp, lA, e = gpu(c["log_pi"], c["log_A"], c["em"])
    return lp, lA, e, torch.from_numpy(c["L"]).cuda()


# ------------------------------------------------------------------------------ runners, one per entry
def run_viterbi(log_pi, log_A, em, L, B, T, K, expect_written=True):
    lib, ext = lib_and_ext()
    nb = lib.vqhmm_viterbi_workspace_size(B, T, K)

    def call(o, ws):
        return lib.vqhmm_viterbi_f32(dptr(log_pi), dptr(log_A), dptr(em), dptr(L), B, T, K, o["path"].ptr,
                                     o["score"].ptr, ws.ptr, nb, ext.stream_ptr())
    return run_guarded(call, dict(path=((B, T), torch.int32), score=((B,), torch.float32)), nb, expect_written)


def run_fwdbwd(log_pi, log_A, em, L, B, T, K, expect_written=True):
    lib, ext = lib_and_ext()
    nb = lib.vqhmm_fwdbwd_workspace_size(B, T, K)

    def call(o, ws):
        return lib.vqhmm_fwdbwd_f32(dptr(log_pi), dptr(log_A), dptr(em), dptr(L), B, T, K, o["gamma"].ptr,
                                    o["logZ"].ptr, ws.ptr, nb, ext.stream_ptr())
    return run_guarded(call, dict(gamma=((B, T, K), torch.float32), logZ=((B,), torch.float32)), nb, expect_written)


def run_filter(log_pi, log_A, em, L, B, T, K, expect_written=True):
    lib, ext = lib_and_ext()

    def call(o, ws):
        return lib.vqhmm_filter_f32(dptr(log_pi), dptr(log_A), dptr(em), dptr(L), B, T, K, o["filt"].ptr,
                                    o["loglik"].ptr, ext.stream_ptr())
    return run_guarded(call, dict(filt=((B, T, K), torch.float32), loglik=((B,), torch.float32)), None, expect_written)


def run_xi(log_pi, log_A, em, L, B, T, K, expect_written=True):
    lib, ext = lib_and_ext()
    nb = lib.vqhmm_fwdbwd_xi_workspace_size(B, T, K)

    def call(o, ws):
        return lib.vqhmm_fwdbwd_xi_f32(dptr(log_pi), dptr(log_A), dptr(em), dptr(L), B, T, K, o["gamma"].ptr,
                                       o["xi"].ptr, o["logZ"].ptr, ws.ptr, nb, ext.stream_ptr())
    specs = dict(gamma=((B, T, K), torch.float32), xi=((B, T, K, K), torch.float32), logZ=((B,), torch.float32))
    return run_guarded(call, specs, nb, expect_written)


def run_argmin(z, cb, B, Dv, T, K, want_dmin, expect_written=True):
    lib, ext = lib_and_ext()
    specs = dict(idx=((B, T), torch.int32))
    if want_dmin:
        specs["dmin"] = ((B, T), torch.float32)

    def call(o, ws):
        return lib.vqhmm_vq_argmin_f32(dptr(z), B, Dv, T, dptr(cb), K, o["idx"].ptr,
                                       o["dmin"].ptr if want_dmin else ctypes.c_void_p(0), ext.stream_ptr())
    return run_guarded(call, specs, None, expect_written)


def run_quantize(z, cb, B, Dv, T, K, written=("idx", "z_q_st", "sse")):
    """`written`: the outputs the call must write (an empty problem writes only sse = 0: the empty sum)."""
    lib, ext = lib_and_ext()
    nb = lib.vqhmm_vq_quantize_workspace_size(B, Dv, T, K)
    assert nb >= 8
    specs = dict(idx=((B, T), torch.int32), z_q_st=((B, Dv, T), torch.float32), sse=((), torch.float64))
    runs = []
    for fill in (None, 0x3C):
        o = {name: guarded(shape, dtype) for name, (shape, dtype) in specs.items()}
        ws = guarded(nb, torch.uint8)
        if fill is not None:
            ws.poison(fill)
        rc = lib.vqhmm_vq_quantize_f32(dptr(z), B, Dv, T, dptr(cb), K, o["idx"].ptr, o["z_q_st"].ptr, o["sse"].ptr,
                                       ws.ptr, nb, ext.stream_ptr())
        assert rc == 0, f"rc = {rc}"
        check_all(*o.values(), ws)
        for name, g in o.items():
            miss = g.unwritten()
            if name in written:
                assert not bool(miss.any()), f"{name}: {int(miss.sum())} of {miss.numel()} elements never written"
            else:
                assert bool(miss.all()), f"{name}: written by an empty problem"
        runs.append({name: g.t.cpu().numpy() for name, g in o.items()})
    for name in specs:
        assert np.array_equal(bits(runs[0][name]), bits(runs[1][name])), f"{name} depends on the workspace's contents"
    return runs[0]


def prior_params(prior):
    """The parameter pointer array and dims as vqhmm/infer.py's prior_viterbi builds them."""
    from vqhmm import _ext
    from vqhmm.model import _ptr_array
    lin0, lin2 = prior.transition_net[0], prior.transition_net[2]
    d = _ext.Dims(1, 1, prior.K, 1, prior.u_dim, lin0.weight.shape[0])
    w = [None] * _ext.NPARAMS
    w[6:11] = [prior.log_prior, lin0.weight, lin0.bias, lin2.weight, lin2.bias]
    keep = [t.detach() if t is not None else None for t in w]
    return d, _ptr_array(keep), keep


def run_prior_viterbi(prior, u, em, L, B, T, expect_written=True):
    lib, ext = lib_and_ext()
    d, w, keep = prior_params(prior)
    nb = lib.vqhmm_prior_viterbi_workspace_size(ctypes.byref(d), B, T)

    def call(o, ws):
        return lib.vqhmm_prior_viterbi_f32(ctypes.byref(d), w, dptr(u), 0, dptr(em), dptr(L), B, T, o["path"].ptr,
                                           o["score"].ptr, ws.ptr, nb, ext.stream_ptr())
    out = run_guarded(call, dict(path=((B, T), torch.int32), score=((B,), torch.float32)), nb, expect_written)
    del keep
    return out


def run_argmax(q, B, K, T, expect_written=True):
    lib, ext = lib_and_ext()

    def call(o, ws):
        return lib.vqhmm_argmax_f32(dptr(q), B, K, T, o["idx"].ptr, ext.stream_ptr())
    return run_guarded(call, dict(idx=((B, T), torch.int32)), None, expect_written)


# ------------------------------------------------------------------------------ value checks
def check_viterbi(out, c):
    rp, rs = c["vit"]
    assert np.array_equal(out["path"], rp)
    assert np.array_equal(bits(out["score"]), bits(rs))


def check_fwdbwd(out, c, T):
    check_gamma(out["gamma"], c["fb"][0])
    check_logZ(out["logZ"], c["fb"][1], c["L"])
    past = np.arange(T)[None, :] >= c["L"][:, None]
    assert np.all(out["gamma"][past] == 0)


# ------------------------------------------------------------------------------ Viterbi
@pytest.mark.parametrize("K,B,T", LANE + WIDE + GENERIC + SPANS)
def test_viterbi(K, B, T):
    c = hmm_case(K, B, T)
    check_viterbi(run_viterbi(*hmm_inputs(c), B, T, K), c)


# ------------------------------------------------------------------------------ forward-backward
@pytest.mark.parametrize("K,B,T", LANE + WIDE + GENERIC)
def test_fwdbwd_default_kernel(K, B, T):
    c = hmm_case(K, B, T)
    check_fwdbwd(run_fwdbwd(*hmm_inputs(c), B, T, K), c, T)


@pytest.mark.parametrize("kernel", FB_KERNELS)
@pytest.mark.parametrize("K,B,T", [(K, B, T) for K in (3, 4, 8) for B, T in ((5, 70), (3, 130))])
def test_fwdbwd_every_lane_kernel(K, B, T, kernel, monkeypatch):
    use_fb_kernel(monkeypatch, kernel)
    c = hmm_case(K, B, T)
    check_fwdbwd(run_fwdbwd(*hmm_inputs(c), B, T, K), c, T)


def test_fwdbwd_segmented_exact_path(monkeypatch):
    """test_forward_backward_extreme_tables' batch at K = 8 under the parallel-in-time kernel: four of
    its sequences leave the linear range and take the exact path, which is the only one that writes and
    reads that kernel's workspace."""
    use_fb_kernel(monkeypatch, "segmented")
    K, B, T = 8, 6, 150
    rng = np.random.default_rng(K + 100)
    log_pi, log_A, em = random_hmm(K + 200, B, T, K)
    log_A = log_A.astype(np.float64)
    em = em.astype(np.float64)
    tri = np.triu(np.ones((K, K), bool))
    la = np.where(tri, log_A[0], -np.inf)
    log_A[0] = la - np.logaddexp.reduce(la, axis=-1, keepdims=True)   # b0: left-to-right
    em[1] = em[1] * 50.0 - 1000.0                                      # b1: huge negative emissions
    em[2, 40:60] *= 150.0                                              # b2: 300+ nat spread
    log_A[3] = log_softmax(rng.standard_normal((T, K, K)) * 80.0)      # b3: near-deterministic
    L = np.array([T, T, T, T, 77, 1], np.int64)
    log_A = log_A.astype(np.float32)
    em = em.astype(np.float32)
    out = run_fwdbwd(*gpu(log_pi, log_A, em), torch.from_numpy(L).cuda(), B, T, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        rg, rz = hmm_ref.forward_backward_f64(log_pi, log_A, em, L)
    check_gamma(out["gamma"], rg)
    assert np.all(np.abs(out["logZ"] - rz) <= 1e-5 * np.maximum(1.0, np.abs(rz)))


# ------------------------------------------------------------------------------ filter, pairwise posteriors
@pytest.mark.parametrize("K,B,T", PAIR_SHAPES)
def test_filter(K, B, T):
    c = hmm_case(K, B, T)
    out = run_filter(*hmm_inputs(c), B, T, K)
    ref = c["pair"]
    rel_ok(out["loglik"], ref["loglik"])
    assert np.abs(out["filt"] - ref["filt"]).max() <= 1e-5
    for b, n in enumerate(c["L"]):
        assert not out["filt"][b, n:].any()


@pytest.mark.parametrize("K,B,T", PAIR_SHAPES)
def test_fwdbwd_xi(K, B, T):
    """K in {4, 8, 16, 32}: xi_kernel<true> (16-byte loads and stores), the other K <false>."""
    c = hmm_case(K, B, T)
    out = run_xi(*hmm_inputs(c), B, T, K)
    ref = c["pair"]
    check_fwdbwd(out, c, T)
    rel_ok(out["logZ"], ref["logZ"])
    xi = out["xi"]
    assert not np.isnan(xi).any()
    assert np.abs(xi - ref["xi"]).max() <= 2e-5
    assert np.abs(xi.astype(np.float64).sum(2) - out["gamma"])[:, 1:].max(initial=0) <= 1e-6
    for b, n in enumerate(c["L"]):
        assert not xi[b, 0].any() and not xi[b, n:].any()
    plain = run_fwdbwd(*hmm_inputs(c), B, T, K)  # "the same launch: the same bits"
    assert np.array_equal(bits(out["gamma"]), bits(plain["gamma"])) and np.array_equal(bits(out["logZ"]), bits(plain["logZ"]))


# ------------------------------------------------------------------------------ VQ
ROW_LOAD = [(3, 4, 20, 3), (1, 16, 36, 16), (1, 64, 12, 32)]
TILE_32 = [(2, 8, 37, 8), (2, 5, 41, 3)]
VALU = [(2, 65, 37, 3), (1, 100, 7, 8), (1, 8, 33, 40)]


@functools.lru_cache(maxsize=None)
def vq_case(B, Dv, T, K):
    rng = np.random.default_rng(B * 1000 + Dv * 100 + T + K)
    z = rng.standard_normal((B, Dv, T)).astype(np.float32)
    cb = rng.standard_normal((K, Dv)).astype(np.float32)
    return z, cb, c_oracle.vq_argmin(z, cb, want_dmin=True)


@pytest.mark.parametrize("want_dmin", [True, False])
@pytest.mark.parametrize("B,Dv,T,K", ROW_LOAD + TILE_32 + VALU)
def test_vq_argmin(B, Dv, T, K, want_dmin):
    z, cb, (ridx, rd) = vq_case(B, Dv, T, K)
    out = run_argmin(*gpu(z, cb), B, Dv, T, K, want_dmin)
    assert np.array_equal(out["idx"], ridx)
    if want_dmin:
        assert np.array_equal(bits(out["dmin"]), bits(rd))


@pytest.mark.parametrize("B,Dv,T,K", ROW_LOAD + TILE_32 + VALU)
def test_vq_quantize(B, Dv, T, K):
    """The fused epilogue (ROW_LOAD) and the argmin + gather route (the others)."""
    z, cb, (ridx, _) = vq_case(B, Dv, T, K)
    out = run_quantize(*gpu(z, cb), B, Dv, T, K)
    beta = 0.25
    ref = hmm_ref.quantize_f32(z, cb, ridx, beta)
    assert np.array_equal(out["idx"], ridx)
    assert np.array_equal(bits(out["z_q_st"]), bits(ref["z_q_st"]))
    mse = float(out["sse"]) / z.size
    assert abs(beta * mse - ref["commit"]) <= 1e-6 * ref["commit"]
    assert abs(mse - ref["codebook"]) <= 1e-6 * ref["codebook"]


# ------------------------------------------------------------------------------ fused Prior -> Viterbi, argmax
def make_prior(K):
    import vqhmm
    torch.manual_seed(1000 * K + 128 + 4)
    prior = vqhmm.Prior(K, u_dim=4, trans_hidden=128)
    with torch.no_grad():  # sharper tables than the default init: paths that actually switch
        prior.transition_net[2].weight.mul_(4.0)
        prior.log_prior.normal_()
    return prior.cuda()


@pytest.mark.parametrize("K", [3, 8])
def test_prior_viterbi(K):
    import vqhmm
    B, T = 5, 33
    prior = make_prior(K)
    u = (2.0 * torch.randn(B, 4, T)).cuda()
    em = torch.log_softmax(3.0 * torch.randn(B, T, K), dim=2).cuda()
    L = torch.from_numpy(lengths_for(B, T)).cuda()
    out = run_prior_viterbi(prior, u, em, L, B, T)
    with torch.no_grad():
        log_pi, log_A = prior(u)
    ref = run_viterbi(log_pi.contiguous(), log_A.contiguous(), em, L, B, T, K)
    assert np.array_equal(out["path"], ref["path"]) and np.array_equal(bits(out["score"]), bits(ref["score"]))
    rp, rs = c_oracle.viterbi(log_pi.cpu().numpy(), log_A.cpu().numpy(), em.cpu().numpy(), L.cpu().numpy())
    assert np.array_equal(out["path"], rp) and np.array_equal(bits(out["score"]), bits(rs))
    assert len(np.unique(rp[rp >= 0])) > 1


@pytest.mark.parametrize("K", [3, 8])
def test_argmax(K):
    B, T = 5, 33
    q = torch.softmax(torch.randn(B, K, T, generator=torch.Generator().manual_seed(K)), dim=1).cuda()
    out = run_argmax(q, B, K, T)
    assert np.array_equal(out["idx"], torch.argmax(q, dim=1).cpu().numpy())


# ------------------------------------------------------------------------------ empty problems
EMPTY = [(0, 5), (3, 0)]


def empty_hmm(B, T, K):
    log_pi, log_A, em = random_hmm(K, B, T, K)
    return (*gpu(log_pi, log_A, em), torch.full((B,), T, dtype=torch.int64).cuda())


@pytest.mark.parametrize("B,T", EMPTY)
@pytest.mark.parametrize("K", [3, 16, 40])
def test_empty_hmm_problems_launch_nothing(K, B, T):
    """B == 0 or T == 0: VQHMM_OK, and every payload (score, logZ and loglik of B > 0 included) and
    every guard still all sentinel."""
    args = empty_hmm(B, T, K)
    run_viterbi(*args, B, T, K, expect_written=False)
    run_fwdbwd(*args, B, T, K, expect_written=False)
    if K <= 32:
        run_filter(*args, B, T, K, expect_written=False)
        run_xi(*args, B, T, K, expect_written=False)


@pytest.mark.parametrize("B,T", EMPTY)
def test_empty_vq_problems_launch_nothing(B, T):
    Dv, K = 8, 5
    z, cb = gpu(np.zeros((B, Dv, T), np.float32), np.ones((K, Dv), np.float32))
    run_argmin(z, cb, B, Dv, T, K, True, expect_written=False)
    run_argmin(z, cb, B, Dv, T, K, False, expect_written=False)
    # quantize defines *sse as a sum over (b, d, t): the empty sum, 0, is written; nothing else is
    out = run_quantize(z, cb, B, Dv, T, K, written=("sse",))
    assert float(out["sse"]) == 0.0


@pytest.mark.parametrize("B,T", EMPTY)
def test_empty_prior_viterbi_and_argmax_launch_nothing(B, T):
    K = 3
    prior = make_prior(K)
    u = torch.zeros(B, 4, T).cuda()
    em = torch.zeros(B, T, K).cuda()
    L = torch.full((B,), T, dtype=torch.int64).cuda()
    run_prior_viterbi(prior, u, em, L, B, T, expect_written=False)
    run_argmax(torch.zeros(B, K, T).cuda(), B, K, T, expect_written=False)


# ------------------------------------------------------------------------------ T = 0 in the Python wrappers
@pytest.mark.parametrize("K", [3, 16, 40])
def test_wrappers_on_length_zero_batches(K):
    """B > 0, T = 0: the C entries launch and write nothing, and the wrappers return what a sequence of
    length 0 gets from the kernels: score = -inf, logZ = loglik = NaN, empty (B, 0, ..) tensors beside
    them.  The fresh allocations are poisoned first, so a wrapper that returned an unwritten
    torch.empty block would hand the poison back."""
    import vqhmm
    B = 4
    for _ in range(8):  # blocks of the sizes the wrappers ask for, freed with a non-zero, finite content
        torch.full((B,), 7.0, device="cuda")
    log_pi = torch.log_softmax(torch.randn(K), 0).cuda()
    log_A = torch.zeros(B, 0, K, K, device="cuda")
    em = torch.zeros(B, 0, K, device="cuda")
    for lengths in (None, torch.zeros(B, dtype=torch.int64)):
        path, score = vqhmm.viterbi(log_pi, log_A, em, lengths)
        assert path.shape == (B, 0) and path.dtype == torch.int32
        assert score.shape == (B,) and score.dtype == torch.float32 and bool((score == float("-inf")).all())
        gamma, logZ = vqhmm.forward_backward(log_pi, log_A, em, lengths)
        assert gamma.shape == (B, 0, K) and logZ.shape == (B,) and bool(torch.isnan(logZ).all())
        if K <= 32:
            ga, za = vqhmm.forward_backward(log_pi, log_A, em.clone().requires_grad_(True), lengths)  # autograd route
            assert ga.shape == (B, 0, K) and za.shape == (B,) and bool(torch.isnan(za).all())
            filt, loglik = vqhmm.forward_filter(log_pi, log_A, em, lengths)
            assert filt.shape == (B, 0, K) and loglik.shape == (B,) and bool(torch.isnan(loglik).all())
            g2, xi, z2 = vqhmm.pairwise_posteriors(log_pi, log_A, em, lengths)
            assert g2.shape == (B, 0, K) and xi.shape == (B, 0, K, K) and z2.shape == (B,)
            assert bool(torch.isnan(z2).all())
        else:  # the K limits of these three hold at T = 0 as at any T
            with pytest.raises(RuntimeError, match="32"):
                vqhmm.forward_backward(log_pi, log_A, em.clone().requires_grad_(True), lengths)
            with pytest.raises(RuntimeError):
                vqhmm.forward_filter(log_pi, log_A, em, lengths)
            with pytest.raises(RuntimeError, match="32"):
                vqhmm.pairwise_posteriors(log_pi, log_A, em, lengths)
