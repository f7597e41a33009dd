// vqhmm_backtest_f32 / vqhmm_backtest_bwd_f32 (contract: include/vqhmm.h, "Historical back-test"): the wealth
// recursion of a regime-conditional portfolio over B windows x P policies, its twelve statistics, and the
// gradient of any function of them with respect to the weight tables.
//
// The recursion has no true recurrence but a scan: the holdings of step t are a function of probs[t_k - lag] and
// W alone, so 1 + rho_t is computed for every step independently, V is a prefix product, the peak a prefix
// maximum, the rest reductions.  Plan:
//   a workgroup takes one window and nw policies (one wave = one policy); per 64-step chunk the workgroup stages
//     the chunk's returns rows once (LDS, odd row stride) and looks at every returns / probs value of the chunk for
//     a non-finite one;
//   the wave's lanes first run over the (date, asset) pairs of the chunk's rebalance dates, and of the last date
//     before the chunk, and leave h_k[d] = sum_s q_k[s] W[s,d] (hard: W[argmax q_k, d]) in a wave-private fp64 LDS
//     tile of at most 65 rows (odd stride); q_k is read from global memory (the lanes of a date share the
//     addresses), W[p] sits in the wave's LDS.  A date's row is a function of its probs row and W only, so it does
//     not matter which chunk computes it;
//   then lane l owns step t0 + l: g = h . r from its date's row and its returns row, on a rebalance date tau =
//     |h_k - h_{k-1}|_1 from the row above, and 1 + rho in fp64;
//   a Kogge-Stone product over the lanes with the carry of the previous chunk gives V, a (value, index) maximum
//     scan gives the running peak and its step; each lane keeps its own deepest drawdown and its partial sums,
//     which are reduced across the lanes once, after the last chunk.
// Nothing depends on the tile a window or a policy falls in, on T beyond the window's length, or on whether
// wealth is written: stats[b, p] has the same bits in every call that contains (b, p).
//
// Backward: the same forward pass (V_L, drawdown, i*, j*), then a second pass over the chunks: lane l forms the
// adjoint a_t of its step's net return, alpha_t = a_t (1 - c tau_t) and, on a rebalance date, u_t; then the lanes
// turn to the S D entries of dW[p] and each adds, over the chunk's steps,
//     alpha_t q_t[s] r[t, d] + u_t sign(h_t - h'_t)[d] (q_t[s] - q'_t[s])
// which is sum_k q_k[s] abar_k[d] of the contract regrouped by step (u_k sign_k enters abar_k with + and
// abar_{k-1} with -); the step's date is wave-uniform there, so q is one coalesced load over s.  A wave keeps
// dW[p] in fp64 in LDS over the BT_TB windows of its tile and writes one partial per (tile, policy); a second
// launch adds the tiles in order.
#include "kernels.h"

namespace vqhmm {

namespace {
constexpr int BT_CH = 64;                    // steps per chunk: one per lane
constexpr int BT_ROWS = BT_CH + 1;           // rows of the holdings tile: the chunk's dates and the one before
constexpr int BT_TB = 8;                     // windows per tile of the backward pass (a function of nothing else)
constexpr size_t BT_LDS_MAX = 156 * 1024;    // of the CU's 160 KB
constexpr size_t BT_LDS_SOFT = 64 * 1024;    // fewer waves per workgroup above this
constexpr int64_t BT_MAX_T = 1 << 28;
constexpr int64_t BT_MAX_P = 1 << 24;
constexpr int64_t BT_MAX_BLOCKS = (int64_t(1) << 31) - 1;

struct BtArgs {
  const float* ret;
  const float* probs;
  const int64_t* lengths;
  const float* W;
  const int32_t* reb;
  const float* txc;
  double* stats;
  float* wealth;
  const double* gstats;
  double* part;
  int64_t B, T;
  int S, D, P, lag, hard;
  int PT;                       // policy tiles = ceil(P / waves per workgroup)
  int SD;                       // odd row stride of the D-wide LDS rows (floats, and doubles in the tile)
  int wdbl, wflt;               // doubles / floats of LDS per wave
};

struct BtLds {
  float* rt;      // (64, SD) the chunk's returns, shared by the workgroup
  int* flag;      // a non-finite input was seen in this window
  float* Wt;      // (S, SD) the wave's weight table
  int* arg;       // (65) hard: argmax q_k per tile row (-1: no date)
  double* H;      // (65, SD) h_k per tile row
  double* dW;     // (S D) the wave's gradient tile (backward)
  double* al;     // (64) alpha_t
  double* u;      // (64) u_t
};

struct BtChunk {
  int km1;        // the date index of tile row 0 (the last date before the chunk; -1: none, the row is 0)
};

struct BtRes {
  double fin, sum, sumsq, nneg, sumneg, sumsqneg, npos, dd, turn;
  int ip, jt;
};

__host__ __device__ __forceinline__ int bt_odd(int v) { return v | 1; }

__device__ __forceinline__ void bt_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool bt_nonfinite(float v) { return !(fabsf(v) < __builtin_inff()); }

// the chunk's returns rows -> rt (rows past the length zeroed); with check, every returns and probs value of the
// chunk inside the length is tested
__device__ __forceinline__ void bt_stage(const BtArgs& a, const BtLds& l, int64_t b, int t0, int L, bool check,
                                         int tid, int nthr) {
  const int D = a.D, S = a.S;
  const int rows = min(BT_CH, L - t0);
  const int n = rows * D;
  const float* src = a.ret + (b * a.T + t0) * D;
  bool bad = false;
  for (int e = tid; e < BT_CH * D; e += nthr) {
    const int r = e / D, d = e - r * D;
    float v = 0.f;
    if (e < n) {
      v = src[e];
      bad |= bt_nonfinite(v);
    }
    l.rt[r * a.SD + d] = v;
  }
  if (check) {
    const float* ps = a.probs + (b * a.T + t0) * S;
    for (int e = tid; e < rows * S; e += nthr) bad |= bt_nonfinite(ps[e]);
    if (bad) *l.flag = 1;
  }
}

// the holdings of the chunk's dates (steps [t0, tend)) and of the last date before it -> the tile; date k trades at
// step lag + k R on probs row k R
__device__ __forceinline__ BtChunk bt_holdings(const BtArgs& a, const BtLds& l, int64_t b, int t0, int tend, int R,
                                               int lane) {
  const int S = a.S, D = a.D, SD = a.SD;
  const int x = t0 - a.lag;
  const int k0 = x > 0 ? (x - 1) / R + 1 : 0;                          // the first date at or after t0
  const int kend = tend > a.lag ? (tend - 1 - a.lag) / R + 1 : 0;     // one past the last date before tend
  BtChunk ch;
  ch.km1 = k0 - 1;
  const int nrows = (kend > k0 ? kend - k0 : 0) + 1;                   // <= 65
  const int npair = nrows * D;
  for (int idx = lane; idx < npair; idx += 64) {
    const int j = idx / D, d = idx - j * D;
    const int k = ch.km1 + j;
    double h = 0.0;
    int arg = -1;
    if (k >= 0) {
      const float* q = a.probs + (b * a.T + (int64_t)k * R) * S;
      if (a.hard) {
        float best = q[0];
        arg = 0;
        for (int s = 1; s < S; ++s) {
          const float v = q[s];
          if (v > best) { best = v; arg = s; }
        }
        h = (double)l.Wt[arg * SD + d];
      } else {
        for (int s = 0; s < S; ++s) h = fma((double)q[s], (double)l.Wt[s * SD + d], h);
      }
    }
    l.H[j * SD + d] = h;
    if (d == 0) l.arg[j] = arg;
  }
  bt_wave_sync();
  return ch;
}

// step t of (b, p), one lane: g = h . r with its date's holdings and, on the date itself, the turnover against the
// previous date's.  -> g, tau, is_reb
__device__ __forceinline__ void bt_step(const BtArgs& a, const BtLds& l, const BtChunk& ch, int t, bool valid, int R,
                                        int lane, double& g, double& tau, bool& is_reb) {
  const int D = a.D, SD = a.SD;
  g = 0.0;
  tau = 0.0;
  is_reb = false;
  if (valid && t >= a.lag) {
    const int rel = t - a.lag, k = rel / R;
    is_reb = rel - k * R == 0;
    const double* hk = l.H + (k - ch.km1) * SD;     // row >= 1 on a date
    const float* rr = l.rt + lane * SD;
    if (is_reb) {
      for (int d = 0; d < D; ++d) {
        const double h = hk[d];
        g = fma(h, (double)rr[d], g);
        tau += fabs(h - hk[d - SD]);
      }
    } else {
      for (int d = 0; d < D; ++d) g = fma(hk[d], (double)rr[d], g);
    }
  }
}

// the forward pass of (b, p) by one wave; every wave of the workgroup calls it with the same b and L (barriers).
// Returns the statistics in every lane; writes wealth when asked (live waves only).
__device__ __forceinline__ void bt_forward(const BtArgs& a, const BtLds& l, int64_t b, int p, int L, int R, double c,
                                           float* wealth_row, int tid, int nthr, BtRes& res) {
  const int lane = tid & 63;
  double carryV = 1.0, carryPk = 1.0;
  int carryI = -1;
  double sum = 0.0, sumsq = 0.0, sumneg = 0.0, sumsqneg = 0.0, turn = 0.0, nneg = 0.0, npos = 0.0;
  double bdd = 0.0, fin = 1.0;
  int bi = -1, bj = -1;
  for (int t0 = 0; t0 < L; t0 += BT_CH) {
    __syncthreads();   // the previous chunk's reads of rt are done
    bt_stage(a, l, b, t0, L, true, tid, nthr);
    __syncthreads();
    const int t = t0 + lane;
    const bool valid = t < L;
    const BtChunk ch = bt_holdings(a, l, b, t0, min(t0 + BT_CH, L), R, lane);
    double g, tau;
    bool is_reb;
    bt_step(a, l, ch, t, valid, R, lane, g, tau, is_reb);
    const double m = (1.0 - c * tau) * (1.0 + g);
    const double rho = valid ? m - 1.0 : 0.0;
    const double x = 1.0 + rho;
    if (valid) {
      sum += rho;
      sumsq += rho * rho;
      if (rho < 0.0) { nneg += 1.0; sumneg += rho; sumsqneg += rho * rho; }
      if (rho > 0.0) npos += 1.0;
      turn += tau;
    }
    // V: inclusive product over the lanes, times the carry
    double pr = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double y = __shfl_up(pr, o);
      if (lane >= o) pr *= y;
    }
    const double V = carryV * pr;
    // the running peak and its step: (value, index) scan, the earlier of two equal values stays
    double pk = valid ? V : -__builtin_inf();
    int pi = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double yv = __shfl_up(pk, o);
      const int yi = __shfl_up(pi, o);
      if (lane >= o && !(pk > yv)) { pk = yv; pi = yi; }
    }
    if (!(pk > carryPk)) { pk = carryPk; pi = carryI; }
    if (valid && V < pk) {
      const double d = 1.0 - V / pk;
      if (d > bdd) { bdd = d; bi = pi; bj = t; }
    }
    if (wealth_row && t < a.T) wealth_row[t] = valid ? (float)V : 0.f;
    const int last = min(BT_CH, L - t0) - 1;
    fin = __shfl(V, last);
    carryV = __shfl(V, 63);
    carryPk = __shfl(pk, 63);
    carryI = __shfl(pi, 63);
  }
  // the lanes' sums and the deepest drawdown (the earliest trough among equal ones), once
  res.sum = wave_sum_dpp(sum);
  res.sumsq = wave_sum_dpp(sumsq);
  res.sumneg = wave_sum_dpp(sumneg);
  res.sumsqneg = wave_sum_dpp(sumsqneg);
  res.turn = wave_sum_dpp(turn);
  res.nneg = wave_sum_dpp(nneg);
  res.npos = wave_sum_dpp(npos);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = __shfl_xor(bdd, o);
    const int oi = __shfl_xor(bi, o), oj = __shfl_xor(bj, o);
    if (od > bdd || (od == bdd && oj < bj)) { bdd = od; bi = oi; bj = oj; }
  }
  res.dd = bdd;
  res.ip = bdd > 0.0 ? bi : -1;
  res.jt = bdd > 0.0 ? bj : -1;
  res.fin = fin;
}

__device__ __forceinline__ BtLds bt_carve(const BtArgs& a, double* smem, int nw, int wave, bool bwd) {
  BtLds l;
  double* wd = smem + wave * a.wdbl;
  l.H = wd;
  l.dW = l.H + BT_ROWS * a.SD;
  l.al = l.dW + (bwd ? a.S * a.D : 0);
  l.u = l.al + BT_CH;
  float* fl = reinterpret_cast<float*>(smem + nw * a.wdbl);
  l.rt = fl;
  l.flag = reinterpret_cast<int*>(fl + BT_CH * a.SD);
  float* wf = fl + BT_CH * a.SD + 1 + wave * a.wflt;
  l.Wt = wf;
  l.arg = reinterpret_cast<int*>(l.Wt + a.S * a.SD);
  return l;
}

__device__ __forceinline__ void bt_load_W(const BtArgs& a, const BtLds& l, int p, int lane) {
  const float* Wp = a.W + (int64_t)p * a.S * a.D;
  for (int e = lane; e < a.S * a.D; e += 64) {
    const int s = e / a.D, d = e - s * a.D;
    l.Wt[s * a.SD + d] = Wp[e];
  }
  bt_wave_sync();
}

__device__ __forceinline__ int bt_length(const BtArgs& a, int64_t b) {
  int64_t L = a.lengths ? a.lengths[b] : a.T;
  L = L < 0 ? 0 : L > a.T ? a.T : L;
  return (int)L;
}
}  // namespace

__global__ __launch_bounds__(256) void backtest_fwd_kernel(BtArgs a) {
  extern __shared__ double bt_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int nw = nthr >> 6, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const BtLds l = bt_carve(a, bt_smem, nw, wave, false);
  const int64_t b = blockIdx.x / (unsigned)a.PT;
  const int p = (int)(blockIdx.x - b * a.PT) * nw + wave;
  const bool live = p < a.P;
  const int pc = live ? p : a.P - 1;   // a dead wave replays the last policy and writes nothing
  bt_load_W(a, l, pc, lane);
  int R = a.reb[pc];
  R = R < 1 ? 1 : R;
  const double c = (double)a.txc[pc];
  const int L = bt_length(a, b);
  if (tid == 0) *l.flag = 0;
  float* wrow = (a.wealth && live) ? a.wealth + (b * a.P + p) * a.T : nullptr;
  BtRes r;
  bt_forward(a, l, b, pc, L, R, c, wrow, tid, nthr, r);
  __syncthreads();
  const bool bad = *l.flag != 0;
  if (!live) return;
  const double NaN = __builtin_nan("");
  if (wrow) {
    // past the chunks of the length: zeros; a failed window: NaN inside the length
    for (int64_t t = (int64_t)cdiv(L, BT_CH) * BT_CH + lane; t < a.T; t += 64) wrow[t] = 0.f;
    if (bad)
      for (int t = lane; t < L; t += 64) wrow[t] = __builtin_nanf("");
  }
  if (lane < 12) {
    double v;
    switch (lane) {
      case 0: v = r.fin; break;
      case 1: v = (double)L; break;
      case 2: v = r.sum; break;
      case 3: v = r.sumsq; break;
      case 4: v = r.nneg; break;
      case 5: v = r.sumneg; break;
      case 6: v = r.sumsqneg; break;
      case 7: v = r.npos; break;
      case 8: v = r.dd; break;
      case 9: v = r.turn; break;
      case 10: v = (double)r.ip; break;
      default: v = (double)r.jt; break;
    }
    a.stats[(b * a.P + p) * 12 + lane] = bad ? NaN : v;
  }
}

__global__ __launch_bounds__(256) void backtest_bwd_kernel(BtArgs a) {
  extern __shared__ double bt_smem[];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int nw = nthr >> 6, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const BtLds l = bt_carve(a, bt_smem, nw, wave, true);
  const int S = a.S, D = a.D, SD = a.SD, E = S * D;
  const int64_t tile = blockIdx.x / (unsigned)a.PT;
  const int p = (int)(blockIdx.x - tile * a.PT) * nw + wave;
  const bool live = p < a.P;
  const int pc = live ? p : a.P - 1;
  bt_load_W(a, l, pc, lane);
  for (int e = lane; e < E; e += 64) l.dW[e] = 0.0;
  int R = a.reb[pc];
  R = R < 1 ? 1 : R;
  const double c = (double)a.txc[pc];
  const int64_t b1 = min(a.B, (tile + 1) * BT_TB);
  for (int64_t b = tile * BT_TB; b < b1; ++b) {
    const int L = bt_length(a, b);
    __syncthreads();   // the previous window's flag has been read
    if (tid == 0) *l.flag = 0;
    BtRes r;
    bt_forward(a, l, b, pc, L, R, c, nullptr, tid, nthr, r);
    __syncthreads();
    const bool bad = *l.flag != 0;
    const double* gs = a.gstats + (b * a.P + pc) * 12;
    const double g_fin = gs[0], g_sum = gs[2], g_sumsq = gs[3], g_sumneg = gs[5], g_sumsqneg = gs[6], g_dd = gs[8],
                 g_turn = gs[9];
    const double VL = bad ? __builtin_nan("") : r.fin;   // a failed window's gradient is NaN, as its statistics
    const double ratio = 1.0 - r.dd;                     // V_{j*} / V_{i*}
    for (int t0 = 0; t0 < L; t0 += BT_CH) {
      __syncthreads();
      bt_stage(a, l, b, t0, L, false, tid, nthr);
      __syncthreads();
      const int t = t0 + lane;
      const bool valid = t < L;
      const BtChunk ch = bt_holdings(a, l, b, t0, min(t0 + BT_CH, L), R, lane);
      double g, tau;
      bool is_reb;
      bt_step(a, l, ch, t, valid, R, lane, g, tau, is_reb);
      const double keep = 1.0 - c * tau;
      const double rho = keep * (1.0 + g) - 1.0;
      const double x = 1.0 + rho;
      double at = g_sum + 2.0 * rho * g_sumsq + g_fin * (VL / x);
      if (rho < 0.0) at += g_sumneg + 2.0 * rho * g_sumsqneg;
      if (r.ip < t && t <= r.jt) at -= g_dd * (ratio / x);
      const bool active = valid && t >= a.lag;
      l.al[lane] = active ? at * keep : 0.0;
      l.u[lane] = is_reb ? g_turn - c * (1.0 + g) * at : 0.0;
      bt_wave_sync();
      // the lanes over the entries of dW; the step's date (k, its tile row, whether it trades) is wave-uniform
      const int nt = min(BT_CH, L - t0);
      const int tt0 = max(0, a.lag - t0);
      const float* pb = a.probs + b * a.T * S;
      for (int e = lane; e < E && tt0 < nt; e += 64) {
        const int s = e / D, d = e - s * D;
        const int rel0 = t0 + tt0 - a.lag;
        int k = rel0 / R, rem = rel0 - k * R;
        // q_k[s] and q_{k-1}[s] (hard: whether s is the date's argmax), loaded once per date
        auto q_of = [&](int kk) -> double {
          if (kk < 0) return 0.0;
          return a.hard ? (l.arg[kk - ch.km1] == s ? 1.0 : 0.0) : (double)pb[(int64_t)kk * R * S + s];
        };
        double q = q_of(k), qp = rem == 0 ? q_of(k - 1) : 0.0;   // off a date qp is set at the next date, before its use
        double acc = 0.0;
        for (int tt = tt0; tt < nt; ++tt) {
          acc = fma(l.al[tt] * q, (double)l.rt[tt * SD + d], acc);
          if (rem == 0) {
            const int j = k - ch.km1;
            const double df = l.H[j * SD + d] - l.H[(j - 1) * SD + d];
            const double sg = df > 0.0 ? 1.0 : df < 0.0 ? -1.0 : 0.0;
            acc = fma(l.u[tt] * sg, q - qp, acc);
          }
          if (++rem == R) {
            rem = 0;
            ++k;
            qp = q;
            if (tt + 1 < nt) q = q_of(k);   // the next step is date k: its row k R = t + 1 - lag lies inside the length
          }
        }
        l.dW[e] += acc;
      }
      bt_wave_sync();
    }
  }
  if (live)
    for (int e = lane; e < E; e += 64) a.part[(tile * a.P + p) * E + e] = l.dW[e];
}

// grad_weights[p, e] = the tiles' partials added in tile order
__global__ __launch_bounds__(256) void backtest_reduce_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                             int64_t ntile, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  for (int64_t k = 0; k < ntile; ++k) acc += part[k * n + i];
  out[i] = acc;
}

bool hmm_backtest_supported(int64_t B, int64_t T, int64_t S, int64_t D, int64_t P) {
  if (S < 1 || S > 32 || D < 1 || D > 64) return false;
  if (T > BT_MAX_T || P > BT_MAX_P) return false;
  return B <= BT_MAX_BLOCKS / (P > 0 ? P : 1);
}

size_t hmm_backtest_bwd_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D, int64_t P) {
  if (B < 0 || T < 0 || P < 0 || !hmm_backtest_supported(B, T, S, D, P)) return 0;
  return (size_t)(cdiv(B, BT_TB) * P * S * D) * sizeof(double);
}

namespace {
// the workgroup's waves and its LDS bytes
int bt_plan(BtArgs& a, bool bwd, size_t& lds) {
  a.SD = bt_odd(a.D);
  a.wdbl = BT_ROWS * a.SD + (bwd ? a.S * a.D + 2 * BT_CH : 0);
  a.wflt = a.S * a.SD + BT_ROWS + 1;
  a.wflt = (a.wflt + 1) & ~1;
  auto bytes = [&](int w) {
    return (size_t)w * a.wdbl * 8 + (size_t)(BT_CH * a.SD + 1 + w * a.wflt) * 4;
  };
  int nw = 4;
  while (nw > 1 && (bytes(nw) > BT_LDS_SOFT || nw >= 2 * a.P)) nw >>= 1;
  lds = (bytes(nw) + 7) & ~(size_t)7;
  a.PT = (int)cdiv(a.P, nw);
  return nw;
}

template <typename K>
void bt_big_lds(K kern) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)BT_LDS_MAX);
}

BtArgs bt_args(const float* returns, const float* probs, const int64_t* lengths, const float* weights,
               const int32_t* rebalance, const float* tx_cost, int64_t lag, int hard, int64_t B, int64_t T, int64_t S,
               int64_t D, int64_t P) {
  BtArgs a = {};
  a.ret = returns; a.probs = probs; a.lengths = lengths; a.W = weights; a.reb = rebalance; a.txc = tx_cost;
  a.B = B; a.T = T; a.S = (int)S; a.D = (int)D; a.P = (int)P;
  a.lag = (int)(lag < BT_MAX_T ? lag : BT_MAX_T);   // T <= 2^28: a longer lag never trades
  a.hard = hard ? 1 : 0;
  return a;
}
}  // namespace

int launch_hmm_backtest(const float* returns, const float* probs, const int64_t* lengths, const float* weights,
                        const int32_t* rebalance, const float* tx_cost, int64_t lag, int hard, int64_t B, int64_t T,
                        int64_t S, int64_t D, int64_t P, double* stats, float* wealth, hipStream_t s) {
  if (!hmm_backtest_supported(B, T, S, D, P)) return VQHMM_EUNSUPPORTED;
  if (B == 0 || P == 0) return VQHMM_OK;
  BtArgs a = bt_args(returns, probs, lengths, weights, rebalance, tx_cost, lag, hard, B, T, S, D, P);
  a.stats = stats;
  a.wealth = T > 0 ? wealth : nullptr;
  size_t lds;
  const int nw = bt_plan(a, false, lds);
  if (lds > BT_LDS_MAX) return VQHMM_EUNSUPPORTED;   // not reached inside the domain
  if (lds > 64 * 1024) {
    static const bool once = (bt_big_lds(backtest_fwd_kernel), true);
    (void)once;
  }
  backtest_fwd_kernel<<<(unsigned)(B * a.PT), nw * 64, lds, s>>>(a);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_backtest_bwd(const float* returns, const float* probs, const int64_t* lengths, const float* weights,
                            const int32_t* rebalance, const float* tx_cost, int64_t lag, int hard, int64_t B,
                            int64_t T, int64_t S, int64_t D, int64_t P, const double* grad_stats,
                            double* grad_weights, void* ws, hipStream_t s) {
  if (!hmm_backtest_supported(B, T, S, D, P)) return VQHMM_EUNSUPPORTED;
  if (P == 0) return VQHMM_OK;
  const int64_t n = P * S * D, ntile = cdiv(B, BT_TB);
  if (ntile > 0) {
    BtArgs a = bt_args(returns, probs, lengths, weights, rebalance, tx_cost, lag, hard, B, T, S, D, P);
    a.gstats = grad_stats;
    a.part = static_cast<double*>(ws);
    size_t lds;
    const int nw = bt_plan(a, true, lds);
    if (lds > BT_LDS_MAX) return VQHMM_EUNSUPPORTED;   // not reached inside the domain
    if (lds > 64 * 1024) {
      static const bool once = (bt_big_lds(backtest_bwd_kernel), true);
      (void)once;
    }
    backtest_bwd_kernel<<<(unsigned)(ntile * a.PT), nw * 64, lds, s>>>(a);
    VQHMM_LAUNCH_CHECK();
  }
  backtest_reduce_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(static_cast<const double*>(ws), grad_weights, ntile,
                                                                 n);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

}  // namespace vqhmm
