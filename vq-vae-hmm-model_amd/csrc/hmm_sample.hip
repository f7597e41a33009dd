// Regime-path samplers of the time-varying HMM over the Prior's tables (contracts and the draw rule
// in include/vqhmm.h, fp64 restatement in tests/sample_ref.py).
//
//   FFBS        z_{L-1} ~ filt_{L-1},  z_{t-1} | z_t = j  ~  filt_{t-1}(i) exp(log_A_t(i,j) - m_j)   (t = L-1 .. 1)
//   simulation  z_0 ~ exp(log_pi - max),  z_t | z_{t-1} = i  ~  exp(log_A_t(i,j) - m_i)              (t = 1 .. L-1)
//
// The step's tables do not depend on the states drawn, so only the draw is on the serial chain.
// A workgroup serves SPW sequences and up to 64 * NWV samples of each (lane = (sequence, sample)).
// Ahead of the walk it turns CH steps of every sequence into cumulative rows in LDS, one thread per
// (sequence, step, conditioning state): the K weights w, their fp32 running sum c in index order
// (K exponentials per row, once per step and not once per sample), the largest index of a positive
// weight and the total.  Rows are KC + 4 floats (KC = K rounded up to 4, 8, 16 or 32; entries
// i >= K hold +inf), so a walking lane reads the row of its state as 16-byte LDS reads:
//   thr = u * c_{K-1};  draw = #{i : c_i <= thr}  (c is non-decreasing, so this is the smallest i
//   with c_i > thr);  draw = K means none, then the largest i with w_i > 0.
// The rows live in a two-slot ring: the raw tables and the uniforms of chunk c + 1 are loaded into
// registers before chunk c is walked and become rows after it, and the states a walk drew are
// stored one chunk later, so the walk itself waits for LDS only; one barrier per chunk.  A failed draw (total 0 or not finite; an all -inf column makes the
// weights NaN) sets the state to -1, which every later position of that sample inherits.
// Addressing: a read belongs to b < B, sample < N and a step inside [0, L), or is clamped to its array's
// first entries; writes are guarded the same way; 64-bit offsets.
#include <math.h>

#include "kernels.h"

namespace vqhmm {

namespace {

constexpr float SM_INF = __builtin_huge_valf();
constexpr int SM_CH_MAX = 8;          // steps per chunk (the uniforms of a chunk sit in registers)
constexpr int SM_BUF_FLOATS = 4096;   // LDS floats per ring slot
constexpr int SM_WAVES_MAX = 4;

struct SamplePlan {
  int KC, NS, NWV, SPW, CH;
  int64_t nsc, nblk;
  size_t lds;
};

SamplePlan sample_plan(int64_t B, int64_t K, int64_t N) {
  SamplePlan p;
  p.KC = K > 16 ? 32 : K > 8 ? 16 : K > 4 ? 8 : 4;
  p.NS = 64;
  if (N < 64) {
    p.NS = 1;
    while (p.NS < N) p.NS *= 2;
  }
  p.NWV = N > 64 ? (int)(cdiv(N, 64) < SM_WAVES_MAX ? cdiv(N, 64) : SM_WAVES_MAX) : 1;
  const int RS = p.KC + 4;
  const int cap = 64 * p.NWV < SM_BUF_FLOATS / RS ? 64 * p.NWV : SM_BUF_FLOATS / RS;  // rows per chunk
  // N < 64: several sequences share the wave's lanes, as long as a chunk still holds SM_CH_MAX steps
  // (a chunk's walk has to cover the next chunk's loads; shorter chunks cost more than idle lanes)
  p.SPW = 1;
  if (N < 64) {
    const int by_lanes = 64 / p.NS, by_rows = cap / (SM_CH_MAX * (int)K);
    p.SPW = by_lanes < by_rows ? by_lanes : by_rows;
    if (p.SPW < 1) p.SPW = 1;
  }
  p.CH = cap / (p.SPW * (int)K);
  p.CH = p.CH < 1 ? 1 : p.CH > SM_CH_MAX ? SM_CH_MAX : p.CH;
  p.nsc = cdiv(N, (int64_t)p.NS * p.NWV);
  p.nblk = cdiv(B, p.SPW) * p.nsc;
  p.lds = 2 * (size_t)p.SPW * p.CH * K * RS * sizeof(float);
  return p;
}

__device__ __forceinline__ int clamp_len(int64_t l, int T) { return (int)(l <= 0 ? 0 : (l < T ? l : T)); }

}  // namespace

template <int KC, bool FFBS>
__global__ __launch_bounds__(64 * SM_WAVES_MAX) void sample_kernel(
    const float* __restrict__ head /* FFBS: filt (B,T,K); simulation: log_pi (K) */, const float* __restrict__ log_A,
    const int64_t* __restrict__ lengths, const float* __restrict__ u, int64_t B, int T, int K, int64_t N, int NS,
    int SPW, int CH, int nsc, bool row16, int32_t* __restrict__ paths) {
  constexpr int RS = KC + 4;
  extern __shared__ float4 sample_smem[];
  float* ring = reinterpret_cast<float*>(sample_smem);  // [2][SPW * CH * K][RS]
  const int R = SPW * CH * K;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t sg = blockIdx.x / (unsigned)nsc;
  const int64_t sc = blockIdx.x - sg * nsc;
  const int64_t b0 = sg * SPW;

  // the walking lane: sequence q of the workgroup, sample s
  const int q = lane / NS;
  const int64_t s = sc * blockDim.x + (tid - lane) + lane % NS;
  const int64_t bw = b0 + q;
  const bool wlive = q < SPW && bw < B && s < N;
  const int Lw = wlive ? clamp_len(lengths[bw], T) : 0;
  const int64_t base = wlive ? (bw * N + s) * (int64_t)T : 0;
  // the staging thread: row tid = (sequence sq, step srr of the chunk, conditioning state sk)
  const bool srow = tid < R;
  const int sq = tid / (CH * K), srem = tid - sq * (CH * K), srr = srem / K, sk = srem - srr * K;
  const int64_t sb = b0 + sq;
  const int sL = (srow && sb < B) ? clamp_len(lengths[sb], T) : 0;
  int Lmax = 0;
  for (int k = 0; k < SPW; ++k)
    if (b0 + k < B) Lmax = max(Lmax, clamp_len(lengths[b0 + k], T));
  const int nchunks = Lmax > 1 ? (Lmax - 1 + CH - 1) / CH : 0;

  // raw tables of the staging thread's row of chunk c: transition r = c CH + srr of its sequence.
  // Every load is issued whatever the row (a row outside the walk reads the tables' first entries and
  // is dropped), so the loads of a chunk are straight-line code whose count the compiler knows.
  auto load_raw = [&](int c, float (&a)[KC], float (&f)[KC]) {
    const int r = c * CH + srr;
    const bool ok = srow && r < sL - 1;
    const int t = ok ? (FFBS ? sL - 1 - r : 1 + r) : 0;  // ok: 1 <= t <= sL - 1
    const int64_t bt = (ok ? sb : 0) * (int64_t)T;
    const int kk = ok ? sk : 0;
    const float* At = log_A + (bt + t) * K * K;
    if constexpr (!FFBS) {
      if (row16) {  // K % 4 == 0 and a 16-byte aligned table: the row as 16-byte loads
        const float4* Ar = reinterpret_cast<const float4*>(At + kk * K);
#pragma unroll
        for (int v = 0; v < KC / 4; ++v) {
          const float4 q4 = Ar[4 * v < K ? v : 0];
          a[4 * v] = q4.x; a[4 * v + 1] = q4.y; a[4 * v + 2] = q4.z; a[4 * v + 3] = q4.w;
        }
        return;
      }
    }
    const float* Ft = head + (bt + (ok ? t - 1 : 0)) * K;  // FFBS only: filt_{t-1}
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      const int ic = i < K ? i : 0;
      a[i] = FFBS ? At[ic * K + kk] : At[kk * K + ic];
      if constexpr (FFBS) f[i] = Ft[ic];
    }
  };
  auto store_row = [&](int c, const float (&a)[KC], const float (&f)[KC]) {
    const int r = c * CH + srr;
    if (!(srow && r < sL - 1)) return;
    float m = -SM_INF;
#pragma unroll
    for (int i = 0; i < KC; ++i)
      if (i < K) m = fmaxf(m, a[i]);
    float row[RS];
    float run = 0.f;
    int last = -1;
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      if (i < K) {
        const float e = expf(a[i] - m);
        const float w = FFBS ? f[i] * e : e;
        run += w;
        last = w > 0.f ? i : last;
        row[i] = run;
      } else {
        row[i] = SM_INF;
      }
    }
    row[KC] = __int_as_float(last);
    row[KC + 1] = run;
    row[KC + 2] = 0.f;
    row[KC + 3] = 0.f;
    float4* dst = reinterpret_cast<float4*>(ring + ((size_t)(c & 1) * R + tid) * RS);
#pragma unroll
    for (int v = 0; v < RS / 4; ++v) dst[v] = make_float4(row[4 * v], row[4 * v + 1], row[4 * v + 2], row[4 * v + 3]);
  };
  // position that transition r of the walking lane's sequence draws
  auto draw_pos = [&](int r) { return FFBS ? Lw - 2 - r : 1 + r; };
  auto load_u = [&](int c, float (&uu)[SM_CH_MAX]) {
#pragma unroll
    for (int rr = 0; rr < SM_CH_MAX; ++rr) {
      const int r = c * CH + rr;
      uu[rr] = u[(rr < CH && wlive && r < Lw - 1) ? base + draw_pos(r) : 0];
    }
  };
  // the states a chunk's walk drew leave one chunk later, ahead of the next loads: the walk itself
  // then issues no global access and waits for none
  auto flush = [&](int c, const int (&zs)[SM_CH_MAX]) {
#pragma unroll
    for (int rr = 0; rr < SM_CH_MAX; ++rr) {
      const int r = c * CH + rr;
      if (rr < CH && wlive && r < Lw - 1) paths[base + draw_pos(r)] = zs[rr];
    }
  };

  // positions past the length, and the walk's first draw straight from global memory
  int z = -1;
  if (wlive) {
    for (int t = Lw; t < T; ++t) paths[base + t] = -1;
    if (Lw > 0) {
      const int t0 = FFBS ? Lw - 1 : 0;
      const float* hp = FFBS ? head + (bw * (int64_t)T + t0) * K : head;
      float m = -SM_INF;
      if constexpr (!FFBS)
        for (int i = 0; i < K; ++i) m = fmaxf(m, hp[i]);
      auto weight = [&](int i) { return FFBS ? hp[i] : expf(hp[i] - m); };
      float tot = 0.f;
      for (int i = 0; i < K; ++i) tot += weight(i);
      const float thr = u[base + t0] * tot;
      float run = 0.f;
      int cnt = 0, last = -1;
      for (int i = 0; i < K; ++i) {
        const float w = weight(i);
        run += w;
        cnt += run <= thr ? 1 : 0;
        last = w > 0.f ? i : last;
      }
      const int pick = cnt < K ? cnt : last;
      z = (tot > 0.f && tot < SM_INF && pick >= 0) ? pick : -1;
      paths[base + t0] = z;
    }
  }

  float a[KC], f[KC], un[SM_CH_MAX], uc[SM_CH_MAX];
  int zs[SM_CH_MAX];
#pragma unroll
  for (int rr = 0; rr < SM_CH_MAX; ++rr) zs[rr] = -1;
  if (nchunks > 0) {
    load_u(0, un);
    load_raw(0, a, f);  // last, so that waiting for it at the loop's top covers the uniforms too
  }
  for (int c = 0; c < nchunks; ++c) {
    store_row(c, a, f);
#pragma unroll
    for (int rr = 0; rr < SM_CH_MAX; ++rr) uc[rr] = un[rr];
    __syncthreads();
    if (c > 0) flush(c - 1, zs);
    if (c + 1 < nchunks) {
      load_u(c + 1, un);
      load_raw(c + 1, a, f);
    }
    const float* slot = ring + (size_t)(c & 1) * R * RS;
#pragma unroll
    for (int rr = 0; rr < SM_CH_MAX; ++rr) {
      const int r = c * CH + rr;
      if (rr < CH && wlive && r < Lw - 1) {
        const float4* row = reinterpret_cast<const float4*>(slot + ((size_t)(q * CH + rr) * K + max(z, 0)) * RS);
        const float4 tail = row[KC / 4];
        const float tot = tail.y;
        const int last = __float_as_int(tail.x);
        const float thr = uc[rr] * tot;
        int cnt = 0;
#pragma unroll
        for (int v = 0; v < KC / 4; ++v) {
          const float4 cv = row[v];
          cnt += (cv.x <= thr ? 1 : 0) + (cv.y <= thr ? 1 : 0) + (cv.z <= thr ? 1 : 0) + (cv.w <= thr ? 1 : 0);
        }
        const int pick = cnt < K ? cnt : last;
        z = (z >= 0 && tot > 0.f && tot < SM_INF && pick >= 0) ? pick : -1;
        zs[rr] = z;
      }
    }
  }
  if (nchunks > 0) flush(nchunks - 1, zs);
}

template <bool FFBS>
static int sample_go(const float* head, const float* log_A, const int64_t* lengths, const float* u, int64_t B,
                     int64_t T, int64_t K, int64_t N, int32_t* paths, hipStream_t s) {
  if (K < 1 || K > 32 || T > (1 << 28) || B > INT32_MAX) return VQHMM_EUNSUPPORTED;
  const SamplePlan p = sample_plan(B, K, N);
  if (p.nblk > INT32_MAX || p.nsc > INT32_MAX) return VQHMM_EUNSUPPORTED;
  const dim3 grid((unsigned)p.nblk), block(64 * p.NWV);
  const bool row16 = K % 4 == 0 && (reinterpret_cast<uintptr_t>(log_A) & 15) == 0;
#define SM_LAUNCH(KCV)                                                                                              \
  sample_kernel<KCV, FFBS><<<grid, block, p.lds, s>>>(head, log_A, lengths, u, B, (int)T, (int)K, N, p.NS, p.SPW, \
                                                      p.CH, (int)p.nsc, row16, paths)
  switch (p.KC) {
    case 4: SM_LAUNCH(4); break;
    case 8: SM_LAUNCH(8); break;
    case 16: SM_LAUNCH(16); break;
    default: SM_LAUNCH(32); break;
  }
#undef SM_LAUNCH
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_ffbs_sample(const float* filt, const float* log_A, const int64_t* lengths, const float* u, int64_t B,
                           int64_t T, int64_t K, int64_t N, int32_t* paths, hipStream_t s) {
  return sample_go<true>(filt, log_A, lengths, u, B, T, K, N, paths, s);
}

int launch_hmm_markov_sample(const float* log_pi, const float* log_A, const int64_t* lengths, const float* u,
                             int64_t B, int64_t T, int64_t K, int64_t N, int32_t* paths, hipStream_t s) {
  return sample_go<false>(log_pi, log_A, lengths, u, B, T, K, N, paths, s);
}

}  // namespace vqhmm
