// Causal filter and pairwise posteriors of the HMM over the Prior's tables (SURVEY.md §8a rows
// A15 / A16, §8f-1; contracts in include/vqhmm.h, fp64 restatement in tests/hmm_pair_ref.py).
//
//   filt_t(j) = p(z_t = j | x_{1:t}),  loglik = log p(x_{1:L})
//   xi_t(i,j) = p(z_{t-1} = i, z_t = j | x_{1:L})
//             = gamma_t(j) * filt_{t-1}(i) A_t(i,j) / sum_i' filt_{t-1}(i') A_t(i',j)      (1 <= t < L)
//
// The emission e_t(j) and any per-step scale of the forward vector cancel in the column
// normalisation, so xi needs gamma (from launch_fwdbwd, whichever kernel it picks) and one forward
// chain; the forward-backward kernels stay as they are.
//
// Filter.  The chain runs on linear probabilities, normalised at every step:
//   y_t(j) = sum_i x_{t-1}(i) m_t(i,j),   m_t(i,j) = exp(log_A_t(i,j) + em_t(j) - E_t),  E_t = max_j em_t(j)
//   s_t    = sum_i x_{t-1}(i) r_t(i),     r_t(i) = sum_j m_t(i,j)   (= sum_j y_t(j), reduced beside y_t)
//   x_t    = y_t / s_t = filt_t,          loglik = sum_t (E_t + ln s_t)
// m_t and r_t come from the staged tables ahead of the chain, so a step is one multiply, the two
// add-reductions side by side, a reciprocal and a multiply.  ln s_t: the product of up to PF_NORM
// step masses is kept in fp32 (each within [2^-30, 2^30], so the product stays in range), its log2 is
// summed per chunk in fp32 and across chunks in fp64, as is E_t.  A live step whose mass leaves
// [2^-30, 2^30] (underflow to 0, an all -inf column set, overflow, NaN) is redone as a max-shifted
// log-sum-exp step in natural log with its ln s_t added in fp64 (K <= 8: the step's whole chunk, from
// the chunk's start state, so the fast steps stay straight-line code); a sequence whose mass is truly 0
// gets loglik = -inf and keeps x = 0.
//   K <= 8: hmm.hip's lane groups (hmm_lanes.h: G = KP*KP lanes per sequence, the (i,j) map
//     alternating between steps, DPP / permlane reductions), the tables through a two-chunk LDS-DMA ring;
//     the step vectors collect in LDS and leave once per chunk as whole-wave stores.
//   8 < K <= 32: one sequence per wave, hmm_wide.hip's column map (lane = column j and a slice of
//     the reduced axis), tables in registers one chunk ahead, the vector through LDS.
// Addressing: every table read is clamped inside its own sequence's (T, K, K) / (T, K) block
// (stage_chunk; load_cols clamps t to T - 1 and masks i, j >= K), so an exact-size allocation is safe.
//
// xi.  Parallel over (b, t): a workgroup takes NP consecutive positions, whose log_A tiles are one
// contiguous span; the span is staged in LDS with coalesced (16-byte where K % 4 == 0 and the
// pointers allow) loads, one thread per (position, column) forms f(i) exp(a(i,j)) in place and the
// column sum on chip, scales by gamma_t(j) / sum, and the span leaves with coalesced stores.
// Positions t = 0 and t >= L write zeros; a column whose sum is 0 writes zeros.  Every global
// access is guarded by position < B * T.  Bytes per position: K*K read + K*K written + 2 K read.
#include "hmm_lanes.h"
#include "prof.h"

namespace vqhmm {

namespace {

constexpr float PF_LOG2E = 1.44269504088896341f;
constexpr double PF_LN2 = 0.69314718055994531;
constexpr float PF_LO = 0x1p-30f, PF_HI = 0x1p30f;  // a fast step's mass must stay inside
constexpr int PF_NORM = 4;                          // step masses multiplied before one log2
constexpr int PW = 4;                               // wide path: steps per register chunk

__device__ __forceinline__ float pexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float plog2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float pnan() { return __builtin_bit_cast(float, 0x7fc00000u); }

// reductions over the reduced axis i (RED) or the held axis (the step's result index) of parity P
template <int KP, int P, bool RED, typename Op>
__device__ __forceinline__ float axis_red(float v, Op op) {
  // P = 0 (even t): i = g / KP (outer), result index g % KP (inner); P = 1: the other way round
  constexpr bool INNER = RED ? (P == 1) : (P == 0);
  return allred<KP, INNER>(v, op);
}

}  // namespace

// ------------------------------------------------------------------ filter, K <= 8
template <int K, bool W16>
__global__ __launch_bounds__(64) void filter_kernel(const float* __restrict__ log_pi, const float* __restrict__ log_A,
                                                    const float* __restrict__ em,
                                                    const int64_t* __restrict__ lengths, int64_t B, int T,
                                                    float* __restrict__ filt, float* __restrict__ loglik) {
  using Gm = Geo<K, W16>;
  using Rg = Ring<K, W16>;
  constexpr int KP = Gm::KP, G = Gm::G, SPW = Gm::SPW, HC = Gm::HC;
  // ring of two chunks: a chunk of steps takes far longer than a chunk's loads, so one chunk ahead is
  // enough, and the smaller ring lets two waves share a SIMD where the batch is large (K = 8: 19 KB)
  constexpr int R = 2;
  constexpr int RWAIT = Rg::NI * (R - 1);
  constexpr int VB = SPW * HC * KP;  // the chunk's step vectors [SPW][HC][KP]
  constexpr int NF = VB / 64;
  static_assert(VB % 64 == 0 && HC % PF_NORM == 0, "whole-wave flush passes, whole mass groups per chunk");
  // the only LDS object (keeps hipcc's LDS-DMA waits counted): the ring, then the vector buffer
  __shared__ __attribute__((aligned(16))) float lds[R * Gm::SLOT + VB];
  float* ring = lds;
  float* vbuf = lds + R * Gm::SLOT;

  const int lane = threadIdx.x, grp = lane / G, g = lane % G;
  const int64_t b0 = (int64_t)blockIdx.x * SPW;
  const int64_t b = b0 + grp;
  const bool live = b < B;
  const int64_t Lr = live ? lengths[b] : 0;
  const int L = (int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T));
  const int jo = g % KP, ji = g / KP;  // lane's inner / outer coordinate
  int Lmax = L;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o));
  Lmax = __builtin_amdgcn_readfirstlane(Lmax);
  // lengths of the sequences each flush pass of this lane serves (-1: past the batch)
  int Lfl[NF];
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int64_t bq = b0 + (k * 64 + lane) / (HC * KP);
    const int64_t l = bq < B ? lengths[bq] : -1;
    Lfl[k] = (int)(l <= 0 ? l : (l < T ? l : T));
  }

  // rows past the sequence: zeros (the chain below writes rows t < L only)
  if (live) {
    float* F = filt + b * (int64_t)T * K;
    for (int64_t e = (int64_t)L * K + g; e < (int64_t)T * K; e += G) F[e] = 0.f;
  }

  // t = 0 in natural log: x_0 = softmax_j(log_pi + em_0), S = its log-sum-exp (held on the inner axis)
  float x = 0.f;
  double S = 0.0;
  {
    const bool ok = L > 0 && jo < K;
    const float ly = ok ? log_pi[jo] + em[b * (int64_t)T * K + jo] : NEG_INF;
    const float mx = allred<KP, true>(ly, OpMax{});
    const float mz = mx == NEG_INF ? 0.f : mx;
    const float ex = ok ? __expf(ly - mz) : 0.f;
    const float sm = allred<KP, true>(ex, OpAdd{});
    x = mx == NEG_INF ? 0.f : ex / sm;
    S = mx == NEG_INF ? (double)NEG_INF : (double)mz + (double)__logf(sm);
    if (ok && ji == 0) filt[b * (int64_t)T * K + jo] = x;
  }
  wait_vm<0>();  // ordinary loads retired before the LDS-DMA stream starts

  const LaneMap<K, W16> lm(grp, g);
  const int nchunks = (int)cdiv(Lmax, HC);
  if (nchunks > 0) {
#pragma unroll
    for (int c = 0; c < R - 1; ++c)
      stage_chunk<K, W16>(log_A, em, b0, B, T, min(c, nchunks - 1), ring + c * Gm::SLOT, lane);
  }
  float* vrow = vbuf + grp * HC * KP;
  float P = 1.f;  // product of the live step masses since the last log2

  for (int c = 0; c < nchunks; ++c) {
    stage_chunk<K, W16>(log_A, em, b0, B, T, min(c + R - 1, nchunks - 1), ring + ((c + R - 1) % R) * Gm::SLOT,
                        lane);
    wait_vm<RWAIT>();
    const float* sl = ring + (c % R) * Gm::SLOT;
    // the chunk's step tables, read and exponentiated up front, off the chain
    float ml[HC], rl[HC], xe[HC];
#pragma unroll
    for (int s = 0; s < HC; ++s) {
      const int p = s & 1;  // parity of t (HC even)
      const float a = lm.a_ok[p] ? sl[lm.a_off[p] + s * K * K] : NEG_INF;
      const float e = lm.e_ok[p] ? sl[lm.e_off[p] + s * K] : 0.f;
      // the outer map's j = g % KP covers every state along the inner axis
      const float ein = lm.e_ok[0] ? sl[lm.e_off[0] + s * K] : NEG_INF;
      float emx = allred<KP, true>(ein, OpMax{});
      emx = emx == NEG_INF ? 0.f : emx;
      const float m = pexp2((a + (e - emx)) * PF_LOG2E);
      ml[s] = m;
      rl[s] = p == 0 ? axis_red<KP, 0, false>(m, OpAdd{}) : axis_red<KP, 1, false>(m, OpAdd{});
      xe[s] = emx;
    }
    // fast pass: straight-line steps; a live step whose mass leaves the range only raises the flag
    float Ea = 0.f, La = 0.f;  // the chunk's sums of E_t and of log2 of the mass products
    const float x0 = x;        // the chunk's start state, for the rare path
    bool bad = false;
    static_for<HC>([&](auto si) {
      constexpr int s = decltype(si)::value, p = s & 1;
      const int t = c * HC + s;
      if (s == 0 && c == 0) return;  // t = 0 is done
      const bool lv = t < L;
      const float y = axis_red<KP, p, true>(x * ml[s], OpAdd{});
      const float tot = axis_red<KP, p, true>(x * rl[s], OpAdd{});
      bad |= lv && !(tot >= PF_LO && tot <= PF_HI);
      const float xn = y * __builtin_amdgcn_rcpf(tot);
      P = lv ? P * tot : P;
      Ea += lv ? xe[s] : 0.f;
      if constexpr (s % PF_NORM == PF_NORM - 1) {
        La += plog2(P);
        P = 1.f;
      }
      x = lv ? xn : x;
      vrow[s * KP + (p == 0 ? jo : ji)] = xn;  // lanes sharing a state write the same word
    });
    if (__builtin_amdgcn_ballot_w64(bad) == 0) {
      S += (double)Ea + (double)La * PF_LN2;
    } else {
      // wave-uniform rare path: the whole chunk again from its start state, every step in natural
      // log and max-shifted, for every sequence of the wave (the tables are still in the ring slot)
      x = x0;
      P = 1.f;
      auto slow_step = [&](int s, auto pi) {
        constexpr int p = decltype(pi)::value;
        const int t = c * HC + s;
        if (t == 0) return;
        const bool lv = t < L;
        const float a = lm.a_ok[p] ? sl[lm.a_off[p] + s * K * K] : NEG_INF;
        const float e = lm.e_ok[p] ? sl[lm.e_off[p] + s * K] : NEG_INF;
        const float u = __logf(x) + a;
        const float M = axis_red<KP, p, true>(u, OpMax{});
        const float Mz = M == NEG_INF ? 0.f : M;
        const float sm = axis_red<KP, p, true>(u == NEG_INF ? 0.f : __expf(u - Mz), OpAdd{});
        const float ly = M == NEG_INF ? NEG_INF : (Mz + __logf(sm)) + e;
        const float Mt = axis_red<KP, p, false>(ly, OpMax{});
        const float Mtz = Mt == NEG_INF ? 0.f : Mt;
        const float ex = ly == NEG_INF ? 0.f : __expf(ly - Mtz);
        const float st = axis_red<KP, p, false>(ex, OpAdd{});
        const float xn = Mt == NEG_INF ? 0.f : ex / st;
        const double ls = Mt == NEG_INF ? (double)NEG_INF : (double)Mtz + (double)__logf(st);
        S = lv ? S + ls : S;
        x = lv ? xn : x;
        vrow[s * KP + (p == 0 ? jo : ji)] = xn;
      };
#pragma unroll 1
      for (int s = 0; s < HC; s += 2) {
        slow_step(s, std::integral_constant<int, 0>{});
        slow_step(s + 1, std::integral_constant<int, 1>{});
      }
    }
    // flush rows [c HC, c HC + HC) of the wave's sequences, t < L only
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int idx = k * 64 + lane;
      const int q = idx / (HC * KP), r = idx - q * (HC * KP), s = r / KP, j = r - s * KP;
      const int t = c * HC + s;
      if (j < K && t > 0 && t < Lfl[k]) filt[((b0 + q) * (int64_t)T + t) * K + j] = vbuf[idx];
    }
    asm volatile("" ::: "memory");
  }
  if (live && g == 0) loglik[b] = L > 0 ? (float)S : pnan();
}

// ------------------------------------------------------------- filter, 8 < K <= 32
namespace {

// a[s][ii] = A_t(i0 + ii, j), e[s] = em_t(j), t = t0 + s clamped into [0, T) (values past the
// chain's end are unused); i, j >= K masked without a read
template <int IH>
__device__ __forceinline__ void load_cols(const float* __restrict__ A, const float* __restrict__ E, int K, int T,
                                          int t0, int j, int i0, float (&a)[PW][IH], float (&e)[PW]) {
#pragma unroll
  for (int s = 0; s < PW; ++s) {
    const int t = min(t0 + s, T - 1);
    const float* At = A + (int64_t)t * K * K;
#pragma unroll
    for (int ii = 0; ii < IH; ++ii) {
      const int i = i0 + ii;
      a[s][ii] = (j < K && i < K) ? At[i * K + j] : NEG_INF;
    }
    e[s] = j < K ? E[(int64_t)t * K + j] : NEG_INF;
  }
}

template <int NQ>
__device__ __forceinline__ float join_add(float v) {
  if constexpr (NQ == 4) v += xor16(v);
  return v + xor32(v);
}
template <int NQ>
__device__ __forceinline__ float join_max(float v) {
  if constexpr (NQ == 4) v = fmaxf(v, xor16(v));
  return fmaxf(v, xor32(v));
}
template <int COLS>
__device__ __forceinline__ float cols_add(float v) {
#pragma unroll
  for (int o = 1; o < COLS; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
template <int COLS>
__device__ __forceinline__ float cols_max(float v) {
#pragma unroll
  for (int o = 1; o < COLS; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

}  // namespace

template <int IH, int NQ>
__global__ __launch_bounds__(64) void filter_wide_kernel(const float* __restrict__ log_pi,
                                                         const float* __restrict__ log_A,
                                                         const float* __restrict__ em,
                                                         const int64_t* __restrict__ lengths, int K, int T,
                                                         float* __restrict__ filt, float* __restrict__ loglik) {
  __shared__ __attribute__((aligned(16))) float xsh[2][32];  // [parity][state]
  // lane (h, j): column j of COLS = 64 / NQ, reduced-axis slice h of IH entries
  constexpr int COLS = 64 / NQ;
  const int lane = threadIdx.x, j = lane % COLS, h = lane / COLS, i0 = h * IH;
  const int64_t b = blockIdx.x;
  const int64_t Lr = lengths[b];
  const int L = (int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T));
  const float* A = log_A + b * (int64_t)T * K * K;
  const float* E = em + b * (int64_t)T * K;
  float* F = filt + b * (int64_t)T * K;
  for (int64_t e = (int64_t)L * K + lane; e < (int64_t)T * K; e += 64) F[e] = 0.f;
  if (L == 0) {
    if (lane == 0) loglik[b] = pnan();
    return;
  }
  float x;
  double S;
  {
    const float ly = j < K ? log_pi[j] + E[j] : NEG_INF;
    const float mx = cols_max<COLS>(ly);
    const float mz = mx == NEG_INF ? 0.f : mx;
    const float ex = ly == NEG_INF ? 0.f : __expf(ly - mz);
    const float sm = cols_add<COLS>(ex);
    x = mx == NEG_INF ? 0.f : ex / sm;
    S = mx == NEG_INF ? (double)NEG_INF : (double)mz + (double)__logf(sm);
    if (h == 0) {
      xsh[0][j] = x;
      if (j < K) F[j] = x;
    }
  }
  float ca[PW][IH], ce[PW], na[PW][IH], ne[PW];
  if (L > 1) load_cols<IH>(A, E, K, T, 1, j, i0, ca, ce);
  for (int t0 = 1; t0 < L; t0 += PW) {
    if (t0 + PW < L) load_cols<IH>(A, E, K, T, t0 + PW, j, i0, na, ne);
    float P = 1.f, Ea = 0.f;
#pragma unroll
    for (int s = 0; s < PW; ++s) {
      const int t = t0 + s;
      if (t >= L) break;
      float emx = cols_max<COLS>(ce[s]);
      emx = emx == NEG_INF ? 0.f : emx;
      float xv[IH];
#pragma unroll
      for (int q = 0; q < IH / 4; ++q) {
        const float4 f = *reinterpret_cast<const float4*>(&xsh[(t - 1) & 1][i0 + 4 * q]);
        xv[4 * q] = f.x; xv[4 * q + 1] = f.y; xv[4 * q + 2] = f.z; xv[4 * q + 3] = f.w;
      }
      float part = 0.f;
#pragma unroll
      for (int ii = 0; ii < IH; ++ii) part += xv[ii] * pexp2((ca[s][ii] + (ce[s] - emx)) * PF_LOG2E);
      const float y = join_add<NQ>(part);
      const float tot = cols_add<COLS>(y);
      float xn;
      if (__builtin_amdgcn_ballot_w64(!(tot >= PF_LO && tot <= PF_HI)) != 0) {
        // rare path: the step in natural log, max-shifted
        float u[IH], mh = NEG_INF;
#pragma unroll
        for (int ii = 0; ii < IH; ++ii) {
          u[ii] = __logf(xv[ii]) + ca[s][ii];
          mh = fmaxf(mh, u[ii]);
        }
        const float M = join_max<NQ>(mh);
        const float Mz = M == NEG_INF ? 0.f : M;
        float sp = 0.f;
#pragma unroll
        for (int ii = 0; ii < IH; ++ii) sp += u[ii] == NEG_INF ? 0.f : __expf(u[ii] - Mz);
        const float sm = join_add<NQ>(sp);
        const float ly = M == NEG_INF ? NEG_INF : (Mz + __logf(sm)) + ce[s];
        const float Mt = cols_max<COLS>(ly);
        const float Mtz = Mt == NEG_INF ? 0.f : Mt;
        const float ex = ly == NEG_INF ? 0.f : __expf(ly - Mtz);
        const float st = cols_add<COLS>(ex);
        xn = Mt == NEG_INF ? 0.f : ex / st;
        S += Mt == NEG_INF ? (double)NEG_INF : (double)Mtz + (double)__logf(st);
      } else {
        xn = y * __builtin_amdgcn_rcpf(tot);
        P *= tot;
        Ea += emx;
      }
      if (h == 0) {
        xsh[t & 1][j] = xn;
        if (j < K) F[(int64_t)t * K + j] = xn;
      }
    }
    S += (double)Ea + (double)plog2(P) * PF_LN2;
#pragma unroll
    for (int s = 0; s < PW; ++s) {
      ce[s] = ne[s];
#pragma unroll
      for (int ii = 0; ii < IH; ++ii) ca[s][ii] = na[s][ii];
    }
  }
  if (lane == 0) loglik[b] = (float)S;
}

// ------------------------------------------------------------------------------ xi
// LDS: NP tiles at stride TS = K*K + K floats (the pad spreads the positions of a wave over the
// banks), then NP gamma rows and NP filt rows.
constexpr float F32_MAX_PAIR = 3.402823466e38f;
constexpr int XI_THREADS = 256;
constexpr int XI_TILE_FLOATS = 8192;  // 32 KB of tiles per workgroup

static int xi_np(int64_t K) {
  const int64_t np = XI_TILE_FLOATS / (K * K + K);
  return (int)(np >= 64 ? 64 : (np / 4) * 4);
}

template <bool V4>
__global__ __launch_bounds__(XI_THREADS) void xi_kernel(const float* __restrict__ log_A,
                                                        const float* __restrict__ filt,
                                                        const float* __restrict__ gamma,
                                                        const int64_t* __restrict__ lengths, int64_t BT, int T, int K,
                                                        int NP, float* __restrict__ xi) {
  extern __shared__ float4 xi_smem[];
  float* tile = reinterpret_cast<float*>(xi_smem);
  const int KK = K * K, TS = KK + K;
  float* gsh = tile + NP * TS;  // [NP][K] gamma_t
  float* fsh = gsh + NP * K;    // [NP][K] filt_{t-1}
  int* ok = reinterpret_cast<int*>(fsh + NP * K);  // [NP] 1: 1 <= t < L
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * NP;
  const int np = (int)(BT - p0 < NP ? BT - p0 : NP);  // positions of this workgroup (>= 1)

  if (tid < np) {
    const int64_t pos = p0 + tid, bq = pos / T;
    const int t = (int)(pos - bq * T);
    const int64_t l = lengths[bq];
    ok[tid] = t >= 1 && t < l;
  }
  // tiles: one contiguous span of np * KK floats
  const float* src = log_A + p0 * KK;
  if constexpr (V4) {  // KK % 4 == 0, 16-byte aligned base
    const int n4 = np * KK / 4, kq = KK / 4;
    for (int f = tid; f < n4; f += XI_THREADS) {
      const int p = f / kq, r = f - p * kq;
      *reinterpret_cast<float4*>(tile + p * TS + 4 * r) = reinterpret_cast<const float4*>(src)[f];
    }
  } else {
    for (int f = tid; f < np * KK; f += XI_THREADS) {
      const int p = f / KK, r = f - p * KK;
      tile[p * TS + r] = src[f];
    }
  }
  // gamma rows p0 .. p0 + np - 1 and filt rows p0 - 1 .. p0 + np - 2 (row -1 is never used: t = 0)
  for (int f = tid; f < np * K; f += XI_THREADS) {
    gsh[f] = gamma[p0 * K + f];
    const int64_t fo = (p0 - 1) * K + f;
    fsh[f] = fo >= 0 ? filt[fo] : 0.f;
  }
  __syncthreads();
  // one thread per (position, column): v(i) = f(i) exp(a(i,j)) in place, the column sum, the scale
  for (int it = tid; it < np * K; it += XI_THREADS) {
    const int p = it / K, j = it - p * K;
    float* col = tile + p * TS + j;
    if (!ok[p]) {
      for (int i = 0; i < K; ++i) col[i * K] = 0.f;
      continue;
    }
    const float* fr = fsh + p * K;
    // shifted by the column's max (the tables need not be normalised; the shift cancels in v / den)
    float cm = NEG_INF;
    for (int i = 0; i < K; ++i) cm = fmaxf(cm, fr[i] > 0.f ? col[i * K] : NEG_INF);
    cm = (cm == NEG_INF || !(cm <= F32_MAX_PAIR)) ? 0.f : cm;
    float den = 0.f;
    for (int i = 0; i < K; ++i) {
      const float v = fr[i] > 0.f ? fr[i] * __expf(col[i * K] - cm) : 0.f;
      col[i * K] = v;
      den += v;
    }
    const float sc = den > 0.f ? gsh[it] / den : 0.f;
    for (int i = 0; i < K; ++i) col[i * K] = sc > 0.f ? col[i * K] * sc : 0.f;
  }
  __syncthreads();
  float* dst = xi + p0 * KK;
  if constexpr (V4) {
    const int n4 = np * KK / 4, kq = KK / 4;
    for (int f = tid; f < n4; f += XI_THREADS) {
      const int p = f / kq, r = f - p * kq;
      reinterpret_cast<float4*>(dst)[f] = *reinterpret_cast<const float4*>(tile + p * TS + 4 * r);
    }
  } else {
    for (int f = tid; f < np * KK; f += XI_THREADS) {
      const int p = f / KK, r = f - p * KK;
      dst[f] = tile[p * TS + r];
    }
  }
}

// ------------------------------------------------------------------------ launchers
template <int K, bool W16>
static void filter_go(const float* log_pi, const float* log_A, const float* em, const int64_t* lengths, int64_t B,
                      int64_t T, float* filt, float* loglik, hipStream_t s) {
  const dim3 grid((unsigned)cdiv(B, Geo<K, W16>::SPW));
  filter_kernel<K, W16><<<grid, 64, 0, s>>>(log_pi, log_A, em, lengths, B, (int)T, filt, loglik);
}

static bool pair_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool hmm_pair_supported(int64_t K) { return K >= 1 && K <= 32; }

size_t hmm_filter_bytes(int64_t B, int64_t T, int64_t K) { return (size_t)B * T * K * sizeof(float); }

int launch_hmm_filter(const float* log_pi, const float* log_A, const float* em, const int64_t* lengths, int64_t B,
                      int64_t T, int64_t K, float* filt, float* loglik, hipStream_t s) {
  if (B == 0 || T == 0) return VQHMM_OK;
  if (!hmm_pair_supported(K) || T > (1 << 28) || B > INT32_MAX) return VQHMM_EUNSUPPORTED;
  if (K > 16) {
    filter_wide_kernel<16, 2><<<(unsigned)B, 64, 0, s>>>(log_pi, log_A, em, lengths, (int)K, (int)T, filt, loglik);
  } else if (K > 8) {
    filter_wide_kernel<4, 4><<<(unsigned)B, 64, 0, s>>>(log_pi, log_A, em, lengths, (int)K, (int)T, filt, loglik);
  } else {
    const bool w16 = pair_aligned16(log_A) && pair_aligned16(em);
    switch (K) {
      case 1: filter_go<1, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s); break;
      case 2: filter_go<2, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s); break;
      case 3: filter_go<3, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s); break;
      case 4:
        if (w16) filter_go<4, true>(log_pi, log_A, em, lengths, B, T, filt, loglik, s);
        else filter_go<4, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s);
        break;
      case 5: filter_go<5, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s); break;
      case 6: filter_go<6, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s); break;
      case 7: filter_go<7, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s); break;
      default:
        if (w16) filter_go<8, true>(log_pi, log_A, em, lengths, B, T, filt, loglik, s);
        else filter_go<8, false>(log_pi, log_A, em, lengths, B, T, filt, loglik, s);
        break;
    }
  }
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_xi(const float* log_A, const float* filt, const float* gamma, const int64_t* lengths, int64_t B,
                  int64_t T, int64_t K, float* xi, hipStream_t s) {
  if (B == 0 || T == 0) return VQHMM_OK;
  if (!hmm_pair_supported(K) || T > (1 << 28)) return VQHMM_EUNSUPPORTED;
  const int NP = xi_np(K);
  const int64_t BT = B * T;
  const int64_t nblk = cdiv(BT, NP);
  if (nblk > INT32_MAX) return VQHMM_EUNSUPPORTED;
  const size_t lds = ((size_t)NP * (K * K + K) + 2 * (size_t)NP * K + NP) * sizeof(float);
  const bool v4 = K % 4 == 0 && pair_aligned16(log_A) && pair_aligned16(xi);
  if (v4)
    xi_kernel<true><<<(unsigned)nblk, XI_THREADS, lds, s>>>(log_A, filt, gamma, lengths, BT, (int)T, (int)K, NP, xi);
  else
    xi_kernel<false><<<(unsigned)nblk, XI_THREADS, lds, s>>>(log_A, filt, gamma, lengths, BT, (int)T, (int)K, NP, xi);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

}  // namespace vqhmm
