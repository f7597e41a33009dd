// Stationary HMM with full-covariance Gaussian emissions on continuous observations: the emission log-densities,
// the fused Baum-Welch E-step with the S x D x D second moments, and the same moments under a caller-supplied
// gamma (contracts in include/vqhmm.h, fp64 restatement in tests/gauss_full_ref.py; DESIGN.md "Full covariances").
//
//   model   log_pi (S), log_A (S,S) rows = from-state, mean (S,D), prec_chol (S,D,D) = W_s = L_s^-1 (Sigma_s = L_s
//           L_s^T), row-major, lower-triangular, positive diagonal; the strict upper triangle is never read
//   data    x (B,T,D), lengths (B), shift (D) (nullable): every moment is taken of y = x - shift
//   E-step  pi_cnt, trans_cnt, occ, m1 = sum gamma_t(s) y_t as in hmm_gauss.hip, m2 (S,D,D) = sum gamma_t(s) y_t
//           y_t^T (fp64, one triangle computed and mirrored), loglik (B), gamma (B,T,S) (optional)
//
// This file follows hmm_gauss.hip: the chain, the x staging, the slabs and the reduction are that file's, and its
// few small helpers are restated here (gf_*) rather than shared.
//
// Emissions.  em[t,s] = -1/2 |W_s (x - mu_s)|^2 + c_s, c_s = sum_i log W_s[i,i] - (D/2) ln 2 pi (summed in fp64,
// rounded once).  Every workgroup builds (W packed by rows: row i at i (i + 1) / 2, mu, c) in LDS with gf_table
// and evaluates gf_em, the one function that holds the arithmetic, with lane = time step on a chunk of 64 rows of
// x staged in LDS: z = x - mu_s goes to registers once per (row, state), the D (D + 1) / 2 products are fmaf
// chains along the rows of W (wave-uniform LDS broadcasts), the squares are summed in row order.  The loops are
// unrolled for D <= 8, 16 or 32 (the same fmaf order in each), and the file is built without contraction, so the
// E-step's internal emissions are the bits the emission entry writes.
//
// Second moments.  Pooled form: the chunk's gamma^T (S x 64) . Z (64 x P), P = D (D + 1) / 2, Z[r, (i,j)] = y_i y_j
// for j <= i, on v_mfma_f32_16x16x4_f32 in tiles of 16 states x 16 pairs (gf_chunk_moments, shared by the E-step and
// the moments entry); the pair of a column comes from a P-entry LDS table.  Each tile's fp32 sums are added with
// the sequence's weight in one fp64 fma to the wave's private LDS slab [m1 S D | m2 S P]; workgroups sum their
// waves' slabs in wave order, and the reduce launch sums the partials in a fixed order and writes both triangles
// of m2 from the one sum: no atomics, the same bits run to run, m2[s,i,j] == m2[s,j,i] bit for bit.
//
// Moments entry.  gamma is given, so there is no chain: a flag launch marks the sequences with a non-finite x or
// gamma inside their length (plain stores of 1 into a zeroed array), then one wave per (sequence, 64-step chunk)
// stages x and gamma, adds the chunk's products to its slab, and the same reduce launch finishes.
//
// Members.  As in hmm_gauss.hip: blockIdx.y of the E-step and of the reduce kernel is the member of a stack of M
// models that share x, lengths and shift (the batched entry; the single-model entry is M = 1).  A member has its own
// parameter slices, weights row, alpha rows, partials (`mstride` workspace bytes apart) and output blocks and runs
// the single model's plan, so its bits are the single-model call's.  The moments entry has no member axis.
//
// Addressing.  x and gamma are read only at rows t < L of the wave's own sequence, parameters only at (s, i, j <=
// i), the workspace only inside the sequence's own rows.
//
// Decode and filter.  hmm_gauss_decode_dev.h's kernels, instantiated at the end of this file on GaussFullEm
// (gf_table, gf_stage_x, gf_chunk_em, gf_em).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // the header's table prologue is not used here
#include "hmm_code_dev.h"  // the lane helpers and the fast step's range
#pragma clang diagnostic pop

namespace vqhmm {

namespace {

constexpr int GF_MAX_NW = 4;                   // waves (private slabs) per workgroup, at most
constexpr size_t GF_LDS_SOFT = 64 * 1024;      // the emission entry's workgroups stay under this
constexpr size_t GF_LDS_CU = 160 * 1024;       // a CU's LDS
constexpr size_t GF_LDS_MAX = 156 * 1024;      // of the CU's 160 KB
constexpr int64_t GF_MAX_WAVES = 2048;         // waves of the grid (partials: one per workgroup)
constexpr int64_t GF_MAX_SDD = 8192;           // S D D, at most
constexpr double GF_LN2PI = 1.8378770664093454836;
typedef float gf_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool gf_nonfinite(float v) {
  return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u;
}
__host__ __device__ __forceinline__ int gf_odd(int v) { return v | 1; }
__host__ __device__ __forceinline__ int gf_tri(int D) { return D * (D + 1) / 2; }

// pij[p] = i | j << 8 for the p-th pair (i, j <= i) in row order, by every thread of the workgroup
__device__ __forceinline__ void gf_pairs(int D, uint32_t* pij, int tid, int nthr) {
  for (int p = tid; p < gf_tri(D); p += nthr) {
    int i = 0;
    while (gf_tri(i + 1) <= p) ++i;
    pij[p] = (uint32_t)i | (uint32_t)(p - gf_tri(i)) << 8;
  }
}

// (W packed, mu, c) in LDS, by every thread of the workgroup; the caller synchronises
__device__ __forceinline__ void gf_table(const float* __restrict__ mean, const float* __restrict__ prec, int S, int D,
                                         float* Wl, float* mu, float* cs, int tid, int nthr) {
  const int P = gf_tri(D);
  for (int k = tid; k < S * D; k += nthr) mu[k] = mean[k];
  for (int k = tid; k < S * D * D; k += nthr) {
    const int s = k / (D * D), r = k - s * D * D;
    const int i = r / D, j = r - i * D;
    if (j <= i) Wl[s * P + gf_tri(i) + j] = prec[k];
  }
  for (int s = tid; s < S; s += nthr) {
    double acc = 0.0;
    for (int i = 0; i < D; ++i) acc += log((double)prec[(s * D + i) * D + i]);
    cs[s] = (float)(acc - 0.5 * (double)D * GF_LN2PI);
  }
}

// the emission log-density of one row of x under one state: the only place this arithmetic is written.  W = the
// state's packed rows; DP >= D bounds the unrolled loops
template <int DP>
__device__ __forceinline__ float gf_em_dp(const float* xr, const float* mu, const float* W, float c, int D) {
  float z[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) z[j] = j < D ? xr[j] - mu[j] : 0.f;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    if (i < D) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j <= i; ++j) acc = fmaf(W[i * (i + 1) / 2 + j], z[j], acc);
      q = fmaf(acc, acc, q);
    }
  }
  return fmaf(-0.5f, q, c);
}
__device__ __forceinline__ float gf_em(const float* xr, const float* mu, const float* W, float c, int D) {
  if (D <= 8) return gf_em_dp<8>(xr, mu, W, c, D);
  if (D <= 16) return gf_em_dp<16>(xr, mu, W, c, D);
  return gf_em_dp<32>(xr, mu, W, c, D);
}

// rows [0, n) of a sequence's x (xg = its row t0, n D contiguous floats) into xbuf with row stride DS;
// -> whether any of them is not finite (wave-uniform)
__device__ __forceinline__ bool gf_stage_x(const float* __restrict__ xg, int n, int D, int DS, int lane,
                                           float* xbuf) {
  const int q = 64 / D, rm = 64 - q * D;
  int r = lane / D, c = lane - r * D;
  bool bad = false;
  for (int k = lane; k < n * D; k += 64) {
    const float v = xg[k];
    xbuf[r * DS + c] = v;
    bad |= gf_nonfinite(v);
    r += q;
    c += rm;
    if (c >= D) {
      c -= D;
      ++r;
    }
  }
  return __builtin_amdgcn_ballot_w64(bad) != 0;
}

// lane = row: em[lane, s] for s < S into ebuf (row stride ES) -> the row's maximum (0 for lanes >= n) and
// whether any emission of a row < n is not finite (wave-uniform)
__device__ __forceinline__ bool gf_chunk_em(const float* xbuf, int DS, const float* mu, const float* Wl,
                                            const float* cs, int S, int D, int n, int lane, float* ebuf, int ES,
                                            float& Mv) {
  const int P = gf_tri(D);
  float M = CE_NEG_INF;
  bool bad = false;
  if (lane < n) {
    for (int s = 0; s < S; ++s) {
      const float em = gf_em(xbuf + lane * DS, mu + s * D, Wl + s * P, cs[s], D);
      ebuf[lane * ES + s] = em;
      M = fmaxf(M, em);
      bad |= gf_nonfinite(em);
    }
  }
  Mv = lane < n ? M : 0.f;
  return __builtin_amdgcn_ballot_w64(bad) != 0;
}

// the moment sums of rows [0, n) of a staged chunk into the wave's slab [m1 S D | m2 S P], each with weight wt in
// one fp64 fma: gamma^T (S x n) . [y | Z] (n x (D + P)), y = x - shift, Z[r, p] = y_i y_j for pij[p] = (i, j), on
// v_mfma_f32_16x16x4_f32 in tiles of 16 states x 16 columns.  g = the chunk's gamma rows (row stride S).  Operand
// lanes: A[row = lane & 15][k = lane >> 4] = gamma[r = 4 kk + k][s = row], B[k][col = lane & 15] = the column's
// value at row r; result register i of a lane is C[row = 4 (lane >> 4) + i][col = lane & 15].  Rows past n and
// columns past S / D / P enter as zeros.
__device__ __forceinline__ void gf_chunk_moments(const float* xbuf, int DS, const float* g, const float* shl,
                                                 const uint32_t* pij, int S, int D, int n, int lane, double wt,
                                                 double* slab) {
  const int P = gf_tri(D), SD = S * D;
  const int kq = lane >> 4, l15 = lane & 15, nk = (n + 3) >> 2;
  for (int mt = 0; mt * 16 < S; ++mt) {
    const int sa = mt * 16 + l15;
    const bool sok = sa < S;
    for (int nt = 0; nt * 16 < D + P; ++nt) {
      // columns [0, D) are y, columns [D, D + P) the pairs; a tile may hold both
      const int col = nt * 16 + l15;
      const bool cok = col < D + P;
      int ci = 0, cj = -1;
      if (cok) {
        if (col < D) {
          ci = col;
        } else {
          const uint32_t ij = pij[col - D];
          ci = (int)(ij & 0xffu);
          cj = (int)(ij >> 8);
        }
      }
      const float shi = shl[ci], shj = cj >= 0 ? shl[cj] : 0.f;
      gf_f4 c = gf_f4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < nk; ++kk) {
        const int r = 4 * kk + kq;
        const bool rok = r < n;
        float bv = 0.f;
        if (rok && cok) {
          bv = xbuf[r * DS + ci] - shi;
          if (cj >= 0) bv *= xbuf[r * DS + cj] - shj;
        }
        const float gq = (rok && sok) ? g[r * S + sa] : 0.f;
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(gq, bv, c, 0, 0, 0);
      }
      if (cok) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int s = mt * 16 + kq * 4 + i;
          if (s < S) {
            double* bp = col < D ? slab + (s * D + col) : slab + (SD + s * P + (col - D));
            *bp = fma(wt, (double)c[i], *bp);
          }
        }
      }
    }
  }
}

struct GaussFullArgs {
  const float* log_pi;
  const float* log_A;
  const float* mean;
  const float* prec;
  const float* x;
  const int64_t* lengths;
  const float* shift;    // (D), nullable (= 0)
  const float* weights;  // (M, B), nullable (= all 1)
  int64_t B;
  int T, S, D;
  float* alpha;   // (B, T, S) scaled forward vectors
  double* part;   // [gridDim.x][m1 S*D | m2 S*P | trans S*S | pi S | occ S]
  float* loglik;  // nullable
  float* gamma;   // nullable
  size_t mstride;  // bytes from a member's alpha / part to the next member's
};

// member m's view of the arguments (m = 0 changes nothing): x, lengths and shift are shared
__device__ __forceinline__ GaussFullArgs gauss_full_member(GaussFullArgs a, int64_t m) {
  a.log_pi += m * a.S;
  a.log_A += m * a.S * a.S;
  a.mean += m * a.S * a.D;
  a.prec += m * a.S * a.D * a.D;
  if (a.weights) a.weights += m * a.B;
  a.alpha = reinterpret_cast<float*>(reinterpret_cast<char*>(a.alpha) + m * a.mstride);
  a.part = reinterpret_cast<double*>(reinterpret_cast<char*>(a.part) + m * a.mstride);
  if (a.loglik) a.loglik += m * a.B;
  if (a.gamma) a.gamma += m * a.B * (int64_t)a.T * a.S;
  return a;
}

// ------------------------------------------------------------------------------ emission entry
// one chunk of 64 rows per wave; LDS: [W S*P][mu S*D][c S] [per wave: xbuf 64*DS, obuf 64*OS]
__global__ __launch_bounds__(256) void gauss_full_emission_kernel(const float* __restrict__ mean,
                                                                  const float* __restrict__ prec,
                                                                  const float* __restrict__ x,
                                                                  const int64_t* __restrict__ lengths, int64_t B,
                                                                  int T, int S, int D, float* __restrict__ em) {
  extern __shared__ float gf_smem_f[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int DS = gf_odd(D), OS = gf_odd(S), P = gf_tri(D);
  float* Wl = gf_smem_f;
  float* mu = Wl + S * P;
  float* cs = mu + S * D;
  float* xbuf = cs + S + wave * (CE_CH * (DS + OS));
  float* obuf = xbuf + CE_CH * DS;
  gf_table(mean, prec, S, D, Wl, mu, cs, tid, (int)blockDim.x);
  __syncthreads();
  const int64_t nch = cdiv(T, CE_CH);
  const int64_t w = (int64_t)blockIdx.x * nw + wave;
  if (w >= B * nch) return;
  const int64_t b = w / nch;
  const int t0 = (int)(w - b * nch) * CE_CH;
  const int64_t Lr = lengths[b];
  const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
  const int rows = min(CE_CH, T - t0);
  const int n = max(0, min(CE_CH, L - t0));
  if (n > 0) {
    gf_stage_x(x + (b * T + t0) * (int64_t)D, n, D, DS, lane, xbuf);
    asm volatile("" ::: "memory");
    float Mv;
    gf_chunk_em(xbuf, DS, mu, Wl, cs, S, D, n, lane, obuf, OS, Mv);
    asm volatile("" ::: "memory");
  }
  float* out = em + (b * T + t0) * (int64_t)S;
  const int q = 64 / S, rm = 64 - q * S;
  int r = lane / S, c = lane - r * S;
  for (int k = lane; k < rows * S; k += 64) {
    out[k] = r < n ? obuf[r * OS + c] : CE_NEG_INF;
    r += q;
    c += rm;
    if (c >= S) {
      c -= S;
      ++r;
    }
  }
}

// -------------------------------------------------------------------------------------- reduce
// out = sum over the partials in a fixed order (gauss_reduce_kernel's scheme): 16 elements per workgroup, thread
// (py, kx) adds partials py, py + 16, .. of element kx in index order, then the 16 sums are added in py order.  An
// m2 sum is written to both triangles.  pi_cnt == nullptr (the moments entry): trans and pi are neither read nor
// written.  blockIdx.y is the member: its own partials (mstride bytes apart) and output blocks
constexpr int GF_RK = 16, GF_RP = 16;
__global__ __launch_bounds__(GF_RK* GF_RP) void gauss_full_reduce_kernel(const double* __restrict__ part,
                                                                         size_t mstride, int np, int S, int D,
                                                                         double* __restrict__ pi_cnt,
                                                                         double* __restrict__ trans_cnt,
                                                                         double* __restrict__ occ,
                                                                         double* __restrict__ m1,
                                                                         double* __restrict__ m2) {
  __shared__ double red[GF_RP][GF_RK];
  const int P = gf_tri(D), SD = S * D, SP2 = S * P, SS = S * S, NE = SD + SP2 + SS + 2 * S;
  const int kx = threadIdx.x % GF_RK, py = threadIdx.x / GF_RK;
  const int k = (int)blockIdx.x * GF_RK + kx;
  const int64_t mem = blockIdx.y;
  part = reinterpret_cast<const double*>(reinterpret_cast<const char*>(part) + mem * mstride);
  if (pi_cnt != nullptr) {
    pi_cnt += mem * S;
    trans_cnt += mem * SS;
  }
  occ += mem * S;
  m1 += mem * SD;
  m2 += mem * (int64_t)SD * D;
  const bool chain_cnt = k >= SD + SP2 && k < SD + SP2 + SS + S;
  const bool live = k < NE && !(chain_cnt && pi_cnt == nullptr);
  double acc = 0.0;
  if (live) {
#pragma unroll 4
    for (int p = py; p < np; p += GF_RP) acc += part[(int64_t)p * NE + k];
  }
  red[py][kx] = acc;
  __syncthreads();
  if (py != 0 || !live) return;
  acc = 0.0;
#pragma unroll
  for (int q = 0; q < GF_RP; ++q) acc += red[q][kx];
  if (k < SD) {
    m1[k] = acc;
  } else if (k < SD + SP2) {
    const int e = k - SD, s = e / P, p = e - s * P;
    int i = 0;
    while (gf_tri(i + 1) <= p) ++i;
    const int j = p - gf_tri(i);
    m2[(s * D + i) * D + j] = acc;
    m2[(s * D + j) * D + i] = acc;
  } else if (k < SD + SP2 + SS) {
    trans_cnt[k - SD - SP2] = acc;
  } else if (k < SD + SP2 + SS + S) {
    pi_cnt[k - SD - SP2 - SS] = acc;
  } else {
    occ[k - SD - SP2 - SS - S] = acc;
  }
}

// -------------------------------------------------------------------------------------- E-step
// all-ones weights give the bits of weights = NULL: fma(1.0, v, acc) is the plain fp64 add.  MEM: the launch has
// more than one member (blockIdx.y); with one the arguments stay kernel arguments, as in hmm_code.hip
template <int SP, bool MEM>
__global__ __launch_bounds__(256) void gauss_full_estep_kernel(const GaussFullArgs a0) {
  extern __shared__ double gf_smem[];
  const GaussFullArgs a = MEM ? gauss_full_member(a0, blockIdx.y) : a0;
  constexpr int ES = SP | 1;  // row stride of the chunk's emission buffer (odd: the lane = time pass is conflict-free)
  const int S = a.S, D = a.D, T = a.T;
  const int P = gf_tri(D), SD = S * D, SL = SD + S * P, NT = S * S + 2 * S, DS = gf_odd(D);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int j = lane, jj = j & (SP - 1);
  const bool act = j < S;
  // LDS: [slab nw x SL doubles] [W S*P][mu SD][c S][shift D][pij P] (an even count of words)
  //      [per wave: xbuf 64 DS | ebuf 64 ES | abuf 65 S floats, an even count]; when the wave has run out of
  //      sequences its staging buffers hold its NT transition / pi / occ doubles for the workgroup's sum
  double* slab = gf_smem + (size_t)wave * SL;
  float* Wl = reinterpret_cast<float*>(gf_smem + (size_t)nw * SL);
  float* mu = Wl + S * P;
  float* cs = mu + SD;
  float* shl = cs + S;
  uint32_t* pij = reinterpret_cast<uint32_t*>(shl + D);
  const int wfl = (CE_CH * (DS + ES) + (CE_CH + 1) * S + 1) & ~1;  // floats of a wave's staging buffers (>= 2 NT)
  float* wave0 = Wl + ((S * P + SD + S + D + P + 1) & ~1);
  float* xbuf = wave0 + wave * wfl;
  float* ebuf = xbuf + CE_CH * DS;
  float* abuf = ebuf + CE_CH * ES;
  gf_table(a.mean, a.prec, S, D, Wl, mu, cs, tid, (int)blockDim.x);
  gf_pairs(D, pij, tid, (int)blockDim.x);
  for (int k = tid; k < D; k += blockDim.x) shl[k] = a.shift ? a.shift[k] : 0.f;
  for (int k = tid; k < nw * SL; k += blockDim.x) gf_smem[k] = 0.0;
  __syncthreads();

  double tc64[SP];
#pragma unroll
  for (int q = 0; q < SP; ++q) tc64[q] = 0.0;
  double pc64 = 0.0, oc64 = 0.0;

  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < a.B; b += (int64_t)gridDim.x * nw) {
    const int64_t Lr = a.lengths[b];
    const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
    const float* xs = a.x + b * (int64_t)T * D;
    float* al = a.alpha + b * (int64_t)T * S;
    float* gm_out = a.gamma ? a.gamma + b * (int64_t)T * S : nullptr;
    if (gm_out)
      for (int64_t e = (int64_t)L * S + lane; e < (int64_t)T * S; e += 64) gm_out[e] = 0.f;
    if (L == 0) {
      if (a.loglik && lane == 0) a.loglik[b] = ce_nan();
      continue;
    }

    // the chunk at t0: x to LDS, then e_t = exp(em_t - max_s em_t) for its n rows (zeros in the columns
    // [S, SP) and the rows past n), Mv = the lane's row maximum -> false if x or an emission is not finite
    auto stage = [&](int t0, int n, float& Mv) {
      asm volatile("" ::: "memory");
      const bool badx = gf_stage_x(xs + (int64_t)t0 * D, n, D, DS, lane, xbuf);
      asm volatile("" ::: "memory");
      const bool bade = gf_chunk_em(xbuf, DS, mu, Wl, cs, S, D, n, lane, ebuf, ES, Mv);
      for (int s = 0; s < SP; ++s) {
        const float v = (lane < n && s < S) ? expf(ebuf[lane * ES + s] - Mv) : 0.f;
        ebuf[lane * ES + s] = v;
      }
      asm volatile("" ::: "memory");
      return !(badx || bade);
    };
    // ln e_t(j) of row s of the staged chunk, for the lane's state (the rare paths)
    auto log_e = [&](int s, float Mv) {
      return act ? gf_em(xbuf + s * DS, mu + j * D, Wl + j * P, cs[j], D) - ce_lane(Mv, s) : CE_NEG_INF;
    };

    // ------------------------------------------------------------------ forward
    float xf = 0.f;
    double Sll = 0.0;
    int status = 0;  // 1: impossible (mass 0), 2: a non-finite x or emission inside the length
    {
      float Acol[SP];
#pragma unroll
      for (int i = 0; i < SP; ++i) Acol[i] = (act && i < S) ? __expf(a.log_A[i * S + j]) : 0.f;
      const float pij0 = act ? __expf(a.log_pi[j]) : 0.f;
      float Pm = 1.f, Dr = 0.f;
      for (int t0 = 0; t0 < L && status == 0; t0 += CE_CH) {
        const int n = min(CE_CH, L - t0);
        float Mv;
        if (!stage(t0, n, Mv)) {
          status = 2;
          break;
        }
        float e_nx = ebuf[jj];
        for (int s = 0; s < n; ++s) {
          const int t = t0 + s;
          const float e = e_nx;
          e_nx = ebuf[min(s + 1, CE_CH - 1) * ES + jj];  // one step ahead of the chain
          Sll += (double)ce_lane(Mv, s);
          float u;
          if (t == 0) {
            u = pij0;
          } else {
            float u0 = 0.f, u1 = 0.f;
#pragma unroll
            for (int i = 0; i < SP; i += 2) {
              u0 = fmaf(Acol[i], ce_lane(xf, i), u0);
              if (i + 1 < SP) u1 = fmaf(Acol[i + 1], ce_lane(xf, i + 1), u1);
            }
            u = u0 + u1;
          }
          const float y = act ? u * e : 0.f;
          const float c = ce_red<SP>(y, CeAdd{});
          const float cu = ce_uni(c);
          if (cu >= CE_LO && cu <= CE_HI) {
            const float r = __builtin_amdgcn_rcpf(c);
            xf = y * r;
            Pm *= c;
            Dr += fmaf(r, c, -1.f);
          } else {
            // rare path: the step in natural log, max-shifted, from the tables in memory
            float lp;
            if (t == 0) {
              lp = act ? a.log_pi[j] : CE_NEG_INF;
            } else {
              const float lx = logf(xf);
              float m = CE_NEG_INF;
              for (int i = 0; i < S; ++i) {
                const float la = act ? a.log_A[i * S + j] : CE_NEG_INF;
                m = fmaxf(m, ce_lane(lx, i) + la);
              }
              float sm = 0.f;
              for (int i = 0; i < S; ++i) {
                const float la = act ? a.log_A[i * S + j] : CE_NEG_INF;
                const float v = ce_lane(lx, i) + la;
                sm += v == CE_NEG_INF ? 0.f : expf(v - m);
              }
              lp = m == CE_NEG_INF ? CE_NEG_INF : m + logf(sm);
            }
            const float lb = log_e(s, Mv);
            const float ly = (lp == CE_NEG_INF || lb == CE_NEG_INF) ? CE_NEG_INF : lp + lb;
            const float M = ce_red<SP>(ly, CeMax{});
            if (ce_uni(M) == CE_NEG_INF) {
              status = 1;
              break;
            }
            const float ex = ly == CE_NEG_INF ? 0.f : expf(ly - M);
            const float st = ce_red<SP>(ex, CeAdd{});
            xf = ex / st;
            Sll += (double)M + (double)logf(st);
          }
          if ((s & 3) == 3) {
            asm volatile("");  // a real (scalar) branch: the log and the fp64 add run every fourth step only
            Sll += (double)__builtin_amdgcn_logf(Pm) * CE_LN2;
            Pm = 1.f;
          }
          if (act) al[(int64_t)t * S + j] = xf;
        }
        Sll += (double)__builtin_amdgcn_logf(Pm) * CE_LN2;
        Pm = 1.f;
      }
      Sll -= (double)Dr;
    }
    if (status != 0) {
      if (a.loglik && lane == 0) a.loglik[b] = status == 1 ? CE_NEG_INF : ce_nan();
      if (gm_out)
        for (int64_t e = lane; e < (int64_t)L * S; e += 64) gm_out[e] = 0.f;
      continue;
    }
    if (a.loglik && lane == 0) a.loglik[b] = (float)Sll;
    const double wt = a.weights ? (double)ce_uni(a.weights[b]) : 1.0;  // the sequence's weight in every count
    __threadfence();  // the staging loads below read rows other lanes of this wave stored

    // ----------------------------------------------------------------- backward
    {
      float Arow[SP], tc[SP];
#pragma unroll
      for (int q = 0; q < SP; ++q) {
        Arow[q] = (act && q < S) ? __expf(a.log_A[j * S + q]) : 0.f;
        tc[q] = 0.f;
      }
      float bn = act ? 1.f : 0.f;
      // t = L - 1: gamma = x_{L-1}
      float glast = act ? xf : 0.f;  // the gamma row of the next chunk's last step
      float oc = glast;
      if (act) {
        if (gm_out) gm_out[(int64_t)(L - 1) * S + j] = xf;
        if (L == 1) pc64 = fma(wt, (double)xf, pc64);
      }
      for (int t0 = ((L - 1) / CE_CH) * CE_CH; t0 >= 0; t0 -= CE_CH) {
        const int n = min(CE_CH, L - t0);
        float Mv;
        stage(t0, n, Mv);
        // x rows t0 - 1 .. t0 + n - 2 (row s <-> time t0 + s - 1), one contiguous span.  A step overwrites the
        // row it consumed with its gamma (the same time), so after the steps rows 1 .. n hold gamma_{t0 .. t0+n-1}
        for (int k = lane; k < n * S; k += 64) {
          const int64_t o = (int64_t)(t0 - 1) * S + k;
          abuf[k] = o >= 0 ? al[o] : 0.f;
        }
        if (act) abuf[n * S + j] = glast;
        asm volatile("" ::: "memory");  // the wave's own LDS stores above, read across lanes below
        float e_nx = ebuf[(n - 1) * ES + jj], xp_nx = act ? abuf[(n - 1) * S + j] : 0.f;
        for (int s = n - 1; s >= 0; --s) {
          const int t = t0 + s;
          if (t == 0) break;
          // this step's operands were read a step ago
          const float e = e_nx, xp = xp_nx;
          const int sn = max(s - 1, 0);
          e_nx = ebuf[sn * ES + jj];
          xp_nx = act ? abuf[sn * S + j] : 0.f;
          const float w = act ? e * bn : 0.f;
          float p[SP], b0 = 0.f, b1 = 0.f;
#pragma unroll
          for (int q = 0; q < SP; q += 2) {
            p[q] = Arow[q] * ce_lane(w, q);
            b0 += p[q];
            if (q + 1 < SP) {
              p[q + 1] = Arow[q + 1] * ce_lane(w, q + 1);
              b1 += p[q + 1];
            }
          }
          const float bnew = b0 + b1;
          const float g = xp * bnew;
          const float Z = ce_red<SP>(g, CeAdd{});
          const float sb = ce_red<SP>(bnew, CeAdd{});
          const float Zu = ce_uni(Z), sbu = ce_uni(sb);
          float gm;
          if (Zu >= CE_LO && Zu <= CE_HI && sbu >= CE_LO && sbu <= CE_HI) {
            const float rZ = __builtin_amdgcn_rcpf(Z);
            gm = g * rZ;
            const float cf = xp * rZ;
#pragma unroll
            for (int q = 0; q < SP; ++q) tc[q] = fmaf(cf, p[q], tc[q]);
            bn = bnew * __builtin_amdgcn_rcpf(sb);
          } else {
            // rare path: the step in natural log, max-shifted
            const float lbn = logf(bn);
            const float lbe = log_e(s, Mv);
            const float lw = (lbe == CE_NEG_INF || lbn == CE_NEG_INF) ? CE_NEG_INF : lbe + lbn;
            const float lxp = act ? logf(xp) : CE_NEG_INF;
            float v[SP], m = CE_NEG_INF;
#pragma unroll
            for (int q = 0; q < SP; ++q) {
              const float la = (act && q < S) ? a.log_A[j * S + q] : CE_NEG_INF;
              const float lq = ce_lane(lw, q);
              v[q] = (la == CE_NEG_INF || lq == CE_NEG_INF) ? CE_NEG_INF : la + lq;
              m = fmaxf(m, v[q]);
            }
            float sm = 0.f;
#pragma unroll
            for (int q = 0; q < SP; ++q) sm += v[q] == CE_NEG_INF ? 0.f : expf(v[q] - m);
            const float lb = m == CE_NEG_INF ? CE_NEG_INF : m + logf(sm);  // ln b_{t-1}(i)
            const float lg = (lb == CE_NEG_INF || lxp == CE_NEG_INF) ? CE_NEG_INF : lb + lxp;
            const float Mg = ce_red<SP>(lg, CeMax{});
            const float Mb = ce_red<SP>(lb, CeMax{});
            if (ce_uni(Mg) == CE_NEG_INF) {
              gm = 0.f;
            } else {
              const float ex = lg == CE_NEG_INF ? 0.f : expf(lg - Mg);
              const float Zs = ce_red<SP>(ex, CeAdd{});
              gm = ex / Zs;
#pragma unroll
              for (int q = 0; q < SP; ++q) {
                const float lv = (v[q] == CE_NEG_INF || lxp == CE_NEG_INF) ? CE_NEG_INF : v[q] + lxp;
                tc[q] += lv == CE_NEG_INF ? 0.f : expf(lv - Mg) / Zs;
              }
            }
            if (ce_uni(Mb) == CE_NEG_INF) {
              bn = 0.f;
            } else {
              const float eb = lb == CE_NEG_INF ? 0.f : expf(lb - Mb);
              bn = eb / ce_red<SP>(eb, CeAdd{});
            }
          }
          // gamma_{t-1} over x_{t-1}'s row (read a step ago); at s = 0 it is the next chunk's last row
          if (act) abuf[s * S + j] = gm;
          if (s == 0) glast = gm;
          oc += gm;
          if (act) {
            if (gm_out) gm_out[(int64_t)(t - 1) * S + j] = gm;
            if (t == 1) pc64 = fma(wt, (double)gm, pc64);
          }
        }
        // the chunk's counts: occ took gamma_{t-1} of the steps above (and gamma_{L-1} with the tail chunk)
#pragma unroll
        for (int q = 0; q < SP; ++q) {
          tc64[q] = fma(wt, (double)tc[q], tc64[q]);
          tc[q] = 0.f;
        }
        oc64 = fma(wt, (double)oc, oc64);
        oc = 0.f;
        asm volatile("" ::: "memory");
        // moments of rows t0 .. t0 + n - 1: their gamma rows are abuf's rows 1 .. n
        gf_chunk_moments(xbuf, DS, abuf + S, shl, pij, S, D, n, lane, wt, slab);
        asm volatile("" ::: "memory");
      }
    }
  }

  // the workgroup's partial: its waves' slabs in wave order
  asm volatile("" ::: "memory");
  double* tr = reinterpret_cast<double*>(xbuf);
  if (act) {
#pragma unroll
    for (int q = 0; q < SP; ++q)
      if (q < S) tr[j * S + q] = tc64[q];
    tr[S * S + j] = pc64;
    tr[S * S + S + j] = oc64;
  }
  __syncthreads();
  double* part = a.part + (int64_t)blockIdx.x * (SL + NT);
  for (int k = tid; k < SL; k += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += gf_smem[(size_t)w * SL + k];
    part[k] = acc;
  }
  for (int k = tid; k < NT; k += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += reinterpret_cast<const double*>(wave0 + w * wfl)[k];
    part[SL + k] = acc;
  }
}

// ------------------------------------------------------------------------------ moments entry
struct GaussMomArgs {
  const float* x;
  const float* gamma;
  const int64_t* lengths;
  const float* shift;    // (D), nullable (= 0)
  const float* weights;  // (B), nullable (= all 1)
  int64_t B;
  int T, S, D;
  int32_t* bad;   // (B): 1 where the sequence has a non-finite x or gamma inside its length
  double* part;   // the E-step's layout; the trans and pi ranges are not touched
};

// one wave per (sequence, chunk): bad[b] = 1 if a value of the chunk's in-length rows is not finite (bad starts
// zeroed; every writer stores the same 1)
__global__ __launch_bounds__(256) void gauss_moments_flag_kernel(const GaussMomArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nch = cdiv(a.T, CE_CH);
  const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + ce_uni((int)(threadIdx.x >> 6));
  if (w >= a.B * nch) return;
  const int64_t b = w / nch;
  const int t0 = (int)(w - b * nch) * CE_CH;
  const int64_t Lr = a.lengths[b];
  const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < a.T ? Lr : a.T)));
  const int n = max(0, min(CE_CH, L - t0));
  const float* xg = a.x + (b * a.T + t0) * (int64_t)a.D;
  const float* gg = a.gamma + (b * a.T + t0) * (int64_t)a.S;
  bool bad = false;
  for (int k = lane; k < n * a.D; k += 64) bad |= gf_nonfinite(xg[k]);
  for (int k = lane; k < n * a.S; k += 64) bad |= gf_nonfinite(gg[k]);
  if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) a.bad[b] = 1;
}

// LDS: [slab nw x SL doubles] [shift D][pij P] (an even count of words) [per wave: xbuf 64 DS | gbuf 64 S, an even
// count]; at the end a wave's staging buffer holds its S occ doubles
__global__ __launch_bounds__(256) void gauss_moments_kernel(const GaussMomArgs a) {
  extern __shared__ double gf_smem[];
  const int S = a.S, D = a.D, T = a.T;
  const int P = gf_tri(D), SD = S * D, SL = SD + S * P, NT = S * S + 2 * S, DS = gf_odd(D);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  double* slab = gf_smem + (size_t)wave * SL;
  float* shl = reinterpret_cast<float*>(gf_smem + (size_t)nw * SL);
  uint32_t* pij = reinterpret_cast<uint32_t*>(shl + D);
  const int wfl = (CE_CH * (DS + S) + 1) & ~1;
  float* wave0 = shl + ((D + P + 1) & ~1);
  float* xbuf = wave0 + wave * wfl;
  float* gbuf = xbuf + CE_CH * DS;
  gf_pairs(D, pij, tid, (int)blockDim.x);
  for (int k = tid; k < D; k += blockDim.x) shl[k] = a.shift ? a.shift[k] : 0.f;
  for (int k = tid; k < nw * SL; k += blockDim.x) gf_smem[k] = 0.0;
  __syncthreads();

  double oc64 = 0.0;
  const int64_t nch = cdiv(T, CE_CH);
  for (int64_t w = (int64_t)blockIdx.x * nw + wave; w < a.B * nch; w += (int64_t)gridDim.x * nw) {
    const int64_t b = w / nch;
    const int t0 = (int)(w - b * nch) * CE_CH;
    const int64_t Lr = a.lengths[b];
    const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
    const int n = max(0, min(CE_CH, L - t0));
    if (n == 0 || ce_uni(a.bad[b]) != 0) continue;
    const double wt = a.weights ? (double)ce_uni(a.weights[b]) : 1.0;
    asm volatile("" ::: "memory");
    gf_stage_x(a.x + (b * T + t0) * (int64_t)D, n, D, DS, lane, xbuf);
    const float* gg = a.gamma + (b * T + t0) * (int64_t)S;
    for (int k = lane; k < n * S; k += 64) gbuf[k] = gg[k];
    asm volatile("" ::: "memory");
    if (lane < S) {
      float oc = 0.f;
      for (int r = 0; r < n; ++r) oc += gbuf[r * S + lane];
      oc64 = fma(wt, (double)oc, oc64);
    }
    gf_chunk_moments(xbuf, DS, gbuf, shl, pij, S, D, n, lane, wt, slab);
    asm volatile("" ::: "memory");
  }

  asm volatile("" ::: "memory");
  if (lane < S) reinterpret_cast<double*>(xbuf)[lane] = oc64;
  __syncthreads();
  double* part = a.part + (int64_t)blockIdx.x * (SL + NT);
  for (int k = tid; k < SL; k += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += gf_smem[(size_t)w * SL + k];
    part[k] = acc;
  }
  for (int k = tid; k < S; k += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += reinterpret_cast<const double*>(wave0 + w * wfl)[k];
    part[SL + S * S + S + k] = acc;
  }
}

// ---------------------------------------------------------------------------------------- host
struct GaussFullPlan {
  int nw;
  int64_t nblk;
  size_t lds_bytes;
  size_t off_part, bytes;
};

// sh: the workgroup's shared bytes, pw: a wave's; items: what the waves stride over; head: the workspace bytes in
// front of the partials
GaussFullPlan gf_plan(size_t sh, size_t pw, int64_t items, size_t head, int64_t S, int64_t D) {
  GaussFullPlan p;
  // the waves per workgroup that put most waves on a CU (4 at most: one per SIMD at these register counts);
  // on a tie the fewest, which spreads a small batch over more CUs
  p.nw = 1;
  int64_t best = 0;
  for (int64_t nw = 1; nw <= GF_MAX_NW; ++nw) {
    const size_t wg = sh + (size_t)nw * pw;
    if (wg > GF_LDS_MAX) break;
    int64_t per_cu = (int64_t)(GF_LDS_CU / wg) * nw;
    per_cu = per_cu > 4 ? 4 : per_cu;
    if (per_cu > best) {
      best = per_cu;
      p.nw = (int)nw;
    }
  }
  p.nblk = cdiv(items, p.nw) < GF_MAX_WAVES / p.nw ? cdiv(items, p.nw) : GF_MAX_WAVES / p.nw;
  if (p.nblk < 1) p.nblk = 1;
  p.lds_bytes = sh + (size_t)p.nw * pw;
  p.off_part = r256(head);
  p.bytes = p.off_part + (size_t)p.nblk * (S * D + S * gf_tri((int)D) + S * S + 2 * S) * 8;
  return p;
}

GaussFullPlan gauss_full_plan(int64_t B, int64_t T, int64_t S, int64_t D) {
  int64_t SP = 1;
  while (SP < S) SP *= 2;
  const int64_t P = gf_tri((int)D), SL = S * D + S * P;
  const size_t sh = (size_t)((S * P + S * D + S + D + P + 1) & ~(int64_t)1) * 4;
  const size_t pw = (size_t)SL * 8 +
                    (size_t)((CE_CH * (gf_odd((int)D) + gf_odd((int)SP)) + (CE_CH + 1) * S + 1) & ~(int64_t)1) * 4;
  return gf_plan(sh, pw, B, (size_t)B * T * S * 4, S, D);
}

GaussFullPlan gauss_moments_plan(int64_t B, int64_t T, int64_t S, int64_t D) {
  const int64_t P = gf_tri((int)D), SL = S * D + S * P;
  const size_t sh = (size_t)((D + P + 1) & ~(int64_t)1) * 4;
  const size_t pw = (size_t)SL * 8 + (size_t)((CE_CH * (gf_odd((int)D) + S) + 1) & ~(int64_t)1) * 4;
  return gf_plan(sh, pw, B * cdiv(T, CE_CH), (size_t)B * 4, S, D);
}

template <int SP, bool MEM>
int gauss_full_go(const GaussFullArgs& a, const GaussFullPlan& p, int64_t M, hipStream_t s) {
  auto kern = gauss_full_estep_kernel<SP, MEM>;
  // more than 64 KB of dynamic LDS has to be asked for, once per kernel
  static const hipError_t big_lds = hipFuncSetAttribute(
      reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GF_LDS_MAX);
  (void)big_lds;
  kern<<<dim3((unsigned)p.nblk, (unsigned)M), 64 * p.nw, p.lds_bytes, s>>>(a);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

template <bool MEM>
int gauss_full_width(const GaussFullArgs& a, const GaussFullPlan& p, int64_t M, hipStream_t s) {
  if (a.S > 16) return gauss_full_go<32, MEM>(a, p, M, s);
  if (a.S > 8) return gauss_full_go<16, MEM>(a, p, M, s);
  if (a.S > 4) return gauss_full_go<8, MEM>(a, p, M, s);
  if (a.S > 2) return gauss_full_go<4, MEM>(a, p, M, s);
  if (a.S > 1) return gauss_full_go<2, MEM>(a, p, M, s);
  return gauss_full_go<1, MEM>(a, p, M, s);
}

// the batch sizes the launches index (and whose workspace size fits size_t): the queries and the launchers agree
bool gauss_full_sizes_ok(int64_t B, int64_t T) {
  return B <= INT32_MAX && T <= (1 << 28) && (B == 0 || T <= (int64_t(1) << 40) / B);
}

// the decode and filter kernels' view of this file's emissions (hmm_gauss_decode_dev.h): the table is
// [W S*P][mu S*D][c S]
struct GaussFullEm {
  __host__ __device__ static int table_floats(int S, int D) { return S * gf_tri(D) + S * D + S; }
  // 4 waves per SIMD up to SP = 8 (<= 128 VGPRs), 3 at SP = 16 (126 and 139), 2 at SP = 32 (171 and 188)
  static int cu_waves(int SP) { return SP > 16 ? 8 : SP > 8 ? 12 : 16; }
  __device__ __forceinline__ static void table(const float* __restrict__ mean, const float* __restrict__ prec, int S,
                                               int D, float* tb, int tid, int nthr) {
    gf_table(mean, prec, S, D, tb, tb + S * gf_tri(D), tb + S * gf_tri(D) + S * D, tid, nthr);
  }
  __device__ __forceinline__ static bool stage_x(const float* __restrict__ xg, int n, int D, int DS, int lane,
                                                 float* xbuf) {
    return gf_stage_x(xg, n, D, DS, lane, xbuf);
  }
  __device__ __forceinline__ static bool chunk_em(const float* xbuf, int DS, const float* tb, int S, int D, int n,
                                                  int lane, float* ebuf, int ES, float& Mv) {
    const int P = gf_tri(D);
    return gf_chunk_em(xbuf, DS, tb + S * P, tb, tb + S * P + S * D, S, D, n, lane, ebuf, ES, Mv);
  }
  __device__ __forceinline__ static float em_one(const float* xr, const float* tb, int j, int S, int D) {
    const int P = gf_tri(D);
    return gf_em(xr, tb + S * P + j * D, tb + j * P, tb[S * P + S * D + j], D);
  }
};

}  // namespace

}  // namespace vqhmm

#include "hmm_gauss_decode_dev.h"

namespace vqhmm {

bool hmm_gauss_full_supported(int64_t S, int64_t D) {
  return S >= 1 && S <= 32 && D >= 1 && D <= 32 && S * D * D <= GF_MAX_SDD;
}

size_t hmm_gauss_full_estep_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D) {
  if (!hmm_gauss_full_supported(S, D) || B < 0 || T < 0 || !gauss_full_sizes_ok(B, T)) return 0;
  return gauss_full_plan(B, T, S, D).bytes;
}

size_t hmm_gauss_moments_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D) {
  if (!hmm_gauss_full_supported(S, D) || B < 0 || T < 0 || !gauss_full_sizes_ok(B, T)) return 0;
  return gauss_moments_plan(B, T, S, D).bytes;
}

int launch_hmm_gauss_full_emission(const float* mean, const float* prec_chol, const float* x, const int64_t* lengths,
                                   int64_t B, int64_t T, int64_t S, int64_t D, float* em, hipStream_t s) {
  if (!hmm_gauss_full_supported(S, D) || !gauss_full_sizes_ok(B, T)) return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) return VQHMM_OK;
  const size_t sh = (size_t)(S * gf_tri((int)D) + S * D + S) * 4;
  const size_t pw = (size_t)CE_CH * (gf_odd((int)D) + gf_odd((int)S)) * 4;
  int64_t nw = (int64_t)((GF_LDS_SOFT - sh) / pw);
  nw = nw < 1 ? 1 : nw > GF_MAX_NW ? GF_MAX_NW : nw;
  const int64_t nblk = cdiv(B * cdiv(T, CE_CH), nw);
  if (nblk > INT32_MAX) return VQHMM_EUNSUPPORTED;
  gauss_full_emission_kernel<<<(unsigned)nblk, 64 * (int)nw, sh + (size_t)nw * pw, s>>>(
      mean, prec_chol, x, lengths, B, (int)T, (int)S, (int)D, em);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_gauss_full_estep(const float* log_pi, const float* log_A, const float* mean, const float* prec_chol,
                                const float* x, const int64_t* lengths, const float* shift, const float* weights,
                                int64_t B, int64_t T, int64_t S, int64_t D, double* pi_cnt, double* trans_cnt,
                                double* occ, double* m1, double* m2, float* loglik, float* gamma, void* ws,
                                hipStream_t s) {
  return launch_hmm_gauss_full_estep_batched(log_pi, log_A, mean, prec_chol, x, lengths, shift, weights, B, T, S, D,
                                             1, pi_cnt, trans_cnt, occ, m1, m2, loglik, gamma, ws, s);
}

// M members: M single-model workspaces, each rounded up to 256 bytes
size_t hmm_gauss_full_estep_batched_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D, int64_t M) {
  if (!hmm_gauss_full_supported(S, D) || !hmm_code_members_supported(M) || B < 0 || T < 0 ||
      !gauss_full_sizes_ok(B, T))
    return 0;
  return (size_t)M * r256(gauss_full_plan(B, T, S, D).bytes);
}

int launch_hmm_gauss_full_estep_batched(const float* log_pi, const float* log_A, const float* mean,
                                        const float* prec_chol, const float* x, const int64_t* lengths,
                                        const float* shift, const float* weights, int64_t B, int64_t T, int64_t S,
                                        int64_t D, int64_t M, double* pi_cnt, double* trans_cnt, double* occ,
                                        double* m1, double* m2, float* loglik, float* gamma, void* ws,
                                        hipStream_t s) {
  if (!hmm_gauss_full_supported(S, D) || !hmm_code_members_supported(M) || !gauss_full_sizes_ok(B, T))
    return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) {
    if (hipMemsetAsync(pi_cnt, 0, sizeof(double) * M * S, s) != hipSuccess ||
        hipMemsetAsync(trans_cnt, 0, sizeof(double) * M * S * S, s) != hipSuccess ||
        hipMemsetAsync(occ, 0, sizeof(double) * M * S, s) != hipSuccess ||
        hipMemsetAsync(m1, 0, sizeof(double) * M * S * D, s) != hipSuccess ||
        hipMemsetAsync(m2, 0, sizeof(double) * M * S * D * D, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    // length-0 sequences: loglik = NaN (all-ones words)
    if (B > 0 && loglik && hipMemsetAsync(loglik, 0xFF, sizeof(float) * M * B, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    return VQHMM_OK;
  }
  const GaussFullPlan p = gauss_full_plan(B, T, S, D);
  char* w = static_cast<char*>(ws);
  GaussFullArgs a;
  a.log_pi = log_pi; a.log_A = log_A; a.mean = mean; a.prec = prec_chol; a.x = x; a.lengths = lengths;
  a.shift = shift; a.weights = weights;
  a.B = B; a.T = (int)T; a.S = (int)S; a.D = (int)D;
  a.alpha = reinterpret_cast<float*>(w);
  a.part = reinterpret_cast<double*>(w + p.off_part);
  a.loglik = loglik; a.gamma = gamma;
  a.mstride = r256(p.bytes);
  const int rc = M > 1 ? gauss_full_width<true>(a, p, M, s) : gauss_full_width<false>(a, p, M, s);
  if (rc) return rc;
  const int64_t NE = S * D + S * gf_tri((int)D) + S * S + 2 * S;
  gauss_full_reduce_kernel<<<dim3((unsigned)cdiv(NE, GF_RK), (unsigned)M), GF_RK * GF_RP, 0, s>>>(
      a.part, a.mstride, (int)p.nblk, (int)S, (int)D, pi_cnt, trans_cnt, occ, m1, m2);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_gauss_moments(const float* x, const float* gamma, const int64_t* lengths, const float* shift,
                             const float* weights, int64_t B, int64_t T, int64_t S, int64_t D, double* occ,
                             double* m1, double* m2, void* ws, hipStream_t s) {
  if (!hmm_gauss_full_supported(S, D) || !gauss_full_sizes_ok(B, T)) return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) {
    if (hipMemsetAsync(occ, 0, sizeof(double) * S, s) != hipSuccess ||
        hipMemsetAsync(m1, 0, sizeof(double) * S * D, s) != hipSuccess ||
        hipMemsetAsync(m2, 0, sizeof(double) * S * D * D, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    return VQHMM_OK;
  }
  const GaussFullPlan p = gauss_moments_plan(B, T, S, D);
  char* w = static_cast<char*>(ws);
  GaussMomArgs a;
  a.x = x; a.gamma = gamma; a.lengths = lengths; a.shift = shift; a.weights = weights;
  a.B = B; a.T = (int)T; a.S = (int)S; a.D = (int)D;
  a.bad = reinterpret_cast<int32_t*>(w);
  a.part = reinterpret_cast<double*>(w + p.off_part);
  if (hipMemsetAsync(a.bad, 0, sizeof(int32_t) * B, s) != hipSuccess) return VQHMM_ELAUNCH;
  const int64_t items = B * cdiv(T, CE_CH);
  if (cdiv(items, 4) > INT32_MAX) return VQHMM_EUNSUPPORTED;
  gauss_moments_flag_kernel<<<(unsigned)cdiv(items, 4), 256, 0, s>>>(a);
  VQHMM_LAUNCH_CHECK();
  static const hipError_t big_lds =
      hipFuncSetAttribute(reinterpret_cast<const void*>(gauss_moments_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)GF_LDS_MAX);
  (void)big_lds;
  gauss_moments_kernel<<<(unsigned)p.nblk, 64 * p.nw, p.lds_bytes, s>>>(a);
  VQHMM_LAUNCH_CHECK();
  const int64_t NE = S * D + S * gf_tri((int)D) + S * S + 2 * S;
  gauss_full_reduce_kernel<<<(unsigned)cdiv(NE, GF_RK), GF_RK * GF_RP, 0, s>>>(a.part, 0, (int)p.nblk, (int)S,
                                                                              (int)D, nullptr, nullptr, occ, m1, m2);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

size_t hmm_gauss_full_viterbi_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D) {
  if (!hmm_gauss_full_supported(S, D) || B < 0 || T < 0 || !gauss_full_sizes_ok(B, T)) return 0;
  return gd_viterbi_ws_bytes(B, T, S);
}

int launch_hmm_gauss_full_viterbi(const float* log_pi, const float* log_A, const float* mean, const float* prec_chol,
                                  const float* x, const int64_t* lengths, int64_t B, int64_t T, int64_t S,
                                  int64_t D, int32_t* path, float* score, void* ws, hipStream_t s) {
  if (!hmm_gauss_full_supported(S, D) || !gauss_full_sizes_ok(B, T)) return VQHMM_EUNSUPPORTED;
  if (B == 0) return VQHMM_OK;
  return gd_launch_viterbi<GaussFullEm>(log_pi, log_A, mean, prec_chol, x, lengths, B, T, S, D, path, score, ws, s);
}

int launch_hmm_gauss_full_filter(const float* log_pi, const float* log_A, const float* mean, const float* prec_chol,
                                 const float* x, const int64_t* lengths, const float* prev, int64_t B, int64_t T,
                                 int64_t S, int64_t D, float* filt, float* last, float* loglik, hipStream_t s) {
  if (!hmm_gauss_full_supported(S, D) || !gauss_full_sizes_ok(B, T)) return VQHMM_EUNSUPPORTED;
  if (B == 0) return VQHMM_OK;
  return gd_launch_filter<GaussFullEm>(log_pi, log_A, mean, prec_chol, x, lengths, prev, B, T, S, D, filt, last,
                                       loglik, s);
}

}  // namespace vqhmm
