// Stationary HMM with diagonal-Gaussian emissions on continuous observations: the emission log-densities, the
// fused Baum-Welch E-step and the ancestral sampler (contracts in include/vqhmm.h, fp64 restatement in
// tests/gauss_hmm_ref.py; DESIGN.md "Gaussian HMM").
//
//   model   log_pi (S), log_A (S,S) rows = from-state, mean (S,D), log_var (S,D)
//   data    x (B,T,D), lengths (B), shift (D) (nullable): every moment is taken of x - shift
//   E-step  pi_cnt = sum_b gamma_0, trans_cnt = sum xi_t, occ = sum gamma_t, m1 = sum gamma_t(s) (x_t - shift),
//           m2 = sum gamma_t(s) (x_t - shift)^2 (fp64), loglik (B), gamma (B,T,S) (optional)
//
// Emissions.  em[t,s] = -1/2 sum_d (x_d - mu_sd)^2 exp(-log_var_sd) + c_s, c_s = -1/2 sum_d log_var_sd -
// (D/2) ln 2 pi (summed in fp64, rounded once).  Every workgroup of both kernels builds the same table
// (mu, exp(-log_var), c) in LDS with ge_table and evaluates ge_em, the one function that holds the arithmetic,
// with lane = time step on a chunk of 64 rows of x staged in LDS: the parameters are wave-uniform LDS
// broadcasts, and the E-step's internal emissions are the bits the emission entry writes (the file is built
// without contraction).
//
// Chain.  hmm_code.hip's plan: one sequence per wave, lane j < S = state j, exp(log_A) in SP registers, linear
// probabilities normalised at every step, the product of four step masses through one log2 into the fp64
// log-likelihood, a step whose mass leaves [2^-30, 2^30] redone max-shifted in natural log, a mass that is truly
// 0 ends the sequence (loglik = -inf, no contribution).  A step's emission vector is e_t = exp(em_t - max_s
// em_t), written to LDS by the chunk's lane = time pass; the maxima are added to the fp64 sum.  A non-finite x
// or emission inside the length makes loglik NaN and the sequence leaves every count.  The scaled forward
// vectors (4 S bytes per position) are the only per-position workspace; the backward pass stages the chunk's x
// again (it needs it for the moments anyway) and recomputes the emissions from it.
//
// Counts.  xi accumulates in SP registers as in hmm_code.hip (fp32 within a chunk, fp64 across).  The chunk's
// gamma rows go to LDS; after the chunk's steps the moment sums are the product gamma^T (S x 64) .
// [y, y^2] (64 x 2D), y = x - shift, taken on the f32 MFMA (v_mfma_f32_16x16x4_f32, a k-ordered fp32 fma chain
// within the chunk; measured against the same product on the VALU in DESIGN.md), and added with the
// sequence's weight in one fp64 fma each to the wave's private LDS slab.  A workgroup sums its waves'
// slabs in wave order into its partial, a second launch sums the partials in a fixed order: no atomics, the same
// bits run to run.  Sequences are assigned statically (wave w of workgroup g takes b = g NW + w, then strides).
//
// Members.  blockIdx.y is the member of a stack of M models that share x, lengths and shift (the batched entry; the
// single-model entry is M = 1), as in hmm_code.hip: a member has its own parameter slices, weights row, alpha rows,
// partials (`mstride` workspace bytes apart) and output blocks, and runs exactly the single model's plan, so its
// bits are the single-model call's.  Each member stages x again.
//
// Addressing.  x is read only at rows t < L of the wave's own sequence, parameters only at (s, d) < (S, D), the
// workspace only inside the sequence's own rows.
//
// Decode and filter.  The Viterbi decode and the streaming causal filter on x are hmm_gauss_decode_dev.h's
// kernels, instantiated at the end of this file on GaussDiagEm (ge_table, ge_stage_x, ge_chunk_em, ge_em), so
// that their emissions are this file's bits.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // the header's table prologue is not used here
#include "hmm_code_dev.h"  // the lane helpers and the fast step's range
#pragma clang diagnostic pop

namespace vqhmm {

namespace {

constexpr int GE_MAX_NW = 4;                   // waves (private slabs) per workgroup, at most
constexpr size_t GE_LDS_SOFT = 64 * 1024;      // the emission entry's workgroups stay under this
constexpr size_t GE_LDS_CU = 160 * 1024;       // a CU's LDS
constexpr size_t GE_LDS_MAX = 156 * 1024;      // of the CU's 160 KB
constexpr int64_t GE_MAX_WAVES = 2048;         // waves of the grid (partials: one per workgroup)
constexpr double GE_LN2PI = 1.8378770664093454836;
typedef float ge_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool ge_nonfinite(float v) {
  return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u;
}
__host__ __device__ __forceinline__ int ge_odd(int v) { return v | 1; }

// (mu, exp(-log_var), c) in LDS, by every thread of the workgroup; the caller synchronises
__device__ __forceinline__ void ge_table(const float* __restrict__ mean, const float* __restrict__ log_var, int S,
                                         int D, float* mu, float* iv, float* cs, int tid, int nthr) {
  for (int k = tid; k < S * D; k += nthr) {
    mu[k] = mean[k];
    iv[k] = expf(-log_var[k]);
  }
  for (int s = tid; s < S; s += nthr) {
    double acc = 0.0;
    for (int d = 0; d < D; ++d) acc += (double)log_var[s * D + d];
    cs[s] = (float)(-0.5 * acc - 0.5 * (double)D * GE_LN2PI);
  }
}

// the emission log-density of one row of x under one state: the only place this arithmetic is written
__device__ __forceinline__ float ge_em(const float* xr, const float* mu, const float* iv, float c, int D) {
  float acc = 0.f;
  for (int d = 0; d < D; ++d) {
    const float z = xr[d] - mu[d];
    acc = fmaf(z * z, iv[d], acc);
  }
  return fmaf(-0.5f, acc, c);
}

// rows [0, n) of a sequence's x (xg = its row t0, n D contiguous floats) into xbuf with row stride DS;
// -> whether any of them is not finite (wave-uniform)
__device__ __forceinline__ bool ge_stage_x(const float* __restrict__ xg, int n, int D, int DS, int lane,
                                           float* xbuf) {
  const int q = 64 / D, rm = 64 - q * D;
  int r = lane / D, c = lane - r * D;
  bool bad = false;
  for (int k = lane; k < n * D; k += 64) {
    const float v = xg[k];
    xbuf[r * DS + c] = v;
    bad |= ge_nonfinite(v);
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
__device__ __forceinline__ bool ge_chunk_em(const float* xbuf, int DS, const float* mu, const float* iv,
                                            const float* cs, int S, int D, int n, int lane, float* ebuf, int ES,
                                            float& Mv) {
  float M = CE_NEG_INF;
  bool bad = false;
  if (lane < n) {
    for (int s = 0; s < S; ++s) {
      const float em = ge_em(xbuf + lane * DS, mu + s * D, iv + s * D, cs[s], D);
      ebuf[lane * ES + s] = em;
      M = fmaxf(M, em);
      bad |= ge_nonfinite(em);
    }
  }
  Mv = lane < n ? M : 0.f;
  return __builtin_amdgcn_ballot_w64(bad) != 0;
}

struct GaussArgs {
  const float* log_pi;
  const float* log_A;
  const float* mean;
  const float* log_var;
  const float* x;
  const int64_t* lengths;
  const float* shift;    // (D), nullable (= 0)
  const float* weights;  // (M, B), nullable (= all 1)
  int64_t B;
  int T, S, D;
  float* alpha;   // (B, T, S) scaled forward vectors
  double* part;   // [gridDim.x][m1 S*D | m2 S*D | trans S*S | pi S | occ S]
  float* loglik;  // nullable
  float* gamma;   // nullable
  size_t mstride;  // bytes from a member's alpha / part to the next member's
};

// member m's view of the arguments (m = 0 changes nothing): x, lengths and shift are shared
__device__ __forceinline__ GaussArgs gauss_member(GaussArgs a, int64_t m) {
  a.log_pi += m * a.S;
  a.log_A += m * a.S * a.S;
  a.mean += m * a.S * a.D;
  a.log_var += m * a.S * a.D;
  if (a.weights) a.weights += m * a.B;
  a.alpha = reinterpret_cast<float*>(reinterpret_cast<char*>(a.alpha) + m * a.mstride);
  a.part = reinterpret_cast<double*>(reinterpret_cast<char*>(a.part) + m * a.mstride);
  if (a.loglik) a.loglik += m * a.B;
  if (a.gamma) a.gamma += m * a.B * (int64_t)a.T * a.S;
  return a;
}

// ------------------------------------------------------------------------------ emission entry
// one chunk of 64 rows per wave; LDS: [mu S*D][iv S*D][c S] [per wave: xbuf 64*DS, obuf 64*OS]
__global__ __launch_bounds__(256) void gauss_emission_kernel(const float* __restrict__ mean,
                                                             const float* __restrict__ log_var,
                                                             const float* __restrict__ x,
                                                             const int64_t* __restrict__ lengths, int64_t B, int T,
                                                             int S, int D, float* __restrict__ em) {
  extern __shared__ float ge_smem_f[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int DS = ge_odd(D), OS = ge_odd(S);
  float* mu = ge_smem_f;
  float* iv = mu + S * D;
  float* cs = iv + S * D;
  float* xbuf = cs + S + wave * (CE_CH * (DS + OS));
  float* obuf = xbuf + CE_CH * DS;
  ge_table(mean, log_var, S, D, mu, iv, cs, tid, (int)blockDim.x);
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
    ge_stage_x(x + (b * T + t0) * (int64_t)D, n, D, DS, lane, xbuf);
    asm volatile("" ::: "memory");
    float Mv;
    ge_chunk_em(xbuf, DS, mu, iv, cs, S, D, n, lane, obuf, OS, Mv);
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

// -------------------------------------------------------------------------------------- E-step
// out = sum over the partials in a fixed order (code_reduce_kernel's scheme): 16 elements per workgroup, thread
// (py, kx) adds partials py, py + 16, .. of element kx in index order, then the 16 sums are added in py order
constexpr int GE_RK = 16, GE_RP = 16;
__global__ __launch_bounds__(GE_RK* GE_RP) void gauss_reduce_kernel(const double* __restrict__ part,
                                                                    size_t mstride, int np, int S, int D,
                                                                    double* __restrict__ pi_cnt,
                                                                    double* __restrict__ trans_cnt,
                                                                    double* __restrict__ occ,
                                                                    double* __restrict__ m1,
                                                                    double* __restrict__ m2) {
  __shared__ double red[GE_RP][GE_RK];
  const int SD = S * D, SS = S * S, NE = 2 * SD + SS + 2 * S;
  const int kx = threadIdx.x % GE_RK, py = threadIdx.x / GE_RK;
  const int k = (int)blockIdx.x * GE_RK + kx;
  const int64_t mem = blockIdx.y;  // member: its own partials (mstride bytes apart) and output blocks
  part = reinterpret_cast<const double*>(reinterpret_cast<const char*>(part) + mem * mstride);
  pi_cnt += mem * S;
  trans_cnt += mem * SS;
  occ += mem * S;
  m1 += mem * SD;
  m2 += mem * SD;
  double acc = 0.0;
  if (k < NE) {
#pragma unroll 4
    for (int p = py; p < np; p += GE_RP) acc += part[(int64_t)p * NE + k];
  }
  red[py][kx] = acc;
  __syncthreads();
  if (py != 0 || k >= NE) return;
  acc = 0.0;
#pragma unroll
  for (int q = 0; q < GE_RP; ++q) acc += red[q][kx];
  if (k < SD) {
    m1[k] = acc;
  } else if (k < 2 * SD) {
    m2[k - SD] = acc;
  } else if (k < 2 * SD + SS) {
    trans_cnt[k - 2 * SD] = acc;
  } else if (k < 2 * SD + SS + S) {
    pi_cnt[k - 2 * SD - SS] = acc;
  } else {
    occ[k - 2 * SD - SS - S] = acc;
  }
}

// WT: the call has weights; without them every weighted add is the plain fp64 add (hmm_code.hip).  MEM: the launch
// has more than one member (blockIdx.y); with one the arguments stay kernel arguments, as in hmm_code.hip
template <int SP, bool WT, bool MEM>
__global__ __launch_bounds__(256) void gauss_estep_kernel(const GaussArgs a0) {
  extern __shared__ double ge_smem[];
  const GaussArgs a = MEM ? gauss_member(a0, blockIdx.y) : a0;
  constexpr int ES = SP | 1;  // row stride of the chunk's emission buffer (odd: the lane = time pass is conflict-free)
  const int S = a.S, D = a.D, T = a.T;
  const int SD = S * D, NT = S * S + 2 * S, DS = ge_odd(D);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int j = lane, jj = j & (SP - 1);
  const bool act = j < S;
  // LDS: [slab nw x 2 SD doubles] [mu SD][iv SD][c S][shift D] (an even count of floats)
  //      [per wave: xbuf 64 DS | ebuf 64 ES | abuf 65 S floats, an even count]; when the wave has run out of
  //      sequences its staging buffers hold its NT transition / pi / occ doubles for the workgroup's sum
  double* slab = ge_smem + (size_t)wave * 2 * SD;
  float* mu = reinterpret_cast<float*>(ge_smem + (size_t)nw * 2 * SD);
  float* iv = mu + SD;
  float* cs = iv + SD;
  float* shl = cs + S;
  const int wfl = (CE_CH * (DS + ES) + (CE_CH + 1) * S + 1) & ~1;  // floats of a wave's staging buffers (>= 2 NT)
  float* wave0 = mu + ((2 * SD + S + D + 1) & ~1);
  float* xbuf = wave0 + wave * wfl;
  float* ebuf = xbuf + CE_CH * DS;
  float* abuf = ebuf + CE_CH * ES;
  ge_table(a.mean, a.log_var, S, D, mu, iv, cs, tid, (int)blockDim.x);
  for (int k = tid; k < D; k += blockDim.x) shl[k] = a.shift ? a.shift[k] : 0.f;
  for (int k = tid; k < nw * 2 * SD; k += blockDim.x) ge_smem[k] = 0.0;
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
      const bool badx = ge_stage_x(xs + (int64_t)t0 * D, n, D, DS, lane, xbuf);
      asm volatile("" ::: "memory");
      const bool bade = ge_chunk_em(xbuf, DS, mu, iv, cs, S, D, n, lane, ebuf, ES, Mv);
      for (int s = 0; s < SP; ++s) {
        const float v = (lane < n && s < S) ? expf(ebuf[lane * ES + s] - Mv) : 0.f;
        ebuf[lane * ES + s] = v;
      }
      asm volatile("" ::: "memory");
      return !(badx || bade);
    };
    // ln e_t(j) of row s of the staged chunk, for the lane's state (the rare paths)
    auto log_e = [&](int s, float Mv) {
      return act ? ge_em(xbuf + s * DS, mu + j * D, iv + j * D, cs[j], D) - ce_lane(Mv, s) : CE_NEG_INF;
    };

    // ------------------------------------------------------------------ forward
    float xf = 0.f;
    double Sll = 0.0;
    int status = 0;  // 1: impossible (mass 0), 2: a non-finite x or emission inside the length
    {
      float Acol[SP];
#pragma unroll
      for (int i = 0; i < SP; ++i) Acol[i] = (act && i < S) ? __expf(a.log_A[i * S + j]) : 0.f;
      const float pij = act ? __expf(a.log_pi[j]) : 0.f;
      float P = 1.f, Dr = 0.f;
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
            u = pij;
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
            P *= c;
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
            Sll += (double)__builtin_amdgcn_logf(P) * CE_LN2;
            P = 1.f;
          }
          if (act) al[(int64_t)t * S + j] = xf;
        }
        Sll += (double)__builtin_amdgcn_logf(P) * CE_LN2;
        P = 1.f;
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
    const double wt = WT ? (double)ce_uni(a.weights[b]) : 1.0;  // the sequence's weight in every count
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
        // moments of rows t0 .. t0 + n - 1: gamma^T (S x n) . [y, y^2] (n x 2D) on v_mfma_f32_16x16x4_f32, in
        // tiles of 16 states x 16 dimensions.  Operand lanes: A[row = lane & 15][k = lane >> 4] = gamma[r = 4 kk +
        // k][s = row], B[k][col = lane & 15] = y[r][d = col]; result register i of a lane is C[row = 4 (lane >>
        // 4) + i][col = lane & 15].  Rows past n and columns past S / D enter as zeros.
        {
          constexpr int MT = SP > 16 ? 2 : 1;
          const int kq = lane >> 4, l15 = lane & 15, nk = (n + 3) >> 2;
          for (int nt = 0; nt * 16 < D; ++nt) {
            const int d = nt * 16 + l15;
            const bool dok = d < D;
            const float shd = dok ? shl[d] : 0.f;
            ge_f4 c1[MT], c2[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) c1[mt] = c2[mt] = ge_f4{0.f, 0.f, 0.f, 0.f};
            for (int kk = 0; kk < nk; ++kk) {
              const int r = 4 * kk + kq;
              const bool rok = r < n;
              const float yv = (rok && dok) ? xbuf[r * DS + d] - shd : 0.f;
              const float y2 = yv * yv;
#pragma unroll
              for (int mt = 0; mt < MT; ++mt) {
                const int s = mt * 16 + l15;
                const float gq = (rok && s < S) ? abuf[(r + 1) * S + s] : 0.f;
                c1[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gq, yv, c1[mt], 0, 0, 0);
                c2[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gq, y2, c2[mt], 0, 0, 0);
              }
            }
            if (dok) {
#pragma unroll
              for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  const int s = mt * 16 + kq * 4 + i;
                  if (s < S) {
                    double* b1p = slab + (s * D + d);
                    double* b2p = b1p + SD;
                    *b1p = fma(wt, (double)c1[mt][i], *b1p);
                    *b2p = fma(wt, (double)c2[mt][i], *b2p);
                  }
                }
              }
            }
          }
        }
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
  double* part = a.part + (int64_t)blockIdx.x * (2 * SD + NT);
  for (int k = tid; k < 2 * SD; k += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += ge_smem[(size_t)w * 2 * SD + k];
    part[k] = acc;
  }
  for (int k = tid; k < NT; k += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += reinterpret_cast<const double*>(wave0 + w * wfl)[k];
    part[2 * SD + k] = acc;
  }
}

// ---------------------------------------------------------------------------- sampler
// vqhmm_code_sample_f32's draw: first k with u < run_k / total (run = the fp32 running sum of exp(lp) in index
// order, total its last value), else the last k with exp(lp[k]) > 0
__device__ __forceinline__ int ge_draw(const float* __restrict__ lp, int n, float total, float u) {
  float run = 0.f;
  int last = 0;
  for (int k = 0; k < n; ++k) {
    const float p = expf(lp[k]);
    run += p;
    if (p > 0.f) {
      last = k;
      if (u < run / total) return k;
    }
  }
  return last;
}

// LDS: [tot 33: pi, rows of A][sd S*D = exp(log_var / 2), taken in fp64 and rounded once]
__global__ __launch_bounds__(256) void gauss_sample_kernel(const float* __restrict__ log_pi,
                                                           const float* __restrict__ log_A,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ log_var,
                                                           const float* __restrict__ uni,
                                                           const float* __restrict__ nrm, int64_t N, int T, int S,
                                                           int D, int32_t* __restrict__ states,
                                                           float* __restrict__ x) {
  extern __shared__ float gs_smem[];
  float* tot = gs_smem;
  float* sd = gs_smem + 33;
  const int tid = threadIdx.x;
  if (tid < S + 1) {
    const float* lp = tid == 0 ? log_pi : log_A + (tid - 1) * S;
    float run = 0.f;
    for (int k = 0; k < S; ++k) run += expf(lp[k]);
    tot[tid] = run;
  }
  for (int k = tid; k < S * D; k += 256) sd[k] = (float)exp(0.5 * (double)log_var[k]);
  __syncthreads();
  const int64_t nq = (int64_t)blockIdx.x * 256 + tid;
  if (nq >= N) return;
  const float* u = uni + nq * (int64_t)T;
  int z = 0;
  for (int t = 0; t < T; ++t) {
    z = t == 0 ? ge_draw(log_pi, S, tot[0], u[0]) : ge_draw(log_A + z * S, S, tot[1 + z], u[t]);
    states[nq * T + t] = z;
    const int64_t o = (nq * T + t) * (int64_t)D;
    for (int d = 0; d < D; ++d) x[o + d] = fmaf(sd[z * D + d], nrm[o + d], mean[z * D + d]);
  }
}

struct GaussPlan {
  int nw;
  int64_t nblk;
  size_t lds_bytes;
  size_t off_part, bytes;
};

size_t ge_wave_bytes(int64_t S, int64_t D, int64_t SP) {
  return (size_t)(2 * S * D) * 8 +
         (size_t)((CE_CH * (ge_odd((int)D) + ge_odd((int)SP)) + (CE_CH + 1) * S + 1) & ~(int64_t)1) * 4;
}

GaussPlan gauss_plan(int64_t B, int64_t T, int64_t S, int64_t D) {
  GaussPlan p;
  int64_t SP = 1;
  while (SP < S) SP *= 2;
  const size_t sh = (size_t)((2 * S * D + S + D + 1) & ~(int64_t)1) * 4, pw = ge_wave_bytes(S, D, SP);
  // the waves per workgroup that put most waves on a CU (4 at most: one per SIMD at these register counts);
  // on a tie the fewest, which spreads a small batch over more CUs
  p.nw = 1;
  int64_t best = 0;
  for (int64_t nw = 1; nw <= GE_MAX_NW; ++nw) {
    const size_t wg = sh + (size_t)nw * pw;
    if (wg > GE_LDS_MAX) break;
    int64_t per_cu = (int64_t)(GE_LDS_CU / wg) * nw;
    per_cu = per_cu > 4 ? 4 : per_cu;
    if (per_cu > best) {
      best = per_cu;
      p.nw = (int)nw;
    }
  }
  p.nblk = cdiv(B, p.nw) < GE_MAX_WAVES / p.nw ? cdiv(B, p.nw) : GE_MAX_WAVES / p.nw;
  if (p.nblk < 1) p.nblk = 1;
  p.lds_bytes = sh + (size_t)p.nw * pw;
  p.off_part = r256((size_t)B * T * S * 4);
  p.bytes = p.off_part + (size_t)p.nblk * (2 * S * D + S * S + 2 * S) * 8;
  return p;
}

template <int SP, bool WT, bool MEM>
int gauss_go(const GaussArgs& a, const GaussPlan& p, int64_t M, hipStream_t s) {
  auto kern = gauss_estep_kernel<SP, WT, MEM>;
  // more than 64 KB of dynamic LDS has to be asked for, once per kernel
  static const hipError_t big_lds = hipFuncSetAttribute(
      reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GE_LDS_MAX);
  (void)big_lds;
  kern<<<dim3((unsigned)p.nblk, (unsigned)M), 64 * p.nw, p.lds_bytes, s>>>(a);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

template <bool WT, bool MEM>
int gauss_width(const GaussArgs& a, const GaussPlan& p, int64_t M, hipStream_t s) {
  if (a.S > 16) return gauss_go<32, WT, MEM>(a, p, M, s);
  if (a.S > 8) return gauss_go<16, WT, MEM>(a, p, M, s);
  if (a.S > 4) return gauss_go<8, WT, MEM>(a, p, M, s);
  if (a.S > 2) return gauss_go<4, WT, MEM>(a, p, M, s);
  if (a.S > 1) return gauss_go<2, WT, MEM>(a, p, M, s);
  return gauss_go<1, WT, MEM>(a, p, M, s);
}

// the decode and filter kernels' view of this file's emissions (hmm_gauss_decode_dev.h): the table is
// [mu S*D][iv S*D][c S]
struct GaussDiagEm {
  __host__ __device__ static int table_floats(int S, int D) { return 2 * S * D + S; }
  // 4 waves per SIMD up to SP = 16 (<= 128 VGPRs), 3 at SP = 32 (150 and 159)
  static int cu_waves(int SP) { return SP > 16 ? 12 : 16; }
  __device__ __forceinline__ static void table(const float* __restrict__ mean, const float* __restrict__ log_var,
                                               int S, int D, float* tb, int tid, int nthr) {
    ge_table(mean, log_var, S, D, tb, tb + S * D, tb + 2 * S * D, tid, nthr);
  }
  __device__ __forceinline__ static bool stage_x(const float* __restrict__ xg, int n, int D, int DS, int lane,
                                                 float* xbuf) {
    return ge_stage_x(xg, n, D, DS, lane, xbuf);
  }
  __device__ __forceinline__ static bool chunk_em(const float* xbuf, int DS, const float* tb, int S, int D, int n,
                                                  int lane, float* ebuf, int ES, float& Mv) {
    return ge_chunk_em(xbuf, DS, tb, tb + S * D, tb + 2 * S * D, S, D, n, lane, ebuf, ES, Mv);
  }
  __device__ __forceinline__ static float em_one(const float* xr, const float* tb, int j, int S, int D) {
    return ge_em(xr, tb + j * D, tb + S * D + j * D, tb[2 * S * D + j], D);
  }
};

}  // namespace

}  // namespace vqhmm

#include "hmm_gauss_decode_dev.h"

namespace vqhmm {

bool hmm_gauss_supported(int64_t S, int64_t D) { return S >= 1 && S <= 32 && D >= 1 && D <= 64; }
// the batch sizes the launches index (and whose workspace size fits size_t): the query and the launchers agree
static bool gauss_sizes_ok(int64_t B, int64_t T) {
  return B <= INT32_MAX && T <= (1 << 28) && (B == 0 || T <= (int64_t(1) << 40) / B);
}

size_t hmm_gauss_estep_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D) {
  if (!hmm_gauss_supported(S, D) || B < 0 || T < 0 || !gauss_sizes_ok(B, T)) return 0;
  return gauss_plan(B, T, S, D).bytes;
}

int launch_hmm_gauss_emission(const float* mean, const float* log_var, const float* x, const int64_t* lengths,
                              int64_t B, int64_t T, int64_t S, int64_t D, float* em, hipStream_t s) {
  if (!hmm_gauss_supported(S, D) || !gauss_sizes_ok(B, T)) return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) return VQHMM_OK;
  const size_t sh = (size_t)(2 * S * D + S) * 4, pw = (size_t)CE_CH * (ge_odd((int)D) + ge_odd((int)S)) * 4;
  int64_t nw = (int64_t)((GE_LDS_SOFT - sh) / pw);
  nw = nw < 1 ? 1 : nw > GE_MAX_NW ? GE_MAX_NW : nw;
  const int64_t nblk = cdiv(B * cdiv(T, CE_CH), nw);
  if (nblk > INT32_MAX) return VQHMM_EUNSUPPORTED;
  gauss_emission_kernel<<<(unsigned)nblk, 64 * (int)nw, sh + (size_t)nw * pw, s>>>(mean, log_var, x, lengths, B,
                                                                                 (int)T, (int)S, (int)D, em);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_gauss_estep(const float* log_pi, const float* log_A, const float* mean, const float* log_var,
                           const float* x, const int64_t* lengths, const float* shift, const float* weights,
                           int64_t B, int64_t T, int64_t S, int64_t D, double* pi_cnt, double* trans_cnt,
                           double* occ, double* m1, double* m2, float* loglik, float* gamma, void* ws,
                           hipStream_t s) {
  return launch_hmm_gauss_estep_batched(log_pi, log_A, mean, log_var, x, lengths, shift, weights, B, T, S, D, 1,
                                        pi_cnt, trans_cnt, occ, m1, m2, loglik, gamma, ws, s);
}

// M members: M single-model workspaces, each rounded up to 256 bytes
size_t hmm_gauss_estep_batched_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D, int64_t M) {
  if (!hmm_gauss_supported(S, D) || !hmm_code_members_supported(M) || B < 0 || T < 0 || !gauss_sizes_ok(B, T))
    return 0;
  return (size_t)M * r256(gauss_plan(B, T, S, D).bytes);
}

int launch_hmm_gauss_estep_batched(const float* log_pi, const float* log_A, const float* mean, const float* log_var,
                                   const float* x, const int64_t* lengths, const float* shift, const float* weights,
                                   int64_t B, int64_t T, int64_t S, int64_t D, int64_t M, double* pi_cnt,
                                   double* trans_cnt, double* occ, double* m1, double* m2, float* loglik,
                                   float* gamma, void* ws, hipStream_t s) {
  if (!hmm_gauss_supported(S, D) || !hmm_code_members_supported(M) || !gauss_sizes_ok(B, T))
    return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) {
    if (hipMemsetAsync(pi_cnt, 0, sizeof(double) * M * S, s) != hipSuccess ||
        hipMemsetAsync(trans_cnt, 0, sizeof(double) * M * S * S, s) != hipSuccess ||
        hipMemsetAsync(occ, 0, sizeof(double) * M * S, s) != hipSuccess ||
        hipMemsetAsync(m1, 0, sizeof(double) * M * S * D, s) != hipSuccess ||
        hipMemsetAsync(m2, 0, sizeof(double) * M * S * D, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    // length-0 sequences: loglik = NaN (all-ones words)
    if (B > 0 && loglik && hipMemsetAsync(loglik, 0xFF, sizeof(float) * M * B, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    return VQHMM_OK;
  }
  const GaussPlan p = gauss_plan(B, T, S, D);
  char* w = static_cast<char*>(ws);
  GaussArgs a;
  a.log_pi = log_pi; a.log_A = log_A; a.mean = mean; a.log_var = log_var; a.x = x; a.lengths = lengths;
  a.shift = shift; a.weights = weights;
  a.B = B; a.T = (int)T; a.S = (int)S; a.D = (int)D;
  a.alpha = reinterpret_cast<float*>(w);
  a.part = reinterpret_cast<double*>(w + p.off_part);
  a.loglik = loglik; a.gamma = gamma;
  a.mstride = r256(p.bytes);
  const int rc = weights ? (M > 1 ? gauss_width<true, true>(a, p, M, s) : gauss_width<true, false>(a, p, M, s))
                         : (M > 1 ? gauss_width<false, true>(a, p, M, s) : gauss_width<false, false>(a, p, M, s));
  if (rc) return rc;
  const int64_t NE = 2 * S * D + S * S + 2 * S;
  gauss_reduce_kernel<<<dim3((unsigned)cdiv(NE, GE_RK), (unsigned)M), GE_RK * GE_RP, 0, s>>>(
      a.part, a.mstride, (int)p.nblk, (int)S, (int)D, pi_cnt, trans_cnt, occ, m1, m2);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_gauss_sample(const float* log_pi, const float* log_A, const float* mean, const float* log_var,
                            const float* uniforms, const float* normals, int64_t N, int64_t T, int64_t S,
                            int64_t D, int32_t* states, float* x, hipStream_t s) {
  if (!hmm_gauss_supported(S, D) || T > (1 << 28) || cdiv(N, 256) > INT32_MAX) return VQHMM_EUNSUPPORTED;
  if (N == 0 || T == 0) return VQHMM_OK;
  gauss_sample_kernel<<<(unsigned)cdiv(N, 256), 256, (size_t)(33 + S * D) * 4, s>>>(
      log_pi, log_A, mean, log_var, uniforms, normals, N, (int)T, (int)S, (int)D, states, x);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

size_t hmm_gauss_viterbi_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t D) {
  if (!hmm_gauss_supported(S, D) || B < 0 || T < 0 || !gauss_sizes_ok(B, T)) return 0;
  return gd_viterbi_ws_bytes(B, T, S);
}

int launch_hmm_gauss_viterbi(const float* log_pi, const float* log_A, const float* mean, const float* log_var,
                             const float* x, const int64_t* lengths, int64_t B, int64_t T, int64_t S, int64_t D,
                             int32_t* path, float* score, void* ws, hipStream_t s) {
  if (!hmm_gauss_supported(S, D) || !gauss_sizes_ok(B, T)) return VQHMM_EUNSUPPORTED;
  if (B == 0) return VQHMM_OK;
  return gd_launch_viterbi<GaussDiagEm>(log_pi, log_A, mean, log_var, x, lengths, B, T, S, D, path, score, ws, s);
}

int launch_hmm_gauss_filter(const float* log_pi, const float* log_A, const float* mean, const float* log_var,
                            const float* x, const int64_t* lengths, const float* prev, int64_t B, int64_t T,
                            int64_t S, int64_t D, float* filt, float* last, float* loglik, hipStream_t s) {
  if (!hmm_gauss_supported(S, D) || !gauss_sizes_ok(B, T)) return VQHMM_EUNSUPPORTED;
  if (B == 0) return VQHMM_OK;
  return gd_launch_filter<GaussDiagEm>(log_pi, log_A, mean, log_var, x, lengths, prev, B, T, S, D, filt, last,
                                       loglik, s);
}

}  // namespace vqhmm
