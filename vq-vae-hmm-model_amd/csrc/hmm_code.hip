// Stationary HMM on VQ code indices: the fused Baum-Welch E-step and the ancestral sampler
// (pseudocode.txt:25-32, math.md:23-62 with M_t = M; contracts in include/vqhmm.h, fp64 restatement in
// tests/code_hmm_ref.py; DESIGN.md "HMM on code indices").
//
//   model   log_pi (S), log_A (S,S) rows = from-state, log_B (S,V) categorical emission over codes
//   E-step  pi_cnt = sum_b gamma_0, trans_cnt = sum_{b, 1<=t<L} xi_t, emit_cnt[s,v] = sum_{codes=v} gamma_t(s),
//           loglik (B), gamma (B,T,S) (optional)
//
// Lane map.  One sequence per wave at a time, lane j < S = state j (SP = S rounded up to a power of two is
// the compile-time width; lanes in [S, SP) carry zeros, lanes >= SP idle).  Every branch on a sequence's
// state (length, dead, bad code, a step leaving the fast range) is therefore wave-uniform.  A step's
// matrix-vector product needs no cross-lane reduction: lane j holds column j (forward) or row i (backward)
// of exp(log_A) in SP registers for the whole sequence and reads the vector's entries with v_readlane into
// scalar registers; only the normaliser is a reduction (DPP over the SP lanes).
//
// Forward (linear probabilities, normalised at every step, as hmm_pair.hip's filter):
//   y_t(j) = e_t(j) sum_i x_{t-1}(i) A(i,j),  c_t = sum_j y_t(j),  x_t = y_t / c_t,  loglik = sum_t ln c_t
// e_t = exp(log_B[:, code_t]) is a row of the (V,S) table a prologue launch builds in the workspace; a
// workgroup copies it to LDS when it fits (LDS tier) and stages each chunk's rows from L2 otherwise.  ln c_t:
// the product of four step masses (each within [2^-30, 2^30]) goes through one log2, added in fp64; the
// reciprocal's rounding (x_t sums to r c_t, not 1) is taken back out of loglik.  A step whose mass leaves
// [2^-30, 2^30] (underflow, an all-zero column set, NaN) is redone in natural log, max-shifted, from log_A /
// log_B in memory; a mass that is truly 0 ends the sequence: loglik = -inf, no contribution to any count.
// x_t is kept in the workspace (4 S bytes per position), the only per-position traffic besides the code.
//
// Backward.  b_{t-1}(i) = sum_j A(i,j) e_t(j) b_t(j) (renormalised every step; its scale cancels below),
//   gamma_{t-1}(i) = x_{t-1}(i) b_{t-1}(i) / Z,   xi_t(i,j) = x_{t-1}(i) A(i,j) e_t(j) b_t(j) / Z,
//   Z = sum_i x_{t-1}(i) b_{t-1}(i)
// so the products A(i,j) w(j) of the beta step are the xi row of lane i: trans_cnt accumulates in SP
// registers (fp32 within a 64-step chunk, fp64 across chunks) and xi never exists off chip.
// emit_cnt: lane j adds gamma_t(j) to bin (code_t, j) of the wave's private fp64 slab (LDS, or the
// workgroup's region of the workspace in the L2 tier); one sequence per wave means no two adds of a step
// share a bin, so there is no atomic anywhere.
//
// Reduction.  Sequences are assigned statically (wave w of workgroup g takes b = g NW + w, then strides by
// the grid), a workgroup sums its waves' slabs in wave order into its partial (workspace), and a second
// launch sums the partials in fp64 in a fixed order (code_reduce_kernel): the same bits run to run.
//
// Members.  blockIdx.y is the member of a stack of M models that share codes and lengths (the batched
// entry; the single-model entry is M = 1): a member has its own parameter slices, exp(log_B)^T table, x rows,
// partials and outputs, `mstride` workspace bytes and one output block after the previous member's, and runs
// exactly the single model's plan, so its bits are the single-model call's.  Sequence b enters member m's counts
// with the weight w[m, b] (1 without weights): one fp64 fma where a contribution is already added in fp64 (the
// slab bin, the per-chunk flush of the transition registers, the t = 0 posterior), so w = 1 keeps the
// unweighted bits.  Member and weight are wave-uniform (blockIdx.y, and a load at the wave's own b).
//
// Addressing.  codes are read at min(t, T - 1) of the wave's own row, parameters only at (i, j) < S and
// validated codes, the workspace only inside its own sequence's rows.
#include "hmm_code_dev.h"  // the lane helpers, the fast step's range and the exp(log_B)^T prologue

namespace vqhmm {

namespace {

constexpr int CE_NW = 4;                            // LDS tier: waves (private slabs) per workgroup
constexpr size_t CE_LDS_MAX = 156 * 1024;           // of the CU's 160 KB
constexpr int64_t CE_MAX_WG = 512;                  // LDS tier: workgroups (partials)
constexpr size_t CE_PART_CAP = size_t(64) << 20;    // L2 tier: bytes of partials

struct CodeArgs {
  const float* log_pi;
  const float* log_A;
  const float* log_B;
  const int32_t* codes;
  const int64_t* lengths;
  int64_t B;
  int T, S, V;
  const float* weights;  // (M, B), nullable (= all 1)
  const float* Bt;  // (V, S) exp(log_B)^T
  float* alpha;     // (B, T, S) x_t
  double* part;     // [gridDim.x][V*S (v-major) + S*S + S]
  float* loglik;    // nullable
  float* gamma;     // nullable
  size_t mstride;   // bytes from a member's Bt / alpha / part to the next member's
};

// out = sum over the partials, in a fixed order: 16 elements per workgroup, thread (py, kx) adds partials
// py, py + 16, .. of element kx in index order (16 independent loads in flight per element instead of one
// serial walk), then the 16 sums are added in py order; the emission block leaves transposed to (S, V)
constexpr int CE_RK = 16, CE_RP = 16;
__global__ __launch_bounds__(CE_RK * CE_RP) void code_reduce_kernel(const double* __restrict__ part, size_t mstride,
                                                                    int np, int S, int V,
                                                                    double* __restrict__ pi_cnt,
                                                                    double* __restrict__ trans_cnt,
                                                                    double* __restrict__ emit_cnt) {
  __shared__ double red[CE_RP][CE_RK];
  const int64_t NV = (int64_t)S * V, NE = NV + (int64_t)S * S + S;
  const int kx = threadIdx.x % CE_RK, py = threadIdx.x / CE_RK;
  const int64_t k = (int64_t)blockIdx.x * CE_RK + kx;
  const int64_t mem = blockIdx.y;  // member: its own partials (mstride bytes apart) and output blocks
  part = reinterpret_cast<const double*>(reinterpret_cast<const char*>(part) + mem * mstride);
  pi_cnt += mem * S;
  trans_cnt += mem * S * S;
  emit_cnt += mem * NV;
  double acc = 0.0;
  if (k < NE) {
#pragma unroll 4
    for (int p = py; p < np; p += CE_RP) acc += part[(int64_t)p * NE + k];
  }
  red[py][kx] = acc;
  __syncthreads();
  if (py != 0 || k >= NE) return;
  acc = 0.0;
#pragma unroll
  for (int q = 0; q < CE_RP; ++q) acc += red[q][kx];
  if (k < NV) {
    const int64_t v = k / S, s = k - v * S;
    emit_cnt[s * V + v] = acc;
  } else if (k < NV + (int64_t)S * S) {
    trans_cnt[k - NV] = acc;
  } else {
    pi_cnt[k - NV - (int64_t)S * S] = acc;
  }
}

// member m's view of the arguments (m = 0 changes nothing)
__device__ __forceinline__ CodeArgs code_member(CodeArgs a, int64_t m) {
  a.log_pi += m * a.S;
  a.log_A += m * a.S * a.S;
  a.log_B += m * (int64_t)a.S * a.V;
  if (a.weights) a.weights += m * a.B;
  a.Bt = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.Bt) + m * a.mstride);
  a.alpha = reinterpret_cast<float*>(reinterpret_cast<char*>(a.alpha) + m * a.mstride);
  a.part = reinterpret_cast<double*>(reinterpret_cast<char*>(a.part) + m * a.mstride);
  if (a.loglik) a.loglik += m * a.B;
  if (a.gamma) a.gamma += m * a.B * (int64_t)a.T * a.S;
  return a;
}

// WT: the call has weights.  Without them the weight is the constant 1 and every weighted add below is the plain
// fp64 add again, at no cost in registers.  MEM: the launch has more than one member.  With one, the arguments
// stay kernel arguments: offset pointers are computed values that the register allocator has to keep (at SP = 32
// in spilled scalar registers, measured at 1 % of the single-model call, profiles/code_ensemble).
template <int SP, bool LDS_T, bool WT, bool MEM>
__global__ __launch_bounds__(256) void code_estep_kernel(const CodeArgs a0) {
  extern __shared__ double ce_smem[];
  const CodeArgs a = MEM ? code_member(a0, blockIdx.y) : a0;
  const int S = a.S, V = a.V, T = a.T;
  const int NV = S * V, NT = S * S + S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int j = lane;
  const bool act = j < S;
  // LDS: [slab nw x NV doubles (LDS tier)] [tr nw x NT doubles] [bt NV floats (LDS tier)]
  //      [abuf nw x CH*S floats] [ebuf nw x CH*SP floats (L2 tier)]
  double* tr_all = ce_smem + (LDS_T ? (size_t)nw * NV : 0);
  float* fl = reinterpret_cast<float*>(tr_all + (size_t)nw * NT);
  const float* bt = fl;
  float* abuf = fl + (LDS_T ? NV : 0) + wave * (CE_CH * S);
  float* ebuf = fl + (LDS_T ? NV : 0) + nw * (CE_CH * S) + wave * (CE_CH * SP);
  double* part = a.part + (int64_t)blockIdx.x * (NV + NT);
  if constexpr (LDS_T) {
    for (int k = tid; k < NV; k += blockDim.x) fl[k] = a.Bt[k];
    for (int k = tid; k < nw * NV; k += blockDim.x) ce_smem[k] = 0.0;
    __syncthreads();
  } else {
    for (int k = tid; k < NV; k += blockDim.x) part[k] = 0.0;
    __threadfence();
    __syncthreads();
  }
  double* slab = LDS_T ? ce_smem + (size_t)wave * NV : part;

  double tc64[SP];
#pragma unroll
  for (int q = 0; q < SP; ++q) tc64[q] = 0.0;
  double pc64 = 0.0;

  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < a.B; b += (int64_t)gridDim.x * nw) {
    const int64_t Lr = a.lengths[b];
    const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
    const int32_t* cb = a.codes + b * T;
    float* al = a.alpha + b * (int64_t)T * S;
    float* gm_out = a.gamma ? a.gamma + b * (int64_t)T * S : nullptr;
    if (gm_out)
      for (int64_t e = (int64_t)L * S + lane; e < (int64_t)T * S; e += 64) gm_out[e] = 0.f;
    if (L == 0) {
      if (a.loglik && lane == 0) a.loglik[b] = ce_nan();
      continue;
    }

    // ------------------------------------------------------------------ forward
    float x = 0.f;
    double Sll = 0.0;
    int status = 0;  // 1: impossible (mass 0), 2: a code outside [0, V) inside the length
    {
      float Acol[SP];
#pragma unroll
      for (int i = 0; i < SP; ++i) Acol[i] = (act && i < S) ? __expf(a.log_A[i * S + j]) : 0.f;
      float P = 1.f, D = 0.f;
      for (int t0 = 0; t0 < L && status == 0; t0 += CE_CH) {
        const int n = min(CE_CH, L - t0);
        const int32_t cv = cb[min(t0 + lane, T - 1)];
        if (__builtin_amdgcn_ballot_w64(lane < n && (cv < 0 || cv >= V)) != 0) {
          status = 2;
          break;
        }
        const int cvs = lane < n ? cv : 0;
        if constexpr (!LDS_T) {
          // the chunk's emission rows through L2, all in flight together
#pragma unroll
          for (int k = 0; k < SP; ++k) {
            const int idx = k * 64 + lane, s = idx / SP, jj = idx - s * SP;
            const int cs = __shfl(cvs, s);
            ebuf[idx] = (jj < S && s < n) ? a.Bt[(int64_t)cs * S + jj] : 0.f;
          }
          asm volatile("" ::: "memory");
        }
        // step s's emission row, for the lane's state (lanes past n hold code 0, so any s < 64 is a safe read)
        auto emis = [&](int s) {
          const int code = __builtin_amdgcn_readlane(cvs, s);
          return LDS_T ? (act ? bt[code * S + j] : 0.f) : ebuf[s * SP + (j & (SP - 1))];
        };
        float e_nx = emis(0);
        for (int s = 0; s < n; ++s) {
          const int t = t0 + s;
          const int code = __builtin_amdgcn_readlane(cvs, s);
          const float e = e_nx;
          e_nx = emis(min(s + 1, CE_CH - 1));  // one step ahead of the chain
          if (t == 0) {
            const float ly = act ? a.log_pi[j] + a.log_B[(int64_t)j * V + code] : CE_NEG_INF;
            const float M = ce_red<SP>(ly, CeMax{});
            if (ce_uni(M) == CE_NEG_INF) {
              status = 1;
              break;
            }
            const float ex = ly == CE_NEG_INF ? 0.f : expf(ly - M);
            const float st = ce_red<SP>(ex, CeAdd{});
            x = ex / st;
            Sll = (double)M + (double)logf(st);
          } else {
            float u0 = 0.f, u1 = 0.f;
#pragma unroll
            for (int i = 0; i < SP; i += 2) {
              u0 = fmaf(Acol[i], ce_lane(x, i), u0);
              if (i + 1 < SP) u1 = fmaf(Acol[i + 1], ce_lane(x, i + 1), u1);
            }
            const float y = (u0 + u1) * e;
            const float c = ce_red<SP>(j < SP ? y : 0.f, CeAdd{});
            const float cu = ce_uni(c);
            if (cu >= CE_LO && cu <= CE_HI) {
              const float r = __builtin_amdgcn_rcpf(c);
              x = y * r;
              P *= c;
              D += fmaf(r, c, -1.f);
            } else {
              // rare path: the step in natural log, max-shifted, from the tables in memory
              const float lx = logf(x);
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
              const float lb = act ? a.log_B[(int64_t)j * V + code] : CE_NEG_INF;
              const float ly = (m == CE_NEG_INF || lb == CE_NEG_INF) ? CE_NEG_INF : (m + logf(sm)) + lb;
              const float M = ce_red<SP>(ly, CeMax{});
              if (ce_uni(M) == CE_NEG_INF) {
                status = 1;
                break;
              }
              const float ex = ly == CE_NEG_INF ? 0.f : expf(ly - M);
              const float st = ce_red<SP>(ex, CeAdd{});
              x = ex / st;
              Sll += (double)M + (double)logf(st);
            }
            if ((s & 3) == 3) {
              asm volatile("");  // a real (scalar) branch: the log and the fp64 add run every fourth step only
              Sll += (double)__builtin_amdgcn_logf(P) * CE_LN2;
              P = 1.f;
            }
          }
          if (act) al[(int64_t)t * S + j] = x;
        }
        Sll += (double)__builtin_amdgcn_logf(P) * CE_LN2;
        P = 1.f;
      }
      Sll -= (double)D;
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
      {
        // t = L - 1: gamma = x_{L-1}
        const int code = ce_uni(cb[L - 1]);
        if (act) {
          double* bin = slab + ((int64_t)code * S + j);
          *bin = fma(wt, (double)x, *bin);
          if (gm_out) gm_out[(int64_t)(L - 1) * S + j] = x;
          if (L == 1) pc64 = fma(wt, (double)x, pc64);
        }
      }
      for (int t0 = ((L - 1) / CE_CH) * CE_CH; t0 >= 0; t0 -= CE_CH) {
        const int n = min(CE_CH, L - t0);
        const int cvs = lane < n ? cb[min(t0 + lane, T - 1)] : 0;                      // code_t
        const int cvm = (lane < n && t0 + lane >= 1) ? cb[min(t0 + lane - 1, T - 1)] : 0;  // code_{t-1}
        // x rows t0 - 1 .. t0 + n - 2 (row s <-> time t0 + s - 1), one contiguous span
        for (int k = lane; k < n * S; k += 64) {
          const int64_t o = (int64_t)(t0 - 1) * S + k;
          abuf[k] = o >= 0 ? al[o] : 0.f;
        }
        if constexpr (!LDS_T) {
#pragma unroll
          for (int k = 0; k < SP; ++k) {
            const int idx = k * 64 + lane, s = idx / SP, jj = idx - s * SP;
            const int cs = __shfl(cvs, s);
            ebuf[idx] = (jj < S && s < n) ? a.Bt[(int64_t)cs * S + jj] : 0.f;
          }
        }
        asm volatile("" ::: "memory");  // the wave's own LDS stores above, read across lanes below
        auto emis = [&](int s) {
          const int code = __builtin_amdgcn_readlane(cvs, s);
          return LDS_T ? (act ? bt[code * S + j] : 0.f) : ebuf[s * SP + (j & (SP - 1))];
        };
        float e_nx = emis(n - 1), xp_nx = act ? abuf[(n - 1) * S + j] : 0.f;
        for (int s = n - 1; s >= 0; --s) {
          const int t = t0 + s;
          if (t == 0) break;
          const int code = __builtin_amdgcn_readlane(cvs, s);
          const int codem = __builtin_amdgcn_readlane(cvm, s);
          // this step's operands were read a step ago; the bin this step adds to is read now, used last
          const float e = e_nx, xp = xp_nx;
          const int sn = max(s - 1, 0);
          e_nx = emis(sn);
          xp_nx = act ? abuf[sn * S + j] : 0.f;
          double* bin = slab + ((int64_t)codem * S + (act ? j : 0));
          const double bin0 = act ? *bin : 0.0;
          const float w = j < SP ? e * bn : 0.f;
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
            const float lbe = act ? a.log_B[(int64_t)j * V + code] : CE_NEG_INF;
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
          if (act) {
            *bin = fma(wt, (double)gm, bin0);
            if (gm_out) gm_out[(int64_t)(t - 1) * S + j] = gm;
            if (t == 1) pc64 = fma(wt, (double)gm, pc64);
          }
        }
#pragma unroll
        for (int q = 0; q < SP; ++q) {
          tc64[q] = fma(wt, (double)tc[q], tc64[q]);
          tc[q] = 0.f;
        }
      }
    }
  }

  // the workgroup's partial: its waves' slabs in wave order
  double* tr = tr_all + (size_t)wave * NT;
  if (act) {
#pragma unroll
    for (int q = 0; q < SP; ++q)
      if (q < S) tr[j * S + q] = tc64[q];
    tr[S * S + j] = pc64;
  }
  __syncthreads();
  if constexpr (LDS_T) {
    for (int k = tid; k < NV; k += blockDim.x) {
      double acc = 0.0;
      for (int w = 0; w < nw; ++w) acc += ce_smem[(size_t)w * NV + k];
      part[k] = acc;
    }
  }
  for (int k = tid; k < NT; k += blockDim.x) {
    double acc = 0.0;
    for (int w = 0; w < nw; ++w) acc += tr_all[(size_t)w * NT + k];
    part[NV + k] = acc;
  }
}

// ---------------------------------------------------------------------------- sampler
// first k with u < run_k / total (run = the fp32 running sum of exp(lp) in index order, total its last
// value), else the last k with exp(lp[k]) > 0
__device__ __forceinline__ int ce_draw(const float* __restrict__ lp, int n, float total, float u) {
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

__global__ __launch_bounds__(256) void code_sample_kernel(const float* __restrict__ log_pi,
                                                          const float* __restrict__ log_A,
                                                          const float* __restrict__ log_B,
                                                          const float* __restrict__ uni, int64_t N, int T, int S, int V,
                                                          int32_t* __restrict__ states, int32_t* __restrict__ codes) {
  __shared__ float tot[65];  // row totals: [0] pi, [1, S] rows of A, [33, 33 + S) rows of B
  const int tid = threadIdx.x;
  if (tid < 2 * S + 1) {
    const float* lp = tid == 0 ? log_pi : tid <= S ? log_A + (tid - 1) * S : log_B + (int64_t)(tid - 1 - S) * V;
    const int n = tid <= S ? S : V;
    float run = 0.f;
    for (int k = 0; k < n; ++k) run += expf(lp[k]);
    tot[tid == 0 ? 0 : tid <= S ? tid : 33 + (tid - 1 - S)] = run;
  }
  __syncthreads();
  const int64_t nq = (int64_t)blockIdx.x * 256 + tid;
  if (nq >= N) return;
  const float* u = uni + nq * (int64_t)T * 2;
  int z = 0;
  for (int t = 0; t < T; ++t) {
    z = t == 0 ? ce_draw(log_pi, S, tot[0], u[0]) : ce_draw(log_A + z * S, S, tot[1 + z], u[2 * t]);
    const int c = ce_draw(log_B + (int64_t)z * V, V, tot[33 + z], u[2 * t + 1]);
    states[nq * T + t] = z;
    codes[nq * T + t] = c;
  }
}

struct CodePlan {
  bool lds;
  int nw;
  int64_t nblk;
  size_t lds_bytes;
  size_t off_bt, off_part, bytes;
};

CodePlan code_plan(int64_t B, int64_t T, int64_t S, int64_t V) {
  CodePlan p;
  int64_t SP = 1;
  while (SP < S) SP *= 2;
  const size_t NV = (size_t)S * V, NT = (size_t)S * S + S;
  const size_t lds_t = CE_NW * (NV + NT) * 8 + NV * 4 + CE_NW * CE_CH * S * 4;
  p.lds = lds_t <= CE_LDS_MAX;
  if (p.lds) {
    p.nw = CE_NW;
    p.nblk = cdiv(B, CE_NW) < CE_MAX_WG ? cdiv(B, CE_NW) : CE_MAX_WG;
    p.lds_bytes = lds_t;
  } else {
    p.nw = 1;
    int64_t cap = (int64_t)(CE_PART_CAP / ((NV + NT) * 8));
    cap = cap < 1 ? 1 : cap > 1024 ? 1024 : cap;
    p.nblk = B < cap ? B : cap;
    p.lds_bytes = NT * 8 + CE_CH * S * 4 + CE_CH * SP * 4;
  }
  if (p.nblk < 1) p.nblk = 1;
  p.off_bt = r256((size_t)B * T * S * 4);
  p.off_part = p.off_bt + r256(NV * 4);
  p.bytes = p.off_part + (size_t)p.nblk * (NV + NT) * 8;
  return p;
}

template <int SP, bool WT, bool MEM>
int estep_go(const CodeArgs& a, const CodePlan& p, int64_t M, hipStream_t s) {
  const dim3 grid((unsigned)p.nblk, (unsigned)M);
  if (p.lds) {
    auto kern = code_estep_kernel<SP, true, WT, MEM>;
    // more than 64 KB of dynamic LDS has to be asked for, once per kernel (the tier's limit covers every launch)
    static const hipError_t big_lds = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CE_LDS_MAX);
    (void)big_lds;
    kern<<<grid, 64 * p.nw, p.lds_bytes, s>>>(a);
  } else {
    code_estep_kernel<SP, false, WT, MEM><<<grid, 64, p.lds_bytes, s>>>(a);
  }
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

template <bool WT, bool MEM>
int estep_width(const CodeArgs& a, const CodePlan& p, int64_t M, hipStream_t s) {
  if (a.S > 16) return estep_go<32, WT, MEM>(a, p, M, s);
  if (a.S > 8) return estep_go<16, WT, MEM>(a, p, M, s);
  if (a.S > 4) return estep_go<8, WT, MEM>(a, p, M, s);
  if (a.S > 2) return estep_go<4, WT, MEM>(a, p, M, s);
  if (a.S > 1) return estep_go<2, WT, MEM>(a, p, M, s);
  return estep_go<1, WT, MEM>(a, p, M, s);
}

}  // namespace

bool hmm_code_supported(int64_t S, int64_t V) { return S >= 1 && S <= 32 && V >= 1 && V <= 65536; }
bool hmm_code_members_supported(int64_t M) { return M >= 1 && M <= 65535; }  // the member axis is gridDim.y

size_t hmm_code_estep_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t V) {
  if (!hmm_code_supported(S, V) || B < 0 || T < 0) return 0;
  return code_plan(B, T, S, V).bytes;
}

// M members: M single-model workspaces, each rounded up to 256 bytes
size_t hmm_code_estep_batched_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t V, int64_t M) {
  if (!hmm_code_supported(S, V) || !hmm_code_members_supported(M) || B < 0 || T < 0) return 0;
  return (size_t)M * r256(code_plan(B, T, S, V).bytes);
}

int launch_hmm_code_estep(const float* log_pi, const float* log_A, const float* log_B, const int32_t* codes,
                          const int64_t* lengths, int64_t B, int64_t T, int64_t S, int64_t V, double* pi_cnt,
                          double* trans_cnt, double* emit_cnt, float* loglik, float* gamma, void* ws, hipStream_t s) {
  return launch_hmm_code_estep_batched(log_pi, log_A, log_B, codes, lengths, nullptr, B, T, S, V, 1, pi_cnt,
                                       trans_cnt, emit_cnt, loglik, gamma, ws, s);
}

int launch_hmm_code_estep_batched(const float* log_pi, const float* log_A, const float* log_B, const int32_t* codes,
                                  const int64_t* lengths, const float* weights, int64_t B, int64_t T, int64_t S,
                                  int64_t V, int64_t M, double* pi_cnt, double* trans_cnt, double* emit_cnt,
                                  float* loglik, float* gamma, void* ws, hipStream_t s) {
  if (!hmm_code_supported(S, V) || !hmm_code_members_supported(M) || T > (1 << 28) || B > INT32_MAX)
    return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) {
    if (hipMemsetAsync(pi_cnt, 0, sizeof(double) * M * S, s) != hipSuccess ||
        hipMemsetAsync(trans_cnt, 0, sizeof(double) * M * S * S, s) != hipSuccess ||
        hipMemsetAsync(emit_cnt, 0, sizeof(double) * M * S * V, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    // length-0 sequences: loglik = NaN (all-ones words)
    if (B > 0 && loglik && hipMemsetAsync(loglik, 0xFF, sizeof(float) * M * B, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    return VQHMM_OK;
  }
  const CodePlan p = code_plan(B, T, S, V);
  char* w = static_cast<char*>(ws);
  CodeArgs a;
  a.log_pi = log_pi; a.log_A = log_A; a.log_B = log_B; a.codes = codes; a.lengths = lengths;
  a.weights = weights;
  a.B = B; a.T = (int)T; a.S = (int)S; a.V = (int)V;
  a.alpha = reinterpret_cast<float*>(w);
  float* Bt = reinterpret_cast<float*>(w + p.off_bt);
  a.Bt = Bt;
  a.part = reinterpret_cast<double*>(w + p.off_part);
  a.loglik = loglik; a.gamma = gamma;
  a.mstride = r256(p.bytes);
  code_bt_kernel<<<dim3((unsigned)cdiv(S * V, 256), (unsigned)M), 256, 0, s>>>(log_B, (int)S, (int)V, Bt, S * V,
                                                                               (int64_t)(a.mstride / 4));
  VQHMM_LAUNCH_CHECK();
  const int rc = weights ? (M > 1 ? estep_width<true, true>(a, p, M, s) : estep_width<true, false>(a, p, M, s))
                         : (M > 1 ? estep_width<false, true>(a, p, M, s) : estep_width<false, false>(a, p, M, s));
  if (rc) return rc;
  const int64_t NE = S * V + S * S + S;
  code_reduce_kernel<<<dim3((unsigned)cdiv(NE, CE_RK), (unsigned)M), CE_RK * CE_RP, 0, s>>>(
      a.part, a.mstride, (int)p.nblk, (int)S, (int)V, pi_cnt, trans_cnt, emit_cnt);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_hmm_code_sample(const float* log_pi, const float* log_A, const float* log_B, const float* uniforms,
                           int64_t N, int64_t T, int64_t S, int64_t V, int32_t* states, int32_t* codes,
                           hipStream_t s) {
  if (!hmm_code_supported(S, V) || T > (1 << 28) || cdiv(N, 256) > INT32_MAX) return VQHMM_EUNSUPPORTED;
  if (N == 0 || T == 0) return VQHMM_OK;
  code_sample_kernel<<<(unsigned)cdiv(N, 256), 256, 0, s>>>(log_pi, log_A, log_B, uniforms, N, (int)T, (int)S, (int)V,
                                                           states, codes);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

}  // namespace vqhmm
