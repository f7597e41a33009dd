// The fused Viterbi decode and the streaming causal filter of the Gaussian HMMs on continuous observations
// (contracts in include/vqhmm.h; restatements in tests/gauss_decode_ref.py; DESIGN.md "Gaussian decode and
// filter").  Included by hmm_gauss.hip and hmm_gauss_full.hip after their emission helpers: the kernels are
// templates over EM, the including file's emission policy
//
//   EM::table_floats(S, D)                      floats of the workgroup's shared emission table
//   EM::cu_waves(SP)                            waves per CU the kernels' registers allow at width SP
//   EM::table(mean, par, S, D, tb, tid, nthr)   builds it (par = log_var or prec_chol); the caller synchronises
//   EM::stage_x / EM::chunk_em / EM::em_one     the file's stage-x helper, its lane = time emission pass and its
//                                               one emission function, on that table
//
// so the emissions are evaluated by the file's one function (ge_em / gf_em) under the file's build flags, and are
// the bits its emission entry writes.
//
// Lane map.  hmm_code_decode.hip's: one sequence per wave at a time, lane j < S = state j, SP = S rounded up to
// a power of two the compile-time width, column j of the transition matrix in SP registers for the whole
// sequence, the previous step's vector read with v_readlane, every branch on a sequence's state wave-uniform.
//
// Per chunk of 64 steps.  The E-step's staging: the chunk's rows of x go to the wave's LDS buffer, the lane =
// time pass writes em[t, s] into the wave's emission buffer (odd row stride: conflict-free both ways), and the
// chain reads its row one step ahead (the filter) or a block of VB steps ahead (Viterbi).  LDS: [table] [per
// wave: xbuf 64 (D|1) | ebuf 64 (SP|1)]: no fp64 slabs, no forward vectors.
//
// Viterbi.  hmm_code_decode.hip's step on the raw log emissions (no max shift): d_0[j] = log_pi[j] + em[0,j],
// d_t[j] = (max_i (d_{t-1}[i] + log_A[i,j])) + em[t,j] in fp32 in this order, i ascending with a strict > (the
// compare tree selects the same candidate), one backpointer byte per state and step packed four steps to a word
// ([b][ceil(T/4)][SP] words), the backtrace from 16 registers per lane with v_readlane at the scalar state.
//
// Filter.  The E-step's forward: e_t = exp(em_t - max_s em_t) written by the lane = time pass, the maxima added
// to the fp64 log-likelihood sum, linear probabilities normalised at every step, the product of four step
// masses through one log2 into fp64, a step whose mass leaves [2^-30, 2^30] redone max-shifted in natural log
// from the tables in memory, a mass that is truly 0 ends the sequence.  With prev, step 0 is an ordinary step
// from prev / sum(prev).  The steps before the first row whose x or emission is not finite still run.
//
// Addressing.  x is read only at rows t < L of the wave's own sequence, parameters only inside their arrays,
// the backpointer words only inside the sequence's own rows; offsets are 64-bit.
#pragma once
#include "hmm_code_dev.h"

namespace vqhmm {

namespace {

constexpr int GD_MAX_NW = 4;                  // waves per workgroup, at most
constexpr size_t GD_LDS_CU = 160 * 1024;      // a CU's LDS
constexpr size_t GD_LDS_SOFT = 64 * 1024;     // more dynamic LDS than this has to be asked for
constexpr size_t GD_LDS_MAX = 156 * 1024;
constexpr int64_t GD_MAX_WAVES = 2048;        // waves of the grid; further sequences by striding
constexpr int GD_VB = 8;                      // Viterbi: steps per unrolled block (a multiple of 4, divides CE_CH)

struct GdArgs {
  const float* log_pi;
  const float* log_A;
  const float* mean;
  const float* par;  // log_var (S,D) or prec_chol (S,D,D)
  const float* x;
  const int64_t* lengths;
  int64_t B;
  int T, S, D;
  // viterbi
  uint32_t* bp;  // [B][ceil(T / 4)][SP]
  int32_t* path;
  float* score;
  // filter
  const float* prev;  // nullable
  float* filt;        // nullable
  float* last;        // nullable
  float* loglik;      // nullable
};

__device__ __forceinline__ bool gd_nonfinite(float v) {
  return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u;
}

__global__ __launch_bounds__(256) void gauss_dec_fill_kernel(float* __restrict__ p, int64_t n, float v) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) p[k] = v;
}

// ---------------------------------------------------------------------------- viterbi
template <int SP, class EM>
__global__ __launch_bounds__(256) void gauss_viterbi_kernel(const GdArgs a) {
  extern __shared__ float gd_smem[];
  constexpr int ES = SP | 1;
  const int S = a.S, D = a.D, T = a.T, DS = D | 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int j = lane, jj = j & (SP - 1);
  const bool act = j < S;
  float* tb = gd_smem;
  float* xbuf = tb + EM::table_floats(S, D) + wave * (CE_CH * (DS + ES));
  float* ebuf = xbuf + CE_CH * DS;
  EM::table(a.mean, a.par, S, D, tb, tid, (int)blockDim.x);
  __syncthreads();
  const int64_t T4 = (T + 3) / 4;

  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < a.B; b += (int64_t)gridDim.x * nw) {
    const int64_t Lr = a.lengths[b];
    const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
    const float* xs = a.x + b * (int64_t)T * D;
    int32_t* P = a.path + b * T;
    uint32_t* bp = a.bp + b * T4 * SP;
    for (int t = L + lane; t < T; t += 64) P[t] = -1;
    if (L == 0) {
      if (lane == 0) a.score[b] = CE_NEG_INF;
      continue;
    }

    // ------------------------------------------------------------------ forward
    float Acol[SP];
#pragma unroll
    for (int i = 0; i < SP; ++i) Acol[i] = (act && i < S) ? a.log_A[i * S + j] : CE_NEG_INF;
    float d = CE_NEG_INF;
    uint32_t bpw = 0;
    bool bad = false;
    for (int t0 = 0; t0 < L; t0 += CE_CH) {
      const int n = min(CE_CH, L - t0);
      asm volatile("" ::: "memory");
      const bool badx = EM::stage_x(xs + (int64_t)t0 * D, n, D, DS, lane, xbuf);
      asm volatile("" ::: "memory");
      float Mv;
      const bool bade = EM::chunk_em(xbuf, DS, tb, S, D, n, lane, ebuf, ES, Mv);
      asm volatile("" ::: "memory");  // the wave's own LDS stores, read across lanes by the steps
      if (badx || bade) {
        bad = true;
        break;
      }
      // step s's emission for the lane's state (the columns [S, SP) of a row are never written: a select)
      auto emis = [&](int s) {
        const float r = ebuf[s * ES + jj];
        return act ? r : 0.f;
      };
      // one step t >= 1 with emission e; sh = 8 (t & 3), the byte of the backpointer word
      auto vstep = [&](float e, int sh) {
        float v[SP];
        int g[SP];
#pragma unroll
        for (int i = 0; i < SP; ++i) {
          v[i] = ce_lane(d, i) + Acol[i];
          g[i] = i;
        }
        // hmm_code_decode.hip's tree: the higher-index half wins only by a strict >, which selects the
        // candidate of "i ascending, strict >"
#pragma unroll
        for (int w = 1; w < SP; w *= 2) {
#pragma unroll
          for (int i = 0; i < SP; i += 2 * w) {
            const bool gt = v[i + w] > v[i];
            v[i] = gt ? v[i + w] : v[i];
            g[i] = gt ? g[i + w] : g[i];
          }
        }
        d = v[0] + e;
        bpw |= (uint32_t)g[0] << sh;
      };
      auto flush = [&](int t) {
        if (j < SP) bp[(int64_t)(t >> 2) * SP + j] = bpw;
        bpw = 0;
      };
      // any step, every case tested: the sequence's first steps and the chunk's last ones
      auto any_step = [&](int s) {
        const int t = t0 + s;
        const float e = emis(s);
        if (t == 0) d = act ? a.log_pi[j] + e : CE_NEG_INF;
        else vstep(e, 8 * (t & 3));
        if ((t & 3) == 3 || t == L - 1) flush(t);
      };
      int s = 0;
      if (t0 == 0)
        for (; s < min(n, GD_VB); ++s) any_step(s);
      // whole blocks of VB steps (s a multiple of VB): the block's emissions are read together, a block ahead
      // of the chain
      if (SP <= 16 && s + GD_VB <= n) {  // (SP = 32: eight unrolled steps cost a wave per SIMD in registers)
        float E[GD_VB];
#pragma unroll
        for (int u = 0; u < GD_VB; ++u) E[u] = emis(s + u);
        for (; s + GD_VB <= n; s += GD_VB) {
          float En[GD_VB] = {};
          if (s + 2 * GD_VB <= n) {
#pragma unroll
            for (int u = 0; u < GD_VB; ++u) En[u] = emis(s + GD_VB + u);
          }
#pragma unroll
          for (int u = 0; u < GD_VB; ++u) {
            vstep(E[u], 8 * (u & 3));
            if ((u & 3) == 3) flush(t0 + s + u);
          }
#pragma unroll
          for (int u = 0; u < GD_VB; ++u) E[u] = En[u];
        }
      }
      for (; s < n; ++s) any_step(s);
    }
    if (bad) {
      for (int t = lane; t < L; t += 64) P[t] = -1;
      if (lane == 0) a.score[b] = ce_nan();
      continue;
    }

    // last state: the first argmax of d_{L-1}
    const float M = ce_uni(ce_red<SP>(d, CeMax{}));
    const uint64_t hit = __builtin_amdgcn_ballot_w64(act && d == M);
    int state = hit ? (int)__builtin_ctzll(hit) : 0;
    if (lane == 0) a.score[b] = M;

    // ----------------------------------------------------------------- backtrace
    for (int t0 = ((L - 1) / CE_CH) * CE_CH; t0 >= 0; t0 -= CE_CH) {
      uint32_t W[CE_CH / 4];  // the chunk's backpointers of state j: word q = steps t0 + 4 q .. + 3
#pragma unroll
      for (int q = 0; q < CE_CH / 4; ++q) {
        const int64_t tq = (t0 >> 2) + q;
        W[q] = (j < SP && tq < T4 && tq * 4 <= L - 1) ? bp[tq * SP + j] : 0u;
      }
      int pv = -1;
      const int tlane = t0 + lane;  // (compared with t, not lane with s: see hmm_code_decode.hip)
#pragma unroll
      for (int s = CE_CH - 1; s >= 0; --s) {
        const int t = t0 + s;
        if (t <= L - 1) {  // wave-uniform
          pv = tlane == t ? state : pv;
          if (t >= 1) state = (int)(((uint32_t)__builtin_amdgcn_readlane((int)W[s >> 2], state) >> (8 * (s & 3))) & 0x1Fu);
        }
      }
      if (t0 + lane <= L - 1) P[t0 + lane] = pv;
    }
  }
}

// ----------------------------------------------------------------------------- filter
template <int SP, class EM>
__global__ __launch_bounds__(256) void gauss_filter_kernel(const GdArgs a) {
  extern __shared__ float gd_smem[];
  constexpr int ES = SP | 1;
  const int S = a.S, D = a.D, T = a.T, DS = D | 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int j = lane, jj = j & (SP - 1);
  const bool act = j < S;
  float* tb = gd_smem;
  float* xbuf = tb + EM::table_floats(S, D) + wave * (CE_CH * (DS + ES));
  float* ebuf = xbuf + CE_CH * DS;
  EM::table(a.mean, a.par, S, D, tb, tid, (int)blockDim.x);
  __syncthreads();

  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < a.B; b += (int64_t)gridDim.x * nw) {
    const int64_t Lr = a.lengths[b];
    const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
    const float* xs = a.x + b * (int64_t)T * D;
    float* F = a.filt ? a.filt + b * (int64_t)T * S : nullptr;
    const float* pvec = a.prev ? a.prev + b * S : nullptr;
    if (L == 0) {
      const float keep = (pvec && act) ? pvec[j] : 0.f;
      if (F)
        for (int64_t e = lane; e < (int64_t)T * S; e += 64) F[e] = 0.f;
      if (a.last && act) a.last[b * S + j] = keep;
      if (a.loglik && lane == 0) a.loglik[b] = ce_nan();
      continue;
    }

    float xf = 0.f;
    double Sll = 0.0;
    int status = 0;  // 1: impossible (mass 0), 2: a non-finite x or emission inside the length
    int tfail = 0;   // the position that failed
    if (pvec) {
      const float p = act ? pvec[j] : 0.f;
      const float sp = ce_uni(ce_red<SP>(p, CeAdd{}));
      if (sp > 0.f && sp < __builtin_huge_valf()) xf = p / sp;
      else status = 1;
    }
    {
      float Acol[SP];
#pragma unroll
      for (int i = 0; i < SP; ++i) Acol[i] = (act && i < S) ? __expf(a.log_A[i * S + j]) : 0.f;
      const float pij = (act && !pvec) ? __expf(a.log_pi[j]) : 0.f;
      float Pm = 1.f, Dr = 0.f;
      for (int t0 = 0; t0 < L && status == 0; t0 += CE_CH) {
        int n = min(CE_CH, L - t0);
        // the chunk at t0: x to LDS, then e_t = exp(em_t - max_s em_t) for its rows (zeros in the columns
        // [S, SP) and the rows past n), Mv = the lane's row maximum
        asm volatile("" ::: "memory");
        const bool badx = EM::stage_x(xs + (int64_t)t0 * D, n, D, DS, lane, xbuf);
        asm volatile("" ::: "memory");
        float Mv;
        const bool bade = EM::chunk_em(xbuf, DS, tb, S, D, n, lane, ebuf, ES, Mv);
        int nbad = -1;
        if (badx || bade) {  // the first row whose x or emission is not finite: the steps before it still run
          bool rb = false;
          if (lane < n) {
            for (int dd = 0; dd < D; ++dd) rb |= gd_nonfinite(xbuf[lane * DS + dd]);
            for (int s = 0; s < S; ++s) rb |= gd_nonfinite(ebuf[lane * ES + s]);
          }
          const uint64_t badm = __builtin_amdgcn_ballot_w64(rb);
          nbad = badm ? (int)__builtin_ctzll(badm) : 0;
          n = nbad;
        }
        for (int s = 0; s < SP; ++s) {
          const float v = (lane < n && s < S) ? expf(ebuf[lane * ES + s] - Mv) : 0.f;
          ebuf[lane * ES + s] = v;
        }
        asm volatile("" ::: "memory");
        // ln e_t(j) of row s of the staged chunk, for the lane's state (the rare path)
        auto log_e = [&](int s) {
          return act ? EM::em_one(xbuf + s * DS, tb, j, S, D) - ce_lane(Mv, s) : CE_NEG_INF;
        };
        float e_nx = ebuf[jj];
        for (int s = 0; s < n; ++s) {
          const int t = t0 + s;
          const float e = e_nx;
          e_nx = ebuf[min(s + 1, CE_CH - 1) * ES + jj];  // one step ahead of the chain
          Sll += (double)ce_lane(Mv, s);
          const bool first = t == 0 && !pvec;
          float u;
          if (first) {
            u = pij;
          } else {
            // four independent accumulation chains
            float u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f;
#pragma unroll
            for (int i = 0; i < SP; i += 4) {
              u0 = fmaf(Acol[i], ce_lane(xf, i), u0);
              if (i + 1 < SP) u1 = fmaf(Acol[i + 1], ce_lane(xf, i + 1), u1);
              if (i + 2 < SP) u2 = fmaf(Acol[i + 2], ce_lane(xf, i + 2), u2);
              if (i + 3 < SP) u3 = fmaf(Acol[i + 3], ce_lane(xf, i + 3), u3);
            }
            u = (u0 + u1) + (u2 + u3);
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
            if (first) {
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
            const float lb = log_e(s);
            const float ly = (lp == CE_NEG_INF || lb == CE_NEG_INF) ? CE_NEG_INF : lp + lb;
            const float M = ce_red<SP>(ly, CeMax{});
            if (ce_uni(M) == CE_NEG_INF) {
              status = 1;
              tfail = t;
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
          if (F && act) F[(int64_t)t * S + j] = xf;
        }
        Sll += (double)__builtin_amdgcn_logf(Pm) * CE_LN2;
        Pm = 1.f;
        if (status == 0 && nbad >= 0) {
          status = 2;
          tfail = t0 + nbad;
        }
      }
      Sll -= (double)Dr;
    }
    // rows past the length, or from the failing position on
    const int tz = status != 0 ? tfail : L;
    if (F)
      for (int64_t e = (int64_t)tz * S + lane; e < (int64_t)T * S; e += 64) F[e] = 0.f;
    if (a.last && act) a.last[b * S + j] = status != 0 ? 0.f : xf;
    if (a.loglik && lane == 0) a.loglik[b] = status == 0 ? (float)Sll : status == 1 ? CE_NEG_INF : ce_nan();
  }
}

// ---------------------------------------------------------------------------------------- host
struct GdPlan {
  int nw;
  int64_t nblk;
  size_t lds_bytes;
};

inline int64_t gd_sp(int64_t S) {
  int64_t SP = 1;
  while (SP < S) SP *= 2;
  return SP;
}

// table_bytes: the workgroup's shared emission table; cap = EM::cu_waves(SP), the waves per CU the kernels'
// registers allow.  The waves per workgroup that put most waves on a CU's LDS (cap at most); on a tie the
// fewest, which spreads a small batch over more CUs
inline GdPlan gd_plan(int64_t B, int64_t S, int64_t D, size_t table_bytes, int64_t cap) {
  GdPlan p;
  const size_t pw = (size_t)CE_CH * ((D | 1) + (gd_sp(S) | 1)) * 4;
  p.nw = 1;
  int64_t best = 0;
  for (int64_t nw = 1; nw <= GD_MAX_NW; ++nw) {
    const size_t wg = table_bytes + (size_t)nw * pw;
    if (wg > GD_LDS_MAX) break;
    int64_t per_cu = (int64_t)(GD_LDS_CU / wg) * nw;
    per_cu = per_cu > cap ? cap : per_cu;
    if (per_cu > best) {
      best = per_cu;
      p.nw = (int)nw;
    }
  }
  p.nblk = cdiv(B, p.nw) < GD_MAX_WAVES / p.nw ? cdiv(B, p.nw) : GD_MAX_WAVES / p.nw;
  if (p.nblk < 1) p.nblk = 1;
  p.lds_bytes = table_bytes + (size_t)p.nw * pw;
  return p;
}

inline size_t gd_viterbi_ws_bytes(int64_t B, int64_t T, int64_t S) {
  return r256((size_t)B * (size_t)cdiv(T, 4) * (size_t)gd_sp(S) * 4);
}

template <int SP, class EM, bool VIT>
int gd_go(const GdArgs& a, const GdPlan& p, hipStream_t s) {
  auto kern = VIT ? gauss_viterbi_kernel<SP, EM> : gauss_filter_kernel<SP, EM>;
  if (p.lds_bytes > GD_LDS_SOFT) {
    // more than 64 KB of dynamic LDS has to be asked for, once per kernel
    static const hipError_t big_lds = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GD_LDS_MAX);
    (void)big_lds;
  }
  kern<<<(unsigned)p.nblk, 64 * p.nw, p.lds_bytes, s>>>(a);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

template <class EM, bool VIT>
int gd_dispatch(const GdArgs& a, const GdPlan& p, hipStream_t s) {
  const int S = a.S;
  if (S > 16) return gd_go<32, EM, VIT>(a, p, s);
  if (S > 8) return gd_go<16, EM, VIT>(a, p, s);
  if (S > 4) return gd_go<8, EM, VIT>(a, p, s);
  if (S > 2) return gd_go<4, EM, VIT>(a, p, s);
  if (S > 1) return gd_go<2, EM, VIT>(a, p, s);
  return gd_go<1, EM, VIT>(a, p, s);
}

inline int gd_fill(float* p, int64_t n, float v, hipStream_t s) {
  if (!p || n <= 0) return VQHMM_OK;
  gauss_dec_fill_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(p, n, v);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

// the launchers' bodies behind the domain checks (B > 0)
template <class EM>
int gd_launch_viterbi(const float* log_pi, const float* log_A, const float* mean, const float* par, const float* x,
                      const int64_t* lengths, int64_t B, int64_t T, int64_t S, int64_t D, int32_t* path,
                      float* score, void* ws, hipStream_t s) {
  if (T == 0) return gd_fill(score, B, CE_NEG_INF, s);  // every length is 0
  const GdPlan p = gd_plan(B, S, D, (size_t)EM::table_floats((int)S, (int)D) * 4, EM::cu_waves((int)gd_sp(S)));
  GdArgs a = {};
  a.log_pi = log_pi; a.log_A = log_A; a.mean = mean; a.par = par; a.x = x; a.lengths = lengths;
  a.B = B; a.T = (int)T; a.S = (int)S; a.D = (int)D;
  a.bp = reinterpret_cast<uint32_t*>(ws);
  a.path = path; a.score = score;
  return gd_dispatch<EM, true>(a, p, s);
}

template <class EM>
int gd_launch_filter(const float* log_pi, const float* log_A, const float* mean, const float* par, const float* x,
                     const int64_t* lengths, const float* prev, int64_t B, int64_t T, int64_t S, int64_t D,
                     float* filt, float* last, float* loglik, hipStream_t s) {
  if (T == 0) {  // every length is 0: loglik = NaN, last = prev (or zeros)
    if (last && prev && last != prev &&
        hipMemcpyAsync(last, prev, sizeof(float) * B * S, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    if (last && !prev && hipMemsetAsync(last, 0, sizeof(float) * B * S, s) != hipSuccess) return VQHMM_ELAUNCH;
    return gd_fill(loglik, B, __builtin_nanf(""), s);
  }
  const GdPlan p = gd_plan(B, S, D, (size_t)EM::table_floats((int)S, (int)D) * 4, EM::cu_waves((int)gd_sp(S)));
  GdArgs a = {};
  a.log_pi = log_pi; a.log_A = log_A; a.mean = mean; a.par = par; a.x = x; a.lengths = lengths;
  a.B = B; a.T = (int)T; a.S = (int)S; a.D = (int)D;
  a.prev = prev; a.filt = filt; a.last = last; a.loglik = loglik;
  return gd_dispatch<EM, false>(a, p, s);
}

}  // namespace

}  // namespace vqhmm
