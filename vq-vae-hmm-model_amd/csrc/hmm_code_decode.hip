// Stationary HMM on VQ code indices: the fused Viterbi decode and the streaming causal filter
// (contracts in include/vqhmm.h; restatements in tests/code_decode_ref.py; DESIGN.md "HMM on code indices").
//
//   model    log_pi (S), log_A (S,S) rows = from-state, log_B (S,V) categorical emission over codes
//   viterbi  path (B,T) int32 (-1 past the length), score (B)
//   filter   filt (B,T,S) = p(z_t | codes_{0:t}) (optional), last (B,S) = filt at L - 1 (optional),
//            loglik (B) (optional); prev (B,S) (optional) = the filtered state just before this chunk
//
// Lane map.  hmm_code.hip's: one sequence per wave at a time, lane j < S = state j, SP = S rounded up to a
// power of two the compile-time width.  Lane j keeps column j of the transition matrix in SP registers for
// the whole sequence and reads the previous step's vector with v_readlane into scalar registers, so a step
// has no LDS round trip and no cross-lane reduction on its chain (the filter's normaliser is one DPP
// all-reduce), and every branch on a sequence's state (its length, a bad code, an impossible step, a step
// that leaves the fast range) is wave-uniform.  The per-position data is the 4-byte code: a chunk of 64 codes
// is one load, lane s holding step s's code.
//
// Emission.  A prologue launch writes the (V,S) transposed table into the workspace: exp(log_B)^T for the
// filter (hmm_code_dev.h's prologue, the E-step's) and log_B^T, the same bits moved, for Viterbi.  LDS tier:
// the table fits 64 KB and every workgroup copies it to LDS once; a step reads its row by the step's code.
// L2 tier: a wave stages the 64 rows of its chunk from the workspace (L2) into its own LDS buffer, all loads
// in flight together.  Steps run in unrolled blocks of VB whose rows are read together, a block ahead of the
// chain; a sequence's first VB steps and a chunk's last n mod VB go through a general step.
//
// Viterbi.  d_0[j] = log_pi[j] + log_B[j,c_0], d_t[j] = (max_i (d_{t-1}[i] + log_A[i,j])) + log_B[j,c_t] in
// fp32 in this order, i ascending with a strict > (evaluated as a compare tree that selects the same
// candidate).  Lane j packs its backpointers of four steps into one word and stores it to the workspace
// ([b][t / 4][SP] words: one byte per state and step).  The backtrace reloads 64 steps' words into 16
// registers per lane and resolves them with v_readlane at the (scalar) current state: no memory access on
// that chain; the 64 path entries leave in one store.
//
// Filter.  The E-step's forward chain: linear probabilities normalised at every step, the logs of the step
// masses summed in fp64 (four masses per log2), a step whose mass leaves [2^-30, 2^30] redone max-shifted in
// natural log from the tables in memory.  With prev, step 0 is an ordinary step from prev / sum(prev).
//
// Addressing.  codes are read at min(t, T - 1) of the wave's own row, the table only at validated codes,
// parameters at (i, j) < S, the backpointer words inside the sequence's own rows; offsets are 64-bit.
#include "hmm_code_dev.h"

namespace vqhmm {

namespace {

constexpr int CD_NW = 4;                      // waves (sequences in flight) per workgroup
constexpr size_t CD_LDS_TAB = 64 * 1024;      // LDS tier: the table's bytes (two workgroups per CU)
constexpr int64_t CD_MAX_WG = 2048;           // workgroups; further sequences by striding
constexpr int VB = 8;                         // steps per unrolled block (a multiple of 4, divides CE_CH)

struct DecArgs {
  const float* log_pi;
  const float* log_A;
  const float* log_B;
  const int32_t* codes;
  const int64_t* lengths;
  int64_t B;
  int T, S, V;
  const float* tab;  // (V, S): log_B^T (viterbi) or exp(log_B)^T (filter)
  // viterbi
  uint32_t* bp;      // [B][ceil(T / 4)][SP]
  int32_t* path;
  float* score;
  // filter
  const float* prev;  // nullable
  float* filt;        // nullable
  float* last;        // nullable
  float* loglik;      // nullable
};

__global__ __launch_bounds__(256) void code_lbt_kernel(const float* __restrict__ log_B, int S, int V,
                                                       float* __restrict__ lbt) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (int64_t)S * V) return;
  const int v = (int)(k / S), s = (int)(k - (int64_t)v * S);
  lbt[k] = log_B[(int64_t)s * V + v];
}

__global__ __launch_bounds__(256) void code_fill_kernel(float* __restrict__ p, int64_t n, float v) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) p[k] = v;
}

// L2 tier: the chunk's emission rows (row s = the table's row of lane s's code) into the wave's buffer
template <int SP>
__device__ __forceinline__ void cd_stage(const float* __restrict__ tab, int S, int cvs, int n, int lane,
                                         float* ebuf) {
#pragma unroll
  for (int k = 0; k < SP; ++k) {
    const int idx = k * 64 + lane, s = idx / SP, jj = idx - s * SP;
    const int cs = __shfl(cvs, s);
    ebuf[idx] = (jj < S && s < n) ? tab[(int64_t)cs * S + jj] : 0.f;
  }
  asm volatile("" ::: "memory");  // the wave's own LDS stores, read across lanes by the steps
}

// ---------------------------------------------------------------------------- viterbi
template <int SP, bool LDS_T>
__global__ __launch_bounds__(256) void code_viterbi_kernel(const DecArgs a) {
  extern __shared__ float cd_smem[];
  const int S = a.S, V = a.V, T = a.T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int j = lane;
  const bool act = j < S;
  const float* tl = cd_smem;                        // LDS tier: the whole table
  float* ebuf = cd_smem + wave * (CE_CH * SP);      // L2 tier: the wave's chunk rows
  if constexpr (LDS_T) {
    for (int k = tid; k < S * V; k += blockDim.x) cd_smem[k] = a.tab[k];
    __syncthreads();
  }
  const int64_t T4 = (T + 3) / 4;

  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < a.B; b += (int64_t)gridDim.x * nw) {
    const int64_t Lr = a.lengths[b];
    const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
    const int32_t* cb = a.codes + b * T;
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
      const int32_t cv = cb[min(t0 + lane, T - 1)];
      if (__builtin_amdgcn_ballot_w64(lane < n && (cv < 0 || cv >= V)) != 0) {
        bad = true;
        break;
      }
      const int cvs = lane < n ? cv : 0;
      if constexpr (!LDS_T) cd_stage<SP>(a.tab, S, cvs, n, lane, ebuf);
      // step s's emission row, for the lane's state (lanes past n hold code 0, so any s < 64 is a safe read)
      // (an unconditional read at a safe column and a select: no branch around the read)
      const int cvS = cvs * S, jj = act ? j : 0;
      auto emis = [&](int s) {
        if constexpr (LDS_T) {
          const float r = tl[__builtin_amdgcn_readlane(cvS, s) + jj];
          return act ? r : 0.f;
        } else {
          return ebuf[s * SP + (j & (SP - 1))];
        }
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
        // the rule's "i ascending, strict >" picks the least (value descending, index ascending) candidate, a
        // total order, so a tree in which the higher-index half wins only by a strict > picks the same one at
        // log2(SP) dependent compares instead of SP - 1
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
        for (; s < min(n, VB); ++s) any_step(s);
      // whole blocks of VB steps (s a multiple of VB): the block's emissions are read together, a block ahead of
      // the chain, and nothing but the steps themselves is left on it
      if (SP <= 16 && s + VB <= n) {  // (SP = 32: eight unrolled steps cost a wave per SIMD in registers)
        float E[VB];
#pragma unroll
        for (int u = 0; u < VB; ++u) E[u] = emis(s + u);
        for (; s + VB <= n; s += VB) {
          float En[VB] = {};
          if (s + 2 * VB <= n) {
#pragma unroll
            for (int u = 0; u < VB; ++u) En[u] = emis(s + VB + u);
          }
#pragma unroll
          for (int u = 0; u < VB; ++u) {
            vstep(E[u], 8 * (u & 3));
            if ((u & 3) == 3) flush(t0 + s + u);
          }
#pragma unroll
          for (int u = 0; u < VB; ++u) E[u] = En[u];
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
      const int tlane = t0 + lane;  // (compared with t, not lane with s: 64 loop-invariant lane masks would be
                                  // hoisted out of the chunk loop and spilled)
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
template <int SP, bool LDS_T>
__global__ __launch_bounds__(256) void code_filter_kernel(const DecArgs a) {
  extern __shared__ float cd_smem[];
  const int S = a.S, V = a.V, T = a.T;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = ce_uni(tid >> 6), nw = (int)(blockDim.x >> 6);
  const int j = lane;
  const bool act = j < S;
  const float* bt = cd_smem;
  float* ebuf = cd_smem + wave * (CE_CH * SP);
  if constexpr (LDS_T) {
    for (int k = tid; k < S * V; k += blockDim.x) cd_smem[k] = a.tab[k];
    __syncthreads();
  }

  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < a.B; b += (int64_t)gridDim.x * nw) {
    const int64_t Lr = a.lengths[b];
    const int L = ce_uni((int)(Lr <= 0 ? 0 : (Lr < T ? Lr : T)));
    const int32_t* cb = a.codes + b * T;
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

    float x = 0.f;
    double Sll = 0.0;
    int status = 0;  // 1: impossible (mass 0), 2: a code outside [0, V) inside the length
    int tfail = 0;   // the position that failed
    if (pvec) {
      const float p = act ? pvec[j] : 0.f;
      const float sp = ce_uni(ce_red<SP>(p, CeAdd{}));
      if (sp > 0.f && sp < __builtin_huge_valf()) x = p / sp;
      else status = 1;
    }
    {
      float Acol[SP];
#pragma unroll
      for (int i = 0; i < SP; ++i) Acol[i] = (act && i < S) ? __expf(a.log_A[i * S + j]) : 0.f;
      float P = 1.f, D = 0.f;
      for (int t0 = 0; t0 < L && status == 0; t0 += CE_CH) {
        int n = min(CE_CH, L - t0);
        const int32_t cv = cb[min(t0 + lane, T - 1)];
        const uint64_t badm = __builtin_amdgcn_ballot_w64(lane < n && (cv < 0 || cv >= V));
        int nbad = -1;
        if (badm != 0) {  // the steps before the first bad code still run
          nbad = (int)__builtin_ctzll(badm);
          n = nbad;
        }
        const int cvs = lane < n ? cv : 0;
        if constexpr (!LDS_T) cd_stage<SP>(a.tab, S, cvs, n, lane, ebuf);
        const int cvS = cvs * S, jj = act ? j : 0;
        auto emis = [&](int s) {
          if constexpr (LDS_T) {
            const float r = bt[__builtin_amdgcn_readlane(cvS, s) + jj];
            return act ? r : 0.f;
          } else {
            return ebuf[s * SP + (j & (SP - 1))];
          }
        };
        // the sequence's first step without prev: in natural log from log_pi
        auto first_step = [&](int code) {
          const float ly = act ? a.log_pi[j] + a.log_B[(int64_t)j * V + code] : CE_NEG_INF;
          const float M = ce_red<SP>(ly, CeMax{});
          if (ce_uni(M) == CE_NEG_INF) {
            status = 1;
            tfail = 0;
            return;
          }
          const float ex = ly == CE_NEG_INF ? 0.f : expf(ly - M);
          const float st = ce_red<SP>(ex, CeAdd{});
          x = ex / st;
          Sll = (double)M + (double)logf(st);
          if (F && act) F[j] = x;
        };
        // an ordinary step t (chunk step s) with emission row e; a failed step leaves status set and stores nothing
        auto fstep = [&](int t, int s, float e) {
          // four independent accumulation chains (the E-step's forward keeps two)
          float u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f;
#pragma unroll
          for (int i = 0; i < SP; i += 4) {
            u0 = fmaf(Acol[i], ce_lane(x, i), u0);
            if (i + 1 < SP) u1 = fmaf(Acol[i + 1], ce_lane(x, i + 1), u1);
            if (i + 2 < SP) u2 = fmaf(Acol[i + 2], ce_lane(x, i + 2), u2);
            if (i + 3 < SP) u3 = fmaf(Acol[i + 3], ce_lane(x, i + 3), u3);
          }
          const float y = ((u0 + u1) + (u2 + u3)) * e;
          const float c = ce_red<SP>(j < SP ? y : 0.f, CeAdd{});
          const float cu = ce_uni(c);
          if (cu >= CE_LO && cu <= CE_HI) {
            const float r = __builtin_amdgcn_rcpf(c);
            x = y * r;
            P *= c;
            D += fmaf(r, c, -1.f);
          } else {
            // rare path: the step in natural log, max-shifted, from the tables in memory
            const int code = __builtin_amdgcn_readlane(cvs, s);
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
              tfail = t;
              return;
            }
            const float ex = ly == CE_NEG_INF ? 0.f : expf(ly - M);
            const float st = ce_red<SP>(ex, CeAdd{});
            x = ex / st;
            Sll += (double)M + (double)logf(st);
          }
          if (F && act) F[(int64_t)t * S + j] = x;
        };
        // the log and the fp64 add of four step masses at once
        auto fold = [&]() {
          Sll += (double)__builtin_amdgcn_logf(P) * CE_LN2;
          P = 1.f;
        };
        // any step, every case tested: the sequence's first steps and the chunk's last ones
        auto any_step = [&](int s) {
          const int t = t0 + s;
          if (t == 0 && !pvec) {
            first_step(__builtin_amdgcn_readlane(cvs, 0));
            return;
          }
          fstep(t, s, emis(s));
          if (status == 0 && (s & 3) == 3) fold();
        };
        int s = 0;
        if (t0 == 0)
          for (; s < min(n, VB) && status == 0; ++s) any_step(s);
        // whole blocks of VB steps (s a multiple of VB): the block's emission rows are read together, a block
        // ahead of the chain
        if (s + VB <= n && status == 0) {
          float E[VB];
#pragma unroll
          for (int u = 0; u < VB; ++u) E[u] = emis(s + u);
          for (; s + VB <= n && status == 0; s += VB) {
            float En[VB] = {};
            if (s + 2 * VB <= n) {
#pragma unroll
              for (int u = 0; u < VB; ++u) En[u] = emis(s + VB + u);
            }
#pragma unroll
            for (int u = 0; u < VB; ++u) {
              if (status == 0) {
                fstep(t0 + s + u, s + u, E[u]);
                if ((u & 3) == 3 && status == 0) fold();
              }
            }
#pragma unroll
            for (int u = 0; u < VB; ++u) E[u] = En[u];
          }
        }
        for (; s < n && status == 0; ++s) any_step(s);
        Sll += (double)__builtin_amdgcn_logf(P) * CE_LN2;
        P = 1.f;
        if (status == 0 && nbad >= 0) {
          status = 2;
          tfail = t0 + nbad;
        }
      }
      Sll -= (double)D;
    }
    // rows past the length, or from the failing position on
    const int tz = status != 0 ? tfail : L;
    if (F)
      for (int64_t e = (int64_t)tz * S + lane; e < (int64_t)T * S; e += 64) F[e] = 0.f;
    if (a.last && act) a.last[b * S + j] = status != 0 ? 0.f : x;
    if (a.loglik && lane == 0) a.loglik[b] = status == 0 ? (float)Sll : status == 1 ? CE_NEG_INF : ce_nan();
  }
}

struct DecPlan {
  bool lds;
  int64_t nblk;
  size_t lds_bytes;
  size_t off_tab, bytes;
};

int64_t dec_sp(int64_t S) {
  int64_t SP = 1;
  while (SP < S) SP *= 2;
  return SP;
}

DecPlan dec_plan(int64_t B, int64_t T, int64_t S, int64_t V, bool viterbi) {
  DecPlan p;
  const int64_t SP = dec_sp(S);
  const size_t NV = (size_t)S * V;
  p.lds = NV * 4 <= CD_LDS_TAB;
  p.lds_bytes = p.lds ? NV * 4 : (size_t)CD_NW * CE_CH * SP * 4;
  p.nblk = cdiv(B, CD_NW) < CD_MAX_WG ? cdiv(B, CD_NW) : CD_MAX_WG;
  if (p.nblk < 1) p.nblk = 1;
  p.off_tab = viterbi ? r256((size_t)B * (size_t)cdiv(T, 4) * SP * 4) : 0;
  p.bytes = p.off_tab + r256(NV * 4);
  return p;
}

template <int SP, bool VIT>
int dec_go(const DecArgs& a, const DecPlan& p, hipStream_t s) {
  if (p.lds) {
    auto kern = VIT ? code_viterbi_kernel<SP, true> : code_filter_kernel<SP, true>;
    // the tier's limit covers every launch; asked for once per kernel
    static const hipError_t lds_attr = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CD_LDS_TAB);
    (void)lds_attr;
    kern<<<(unsigned)p.nblk, 64 * CD_NW, p.lds_bytes, s>>>(a);
  } else {
    auto kern = VIT ? code_viterbi_kernel<SP, false> : code_filter_kernel<SP, false>;
    kern<<<(unsigned)p.nblk, 64 * CD_NW, p.lds_bytes, s>>>(a);
  }
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

template <bool VIT>
int dec_dispatch(const DecArgs& a, const DecPlan& p, hipStream_t s) {
  const int S = a.S;
  if (S > 16) return dec_go<32, VIT>(a, p, s);
  if (S > 8) return dec_go<16, VIT>(a, p, s);
  if (S > 4) return dec_go<8, VIT>(a, p, s);
  if (S > 2) return dec_go<4, VIT>(a, p, s);
  if (S > 1) return dec_go<2, VIT>(a, p, s);
  return dec_go<1, VIT>(a, p, s);
}

int dec_fill(float* p, int64_t n, float v, hipStream_t s) {
  if (!p || n <= 0) return VQHMM_OK;
  code_fill_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(p, n, v);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

}  // namespace

size_t hmm_code_viterbi_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t V) {
  if (!hmm_code_supported(S, V) || B < 0 || T < 0) return 0;
  return dec_plan(B, T, S, V, true).bytes;
}

size_t hmm_code_filter_ws_bytes(int64_t B, int64_t T, int64_t S, int64_t V) {
  if (!hmm_code_supported(S, V) || B < 0 || T < 0) return 0;
  return dec_plan(B, T, S, V, false).bytes;
}

int launch_hmm_code_viterbi(const float* log_pi, const float* log_A, const float* log_B, const int32_t* codes,
                            const int64_t* lengths, int64_t B, int64_t T, int64_t S, int64_t V, int32_t* path,
                            float* score, void* ws, hipStream_t s) {
  if (!hmm_code_supported(S, V) || T > (1 << 28) || B > INT32_MAX) return VQHMM_EUNSUPPORTED;
  if (B == 0) return VQHMM_OK;
  if (T == 0) return dec_fill(score, B, CE_NEG_INF, s);  // every length is 0
  const DecPlan p = dec_plan(B, T, S, V, true);
  char* w = static_cast<char*>(ws);
  float* lbt = reinterpret_cast<float*>(w + p.off_tab);
  DecArgs a = {};
  a.log_pi = log_pi; a.log_A = log_A; a.log_B = log_B; a.codes = codes; a.lengths = lengths;
  a.B = B; a.T = (int)T; a.S = (int)S; a.V = (int)V;
  a.tab = lbt;
  a.bp = reinterpret_cast<uint32_t*>(w);
  a.path = path; a.score = score;
  code_lbt_kernel<<<(unsigned)cdiv(S * V, 256), 256, 0, s>>>(log_B, (int)S, (int)V, lbt);
  VQHMM_LAUNCH_CHECK();
  return dec_dispatch<true>(a, p, s);
}

int launch_hmm_code_filter(const float* log_pi, const float* log_A, const float* log_B, const int32_t* codes,
                           const int64_t* lengths, const float* prev, int64_t B, int64_t T, int64_t S, int64_t V,
                           float* filt, float* last, float* loglik, void* ws, hipStream_t s) {
  if (!hmm_code_supported(S, V) || T > (1 << 28) || B > INT32_MAX) return VQHMM_EUNSUPPORTED;
  if (B == 0) return VQHMM_OK;
  if (T == 0) {  // every length is 0: loglik = NaN, last = prev (or zeros)
    if (last && prev && last != prev &&
        hipMemcpyAsync(last, prev, sizeof(float) * B * S, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return VQHMM_ELAUNCH;
    if (last && !prev && hipMemsetAsync(last, 0, sizeof(float) * B * S, s) != hipSuccess) return VQHMM_ELAUNCH;
    return dec_fill(loglik, B, __builtin_nanf(""), s);
  }
  const DecPlan p = dec_plan(B, T, S, V, false);
  char* w = static_cast<char*>(ws);
  float* Bt = reinterpret_cast<float*>(w + p.off_tab);
  DecArgs a = {};
  a.log_pi = log_pi; a.log_A = log_A; a.log_B = log_B; a.codes = codes; a.lengths = lengths;
  a.B = B; a.T = (int)T; a.S = (int)S; a.V = (int)V;
  a.tab = Bt;
  a.prev = prev; a.filt = filt; a.last = last; a.loglik = loglik;
  code_bt_kernel<<<(unsigned)cdiv(S * V, 256), 256, 0, s>>>(log_B, (int)S, (int)V, Bt);
  VQHMM_LAUNCH_CHECK();
  return dec_dispatch<false>(a, p, s);
}

}  // namespace vqhmm
