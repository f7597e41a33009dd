// vqhmm_gauss_scenario_f32 (contract: include/vqhmm.h, "Gaussian HMM scenarios"): from a regime distribution
// start (B,S) to N Monte Carlo paths of H steps per start, in one launch and without a random number in HBM.
//
// One lane = one path (b, n): the flat path index p = b N + n is the parallel axis, a path's H steps are serial.
// Per step the lane
//   draws a Philox4x32-10 block (counter (n0+n, b0+b, t, 0)) for the regime uniform and takes z_t by
//     vqhmm_code_sample_f32's inverse-CDF rule from start[b] (t = 0) or row z_{t-1} of exp(log_A) (LDS),
//   draws ceil(D / 4) more blocks (counter word 3 = 1 + d / 4), four Box-Muller normals each,
//   forms x = mean + sd eps (diag: block by block, nothing kept) or mean + L eps (full: eps in DP registers, the
//     triangular product fully unrolled over the packed rows of L in LDS),
//   and carries wealth, peak and drawdown in fp64.
// Parameters live in LDS with an odd stride per regime (A rows, mean, sd / packed L, port): the lanes of a wave
// sit in different regimes and read the same (i, j) of different regimes in one instruction, and with an odd
// stride the S <= 32 regimes fall on S different banks of the 32 a ds_read_b32 sees (lanes in one regime
// broadcast).  The turnover sum_d |port[z] - held| is an (S+1) x S fp64 table (held is a row of port or nothing).
// states, wealth and x are staged in a wave-private LDS tile (32 steps of states / wealth, ceil(32 / D) steps of
// x per lane) and leave as runs of consecutive addresses written by consecutive lanes, not as one line per lane
// per step.  A launch that asks for final / drawdown only stages nothing and stores 8 bytes per path.
// A path is a function of (seed, b0+b, n0+n) and the parameters: no lane reads another lane's state.
#include "kernels.h"

namespace vqhmm {

namespace {
constexpr int GS_TS = 32;                    // steps of states / wealth a lane stages between two flushes
constexpr int GS_TSTR = GS_TS + 1;           // ... and their odd LDS stride
constexpr size_t GS_LDS_MAX = 156 * 1024;    // of the CU's 160 KB
constexpr size_t GS_LDS_SOFT = 80 * 1024;    // two workgroups per CU: fewer waves per workgroup above this
constexpr int64_t GS_MAX_PATHS = int64_t(1) << 36;   // B N: 2^30 workgroups of one wave
constexpr int64_t GS_MAX_STEPS = int64_t(1) << 48;   // B N H: the offsets into x stay below 2^54
constexpr int64_t GS_MAX_H = 1 << 28;

struct ScenArgs {
  const float* start;
  const float* log_A;
  const float* mean;
  const float* scale;
  const float* port;
  int32_t* states;
  float* x;
  float* wealth;
  float* fin;
  float* dd;
  int64_t N, P;                // paths per start, paths in all (B N)
  uint32_t k0, k1, b0, n0;     // the Philox key and the counter origin
  int H, S, D, reb;
  float tx;
  int nturn;                   // doubles of the turnover table in front of the floats
  int SA, SD, SL;              // strides: A rows, mean / sd / port rows, the scale rows (SD or the packed L's)
  int oTot, oMean, oScale, oPort, oStage, wstage;   // float offsets; wstage = a wave's staging floats
  int xts, XS;                 // steps of x staged per lane, its stride
};

__host__ __device__ __forceinline__ int gs_odd(int v) { return v | 1; }
__host__ __device__ __forceinline__ int gs_tri(int i) { return i * (i + 1) / 2; }

// WIDE: each product as one 32 x 32 -> 64 multiply (v_mad_u64_u32) instead of a mul_hi and a mul_lo.  The same
// bits; measured in alternation on MI355X the wide form is 3.6 % faster in the diagonal kernel and 5-8 % slower
// in the full ones (profiles/gauss_scenario/), so each takes its own.
template <bool WIDE>
__device__ __forceinline__ void gs_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                          uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0, lo0, hi1, lo1;
    if constexpr (WIDE) {
      const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
      hi0 = (uint32_t)(p0 >> 32); lo0 = (uint32_t)p0;
      hi1 = (uint32_t)(p1 >> 32); lo1 = (uint32_t)p1;
    } else {
      hi0 = __umulhi(0xD2511F53u, c0); lo0 = 0xD2511F53u * c0;
      hi1 = __umulhi(0xCD9E8D57u, c2); lo1 = 0xCD9E8D57u * c2;
    }
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// two normals from two words: u1 in (0, 1], u2 in [0, 1), |eps| <= sqrt(48 ln 2) = 5.77
__device__ __forceinline__ void gs_box_muller(uint32_t wa, uint32_t wb, float& e0, float& e1) {
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
  const float u2 = (float)(wb >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.f * logf(u1));
  e0 = r * cospif(2.f * u2);
  e1 = r * sinpif(2.f * u2);
}

template <bool WIDE>
__device__ __forceinline__ void gs_normals4(uint32_t c0, uint32_t c1, uint32_t t, uint32_t j, uint32_t k0,
                                            uint32_t k1, float (&e)[4]) {
  uint32_t o[4];
  gs_philox<WIDE>(c0, c1, t, j, k0, k1, o);
  gs_box_muller(o[0], o[1], e[0], e[1]);
  gs_box_muller(o[2], o[3], e[2], e[3]);
}

// vqhmm_code_sample_f32's draw over the weights p[0..n): the first k with p_k > 0 and u < run_k / total (run = the
// fp32 running sum), else the last k with p_k > 0.  Always in [0, n).
template <typename P>
__device__ __forceinline__ int gs_draw(const P* __restrict__ p, int n, float total, float u) {
  float run = 0.f;
  int sel = -1, last = 0;
  for (int k = 0; k < n; ++k) {
    const float pk = p[k];
    run += pk;
    if (pk > 0.f) {
      last = k;
      if (sel < 0 && u < run / total) sel = k;
    }
    if (__builtin_amdgcn_ballot_w64(sel < 0) == 0) break;   // every lane of the wave has drawn
  }
  return sel >= 0 ? sel : last;
}

// the wave's staged tile (64 lanes x len words, stride `stride`) -> out[(p0 + l) row + off + i]: consecutive lanes
// write consecutive addresses
template <typename T>
__device__ __forceinline__ void gs_flush(const T* __restrict__ stg, int stride, int len, T* __restrict__ out,
                                         int64_t p0, int64_t P, int64_t row, int64_t off, int lane) {
  const unsigned total = 64u * (unsigned)len;
  for (unsigned e = lane; e < total; e += 64) {
    const unsigned l = e / (unsigned)len, i = e - l * (unsigned)len;
    if (p0 + l < P) out[(p0 + l) * row + off + i] = stg[l * stride + i];
  }
}

__device__ __forceinline__ void gs_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
}  // namespace

// FULL: scale = (S,D,D) lower Cholesky factors, DP = D rounded up to 4 / 8 / 16 / 32 (the eps registers);
// diagonal: scale = (S,D) standard deviations, DP unused.
template <bool FULL, int DP>
__global__ __launch_bounds__(256) void gauss_scenario_kernel(ScenArgs a) {
  extern __shared__ double gs_smem[];
  double* turn = gs_smem;
  float* fl = reinterpret_cast<float*>(gs_smem + a.nturn);
  float* Ae = fl;
  float* tot = fl + a.oTot;
  float* mean = fl + a.oMean;
  float* scale = fl + a.oScale;
  float* port = fl + a.oPort;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, D = a.D, H = a.H, SA = a.SA, SD = a.SD, SL = a.SL;
  const bool want_w = a.port != nullptr;

  // ---- parameters -> LDS
  for (int k = tid; k < S * S; k += nthr) Ae[(k / S) * SA + k % S] = expf(a.log_A[k]);
  if (tid < S) {
    float run = 0.f;
    for (int k = 0; k < S; ++k) run += expf(a.log_A[tid * S + k]);
    tot[tid] = run;
  }
  for (int k = tid; k < S * D; k += nthr) {
    const int s = k / D, d = k - s * D;
    mean[s * SD + d] = a.mean[k];
    if (!FULL) scale[s * SD + d] = a.scale[k];
    if (want_w) port[s * SD + d] = a.port[k];
  }
  if (FULL) {
    for (int k = tid; k < S * D * D; k += nthr) {
      const int s = k / (D * D), r = k - s * D * D, i = r / D, j = r - i * D;
      if (j <= i) scale[s * SL + gs_tri(i) + j] = a.scale[k];
    }
  }
  if (want_w) {
    for (int k = tid; k < (S + 1) * S; k += nthr) {
      const int h = k / S, z = k - h * S;   // h = 0: nothing held, else row h - 1
      double acc = 0.0;
      for (int d = 0; d < D; ++d)
        acc += fabs((double)a.port[z * D + d] - (h ? (double)a.port[(h - 1) * D + d] : 0.0));
      turn[k] = acc;
    }
  }
  __syncthreads();

  // ---- the wave's staging tiles
  float* stage = fl + a.oStage + wave * a.wstage;
  int32_t* st_states = reinterpret_cast<int32_t*>(stage);
  float* st_wealth = stage + (a.states ? 64 * GS_TSTR : 0);
  float* st_x = st_wealth + (a.wealth ? 64 * GS_TSTR : 0);

  const int64_t p0 = (int64_t)blockIdx.x * nthr + wave * 64;   // the wave's first path
  if (p0 >= a.P) return;                                       // the whole wave: no barrier follows
  const int64_t p = p0 + lane;
  const bool live = p < a.P;
  const int64_t pc = live ? p : a.P - 1;   // a dead lane replays the last path and writes nothing
  const int64_t b = pc / a.N, n = pc - b * a.N;
  const uint32_t c0 = a.n0 + (uint32_t)n, c1 = a.b0 + (uint32_t)b;
  const uint32_t k0 = a.k0, k1 = a.k1;
  const float NaN = __builtin_nanf("");

  int z = 0, held = 0 /* row of turn: 0 = nothing, else 1 + regime */, rc = 0, ts = 0, tx = 0;
  bool bad = false;
  double w = 1.0, peak = 1.0, dd = 0.0;
  const double txc = (double)a.tx;

  for (int t = 0; t < H; ++t) {
    // ---- the regime
    uint32_t o[4];
    gs_philox<!FULL>(c0, c1, (uint32_t)t, 0u, k0, k1, o);
    const float u = (float)(o[0] >> 8) * 0x1p-24f;
    if (t == 0) {
      const float* sp = a.start + b * S;
      float total = 0.f;
      for (int k = 0; k < S; ++k) {
        const float pk = sp[k];
        bad |= !(pk >= 0.f && pk < __builtin_inff());
        total += pk;
      }
      bad |= !(total > 0.f && total < __builtin_inff());
      z = gs_draw(sp, S, total, u);
    } else {
      const float total = tot[z];
      bad |= !(total > 0.f && total < __builtin_inff());
      z = gs_draw(Ae + z * SA, S, total, u);
    }
    if (a.states) st_states[lane * GS_TSTR + ts] = bad ? -1 : z;

    // ---- rebalance
    if (want_w) {
      if (rc == 0) {
        w -= w * txc * turn[held * S + z];
        held = z + 1;
        rc = a.reb;
      }
      --rc;
    }
    const float* hp = port + (held - 1) * SD;   // held >= 1 from step 0 on
    double pr = 0.0;

    // ---- the returns
    if constexpr (FULL) {
      float eps[DP];
#pragma unroll
      for (int jb = 0; jb < DP / 4; ++jb) {
        if (jb * 4 < D) {
          float e[4];
          gs_normals4<!FULL>(c0, c1, (uint32_t)t, 1u + jb, k0, k1, e);
          eps[4 * jb] = e[0]; eps[4 * jb + 1] = e[1]; eps[4 * jb + 2] = e[2]; eps[4 * jb + 3] = e[3];
        }
      }
      const float* Lz = scale + z * SL;
      const float* mz = mean + z * SD;
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        if (i < D) {
          float acc = mz[i];
#pragma unroll
          for (int j = 0; j <= i; ++j) acc = fmaf(Lz[gs_tri(i) + j], eps[j], acc);
          const float xv = bad ? NaN : acc;
          if (a.x) st_x[lane * a.XS + tx * D + i] = xv;
          if (want_w) pr += (double)hp[i] * (double)xv;
        }
      }
    } else {
      const float* sz = scale + z * SD;
      const float* mz = mean + z * SD;
      for (int jb = 0; jb * 4 < D; ++jb) {
        float e[4];
        gs_normals4<!FULL>(c0, c1, (uint32_t)t, 1u + jb, k0, k1, e);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int d = 4 * jb + q;
          if (d < D) {
            const float acc = fmaf(sz[d], e[q], mz[d]);
            const float xv = bad ? NaN : acc;
            if (a.x) st_x[lane * a.XS + tx * D + d] = xv;
            if (want_w) pr += (double)hp[d] * (double)xv;
          }
        }
      }
    }

    // ---- wealth
    if (want_w) {
      w *= 1.0 + pr;
      if (a.wealth) st_wealth[lane * GS_TSTR + ts] = (float)w;   // NaN on a failed path: pr is
      if (w > peak) peak = w;
      if (w < peak) dd = fmax(dd, 1.0 - w / peak);
    }

    // ---- whole runs leave
    const bool end = t == H - 1;
    if ((a.states || a.wealth) && (ts == GS_TS - 1 || end)) {
      gs_wave_sync();
      if (a.states) gs_flush(st_states, GS_TSTR, ts + 1, a.states, p0, a.P, (int64_t)H, (int64_t)(t - ts), lane);
      if (a.wealth) gs_flush(st_wealth, GS_TSTR, ts + 1, a.wealth, p0, a.P, (int64_t)H, (int64_t)(t - ts), lane);
      gs_wave_sync();
      ts = -1;
    }
    ++ts;
    if (a.x && (tx == a.xts - 1 || end)) {
      gs_wave_sync();
      gs_flush(st_x, a.XS, (tx + 1) * D, a.x, p0, a.P, (int64_t)H * D, (int64_t)(t - tx) * D, lane);
      gs_wave_sync();
      tx = -1;
    }
    ++tx;
  }
  if (live) {
    if (a.fin) a.fin[p] = (float)w;
    if (a.dd) a.dd[p] = bad ? NaN : (float)dd;
  }
}

template <bool FULL, int DP>
static int gs_launch(const ScenArgs& a, int nw, size_t lds, hipStream_t s) {
  auto kern = gauss_scenario_kernel<FULL, DP>;
  if (lds > 64 * 1024) {
    // more than 64 KB of dynamic LDS has to be asked for, once per kernel
    static const hipError_t big_lds = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GS_LDS_MAX);
    (void)big_lds;
  }
  kern<<<(unsigned)cdiv(a.P, nw * 64), nw * 64, lds, s>>>(a);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

bool hmm_gauss_scenario_supported(int64_t B, int64_t N, int64_t H, int64_t S, int64_t D, int full) {
  if (!(full ? hmm_gauss_full_supported(S, D) : hmm_gauss_supported(S, D))) return false;
  if (!(H <= GS_MAX_H && B <= GS_MAX_PATHS && N <= GS_MAX_PATHS && (B == 0 || N <= GS_MAX_PATHS / B))) return false;
  return B * N == 0 || H <= GS_MAX_STEPS / (B * N);
}

int launch_hmm_gauss_scenario(const float* start, const float* log_A, const float* mean, const float* scale, int full,
                              const float* port, int64_t rebalance, float tx_cost, uint64_t seed, int64_t b0,
                              int64_t n0, int64_t B, int64_t N, int64_t H, int64_t S, int64_t D, int32_t* states,
                              float* x, float* wealth, float* final_wealth, float* drawdown, hipStream_t s) {
  if (!hmm_gauss_scenario_supported(B, N, H, S, D, full)) return VQHMM_EUNSUPPORTED;
  if (B == 0 || N == 0 || H == 0) return VQHMM_OK;
  ScenArgs a;
  a.start = start; a.log_A = log_A; a.mean = mean; a.scale = scale; a.port = port;
  a.states = states; a.x = x; a.wealth = wealth; a.fin = final_wealth; a.dd = drawdown;
  a.N = N; a.P = B * N;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.b0 = (uint32_t)b0; a.n0 = (uint32_t)n0;
  a.H = (int)H; a.S = (int)S; a.D = (int)D;
  a.reb = (int)(rebalance < GS_MAX_H ? rebalance : GS_MAX_H);   // H <= 2^28: a longer period rebalances at t = 0 only
  a.tx = tx_cost;
  const int Si = (int)S, Di = (int)D;
  a.nturn = port ? (Si + 1) * Si : 0;
  a.SA = gs_odd(Si); a.SD = gs_odd(Di); a.SL = full ? gs_odd(gs_tri(Di)) : a.SD;
  a.oTot = Si * a.SA;
  a.oMean = a.oTot + Si;
  a.oScale = a.oMean + Si * a.SD;
  a.oPort = a.oScale + Si * a.SL;
  a.oStage = a.oPort + (port ? Si * a.SD : 0);
  a.xts = (int)cdiv(32, Di);
  a.XS = gs_odd(a.xts * Di);
  a.wstage = (states ? 64 * GS_TSTR : 0) + (wealth ? 64 * GS_TSTR : 0) + (x ? 64 * a.XS : 0);
  // 4 waves per workgroup while two workgroups fit a CU's LDS, else 2, else 1 (which always fits)
  int nw = 4;
  auto bytes = [&](int w) { return (size_t)a.nturn * 8 + (size_t)(a.oStage + w * a.wstage) * 4; };
  while (nw > 1 && bytes(nw) > GS_LDS_SOFT) nw >>= 1;
  const size_t lds = bytes(nw);
  if (lds > GS_LDS_MAX) return VQHMM_EUNSUPPORTED;   // not reached inside the domain (<= 72 KB at nw = 1)
  if (!full) return gs_launch<false, 0>(a, nw, lds, s);
  if (D <= 4) return gs_launch<true, 4>(a, nw, lds, s);
  if (D <= 8) return gs_launch<true, 8>(a, nw, lds, s);
  if (D <= 16) return gs_launch<true, 16>(a, nw, lds, s);
  return gs_launch<true, 32>(a, nw, lds, s);
}

}  // namespace vqhmm
