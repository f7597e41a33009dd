// Codebook learning for the VQ half (pseudocode.txt:8-32): per-code statistics of a batch under given
// assignments, the quantizer's backward from the same pass, and the channels-first lookup (contracts in
// include/vqhmm.h, fp64 restatement in tests/vq_codebook_ref.py; DESIGN.md "Codebook learning").
//
//   in      z (B,Dv,T) channels-first, idx (B,T) int32, lengths (B) int64 (nullable), codebook (K,Dv)
//   counts  a position (b,t) counts when t < clamp(lengths[b], 0, T) and 0 <= idx[b,t] < K; its residual is
//           r_d = fl32(z[b,d,t] - c[idx][d])
//   stats   count[k] = #counted positions with idx = k, rsum[k,d] = sum r_d over them, sse = sum r_d^2 (fp64)
//   bwd     dz[b,d,t] = fl(g + fl(s r_d)) (r_d = 0 where the position does not count), dcodebook = scale * rsum
//
// Lane map.  A workgroup of 4 waves walks a contiguous range of 64-position tiles, one tile at a time, with
// ONE fp64 slab (K Dv + K + 1 doubles: rsum, count, sse).  The tile's channels go through LDS in chunks of
// 64, in three phases between workgroup barriers:
//   stage   wave w loads rows 16 w .. 16 w + 15 of the chunk, each one coalesced load (lane = position),
//           all in flight together, and stores them at stride 65
//   turn    the chunk is read the other way, lane j = channel d0 + j, and becomes its residuals in place
//           (0 at positions that do not count): wave w takes positions 16 w .. 16 w + 15, whose codebook
//           rows are in flight together; the position's code is wave-uniform (v_readlane of the lane that
//           loaded it); sse accumulates per lane in fp64
//   walk    wave w owns the codes k = w (mod 4).  It walks the tile's positions with one of its codes
//           serially, in position order (the set bits of a ballot), and every lane does a plain fp64
//           read-add-write on bin (k, d): a bin has one owning lane of one owning wave, so there is no
//           atomic anywhere and the order of the additions into a bin is the positions' order.  Four
//           positions at a time: when a scalar test finds their codes pairwise distinct the four bins' reads
//           go out together ahead of the four writes.  Lane 0 of the owning wave counts the position.
//           The backward form's row stores dz = g + s r (coalesced, wave w rows 16 w ..) run beside the walk;
//           both only read the chunk.
//
// Tiers.  The slab lives in LDS when it fits beside the chunk (LDS tier) and in the workgroup's own partial
// in the workspace otherwise (L2 tier, partial bytes capped); small slabs leave room for several workgroups
// per CU.
//
// Reduction.  Tiles are assigned statically (workgroup g takes tiles [g per, (g + 1) per)), the workgroup's
// slab is its partial, and a second launch sums the partials in fp64 in a fixed order (hmm_code.hip's
// code_reduce_kernel order): the same bits run to run.  The second launch also writes dcodebook.
//
// Addressing.  z, g_zq and dz are touched only at t < T (the tail lanes are masked, not loaded and dropped),
// idx only at t < length, the codebook only at rows in [0, K).
#include "kernels.h"

namespace vqhmm {

namespace {

constexpr int VC_TP = 64;                           // positions per tile = channels per chunk
constexpr int VC_LD = VC_TP + 1;                    // padded stride: row stores and column reads conflict-free
constexpr size_t VC_STAGE = VC_TP * VC_LD * 4;      // bytes of the chunk
constexpr int VC_NW = 4;                            // waves per workgroup (a power of two: codes k & 3 = wave)
constexpr int VC_PW = VC_TP / VC_NW;                // rows (stage) / positions (turn) per wave
constexpr size_t VC_LDS_MAX = 156 * 1024;           // of the CU's 160 KB
constexpr int64_t VC_MAX_WG = 1024;                 // workgroups (partials) at most
constexpr size_t VC_PART_CAP = size_t(64) << 20;    // bytes of partials at most
constexpr int VC_CB = 4;                            // walk: positions whose bins are in flight together

struct VcArgs {
  const float* z;
  const int32_t* idx;
  const int64_t* lengths;  // nullable
  const float* cb;
  const float* g_zq;      // nullable
  const float* dz_scale;  // BWD
  float* dz;              // BWD
  int64_t B, T, tps, ntile, per;  // tiles per sequence, tiles, tiles per workgroup
  int Dv, K;
  double* part;  // [gridDim.x][K*Dv rsum + K count + 1 sse]
};

__device__ __forceinline__ int vc_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <bool LDS_T, bool BWD>
__global__ __launch_bounds__(64 * VC_NW) void vq_codebook_kernel(const VcArgs a) {
  extern __shared__ double vc_smem[];
  const int Dv = a.Dv, K = a.K;
  const int64_t T = a.T;
  const int64_t KD = (int64_t)K * Dv, NE = KD + K + 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = vc_uni(tid >> 6);
  // LDS: [slab NE doubles (LDS tier)] [chunk 64 x 65 floats]
  float* stage = reinterpret_cast<float*>(vc_smem + (LDS_T ? NE : 0));
  double* part = a.part + (int64_t)blockIdx.x * NE;
  double* slab = LDS_T ? vc_smem : part;
  for (int64_t k = tid; k < NE; k += 64 * VC_NW) slab[k] = 0.0;
  if constexpr (!LDS_T) __threadfence();
  __syncthreads();
  double* cnt = slab + KD;
  double sse = 0.0;
  float sc = 0.f;
  if constexpr (BWD) sc = *a.dz_scale;

  const int64_t tl0 = (int64_t)blockIdx.x * a.per;
  const int64_t tl1 = tl0 + a.per < a.ntile ? tl0 + a.per : a.ntile;
  int64_t b = tl0 / a.tps, ti = tl0 - b * a.tps;
  for (int64_t tl = tl0; tl < tl1; ++tl, ++ti) {
    if (ti == a.tps) {
      ti = 0;
      ++b;
    }
    // everything up to the chunk loop is the same in the four waves, so they skip a tile together
    const int64_t t0 = ti * VC_TP;
    const int64_t Lr = a.lengths ? a.lengths[b] : T;
    const int64_t L = Lr <= 0 ? 0 : (Lr < T ? Lr : T);
    if (!BWD && t0 >= L) continue;
    int kv = -1;  // the lane's position's code, -1 where it does not count
    if (t0 + lane < L) {
      const int c = a.idx[b * T + t0 + lane];
      kv = (c >= 0 && c < K) ? c : -1;
    }
    if (!BWD && __builtin_amdgcn_ballot_w64(kv >= 0) == 0) continue;
    const int n = (int)(T - t0 < VC_TP ? T - t0 : VC_TP);  // positions of the tile inside T
    const uint64_t mine = __builtin_amdgcn_ballot_w64(kv >= 0 && (kv & (VC_NW - 1)) == wave);

    for (int d0 = 0; d0 < Dv; d0 += VC_TP) {
      const int nd = Dv - d0 < VC_TP ? Dv - d0 : VC_TP;
      const int64_t row0 = (b * Dv + d0) * T + t0;
      const int c0 = wave * VC_PW;  // the wave's rows (stage, dz) and positions (turn)
      // stage: the wave's rows, coalesced, all in flight together
      {
        float v[VC_PW];
#pragma unroll
        for (int q = 0; q < VC_PW; ++q)
          v[q] = (c0 + q < nd && lane < n) ? a.z[row0 + (int64_t)(c0 + q) * T + lane] : 0.f;
#pragma unroll
        for (int q = 0; q < VC_PW; ++q)
          if (c0 + q < nd) stage[(c0 + q) * VC_LD + lane] = v[q];
      }
      __syncthreads();

      const bool dact = lane < nd;
      const int d = d0 + (dact ? lane : 0);
      float* col = stage + (dact ? lane : 0) * VC_LD;
      // turn: the wave's positions become their residuals in place, no dependence between positions
      if (c0 < n) {
        float c[VC_PW];
#pragma unroll
        for (int q = 0; q < VC_PW; ++q) {
          const int k = __builtin_amdgcn_readlane(kv, c0 + q);
          c[q] = dact ? a.cb[(int64_t)(k < 0 ? 0 : k) * Dv + d] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < VC_PW; ++q) {
          const int k = __builtin_amdgcn_readlane(kv, c0 + q);
          if (dact) {
            const float r = k >= 0 ? col[c0 + q] - c[q] : 0.f;
            col[c0 + q] = r;
            sse += (double)r * (double)r;
          }
        }
      }
      __syncthreads();

      // walk: the positions with one of the wave's codes, in position order, 4 at a time
      const bool first = d0 == 0 && lane == 0;  // the tile's counts: one lane, once per tile
      for (uint64_t m = mine; m != 0;) {
        int s[VC_CB], k[VC_CB];
#pragma unroll
        for (int q = 0; q < VC_CB; ++q) {
          s[q] = m != 0 ? (int)__builtin_ctzll(m) : -1;
          k[q] = s[q] >= 0 ? __builtin_amdgcn_readlane(kv, s[q]) : -1;
          m &= m - 1;  // 0 stays 0
        }
        bool distinct = k[VC_CB - 1] >= 0;  // a full batch
#pragma unroll
        for (int q = 1; q < VC_CB; ++q) {
#pragma unroll
          for (int p = 0; p < q; ++p) distinct = distinct && k[p] != k[q];
        }
        if (distinct) {
          // four different bins: the reads go out together, the writes follow
          if (dact) {
            double bv[VC_CB];
#pragma unroll
            for (int q = 0; q < VC_CB; ++q) bv[q] = slab[(int64_t)k[q] * Dv + d];
#pragma unroll
            for (int q = 0; q < VC_CB; ++q) slab[(int64_t)k[q] * Dv + d] = bv[q] + (double)col[s[q]];
          }
          if (first) {
            double cn[VC_CB];
#pragma unroll
            for (int q = 0; q < VC_CB; ++q) cn[q] = cnt[k[q]];
#pragma unroll
            for (int q = 0; q < VC_CB; ++q) cnt[k[q]] = cn[q] + 1.0;
          }
        } else {
#pragma unroll
          for (int q = 0; q < VC_CB; ++q) {
            if (k[q] < 0) continue;
            if (dact) {
              double* bin = slab + ((int64_t)k[q] * Dv + d);
              *bin = *bin + (double)col[s[q]];
            }
            if (first) cnt[k[q]] = cnt[k[q]] + 1.0;
          }
        }
      }

      if constexpr (BWD) {
        if (lane < n) {
          float g[VC_PW];
#pragma unroll
          for (int q = 0; q < VC_PW; ++q)
            g[q] = (c0 + q < nd && a.g_zq) ? a.g_zq[row0 + (int64_t)(c0 + q) * T + lane] : 0.f;
#pragma unroll
          for (int q = 0; q < VC_PW; ++q) {
            if (c0 + q < nd) {
              const float p = sc * stage[(c0 + q) * VC_LD + lane];
              a.dz[row0 + (int64_t)(c0 + q) * T + lane] = g[q] + p;
            }
          }
        }
      }
      __syncthreads();  // the next chunk's row stores come after every wave's reads of this one
    }
  }

  // the workgroup's sse: its threads' sums in thread order
  {
    double* sl = reinterpret_cast<double*>(stage);
    sl[tid] = sse;
    __syncthreads();
    if (tid == 0) {
      double acc = 0.0;
      for (int q = 0; q < 64 * VC_NW; ++q) acc += sl[q];
      slab[KD + K] = acc;
    }
  }
  // the workgroup's partial is its slab
  if constexpr (LDS_T) {
    __syncthreads();
    for (int64_t k = tid; k < NE; k += 64 * VC_NW) part[k] = slab[k];
  }
}

// out = sum over the partials in a fixed order (code_reduce_kernel's: thread (py, kx) adds partials py,
// py + 16, .. of element kx in index order, then the 16 sums are added in py order); rsum / count / sse are
// nullable, dcb (nullable) = (float)(*dcb_scale * rsum)
constexpr int VC_RK = 16, VC_RP = 16;
__global__ __launch_bounds__(VC_RK * VC_RP) void vq_codebook_reduce_kernel(const double* __restrict__ part, int np,
                                                                           int64_t KD, int K,
                                                                           double* __restrict__ count,
                                                                           double* __restrict__ rsum,
                                                                           double* __restrict__ sse,
                                                                           const float* __restrict__ dcb_scale,
                                                                           float* __restrict__ dcb) {
  __shared__ double red[VC_RP][VC_RK];
  const int64_t NE = KD + K + 1;
  const int kx = threadIdx.x % VC_RK, py = threadIdx.x / VC_RK;
  const int64_t k = (int64_t)blockIdx.x * VC_RK + kx;
  double acc = 0.0;
  if (k < NE) {
#pragma unroll 4
    for (int p = py; p < np; p += VC_RP) acc += part[(int64_t)p * NE + k];
  }
  red[py][kx] = acc;
  __syncthreads();
  if (py != 0 || k >= NE) return;
  acc = 0.0;
#pragma unroll
  for (int q = 0; q < VC_RP; ++q) acc += red[q][kx];
  if (k < KD) {
    if (rsum) rsum[k] = acc;
    if (dcb) dcb[k] = (float)((double)*dcb_scale * acc);
  } else if (k < KD + K) {
    if (count) count[k - KD] = acc;
  } else if (sse) {
    *sse = acc;
  }
}

// out[b,d,t] = codebook[idx[b,t]][d], 0 where idx is outside [0, K): a thread per position, stores
// coalesced along t
__global__ __launch_bounds__(256) void vq_lookup_kernel(const float* __restrict__ cb, int K, int Dv,
                                                        const int32_t* __restrict__ idx, int64_t T, int64_t tpb,
                                                        float* __restrict__ out) {
  const int64_t b = blockIdx.x / tpb;
  const int64_t t = (blockIdx.x - b * tpb) * 256 + threadIdx.x;
  if (t >= T) return;
  const int k = idx[b * T + t];
  const bool ok = k >= 0 && k < K;
  const float* row = cb + (int64_t)(ok ? k : 0) * Dv;
  float* o = out + b * Dv * T + t;
#pragma unroll 4
  for (int d = 0; d < Dv; ++d) o[(int64_t)d * T] = ok ? row[d] : 0.f;
}

struct VcPlan {
  bool lds;
  int64_t nblk, tps, ntile, per;
  size_t lds_bytes, bytes;
};

VcPlan vc_plan(int64_t B, int64_t Dv, int64_t T, int64_t K) {
  VcPlan p;
  const size_t NE = (size_t)K * Dv + K + 1;
  p.lds = NE * 8 + VC_STAGE <= VC_LDS_MAX;
  p.tps = cdiv(T, VC_TP);
  p.ntile = B * p.tps;
  int64_t cap = (int64_t)(VC_PART_CAP / (NE * 8));
  cap = cap < 1 ? 1 : cap > VC_MAX_WG ? VC_MAX_WG : cap;
  p.nblk = p.ntile < 1 ? 1 : p.ntile > cap ? cap : p.ntile;
  p.per = cdiv(p.ntile, p.nblk);
  p.lds_bytes = (p.lds ? NE * 8 : 0) + VC_STAGE;
  p.bytes = (size_t)p.nblk * NE * 8;
  return p;
}

template <bool BWD>
int vc_go(const VcArgs& a, const VcPlan& p, hipStream_t s) {
  if (p.lds) {
    auto kern = vq_codebook_kernel<true, BWD>;
    // more than 64 KB of dynamic LDS has to be asked for, once per kernel (the tier's limit covers every launch)
    static const hipError_t big_lds = hipFuncSetAttribute(
        reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)VC_LDS_MAX);
    (void)big_lds;
    kern<<<(unsigned)p.nblk, 64 * VC_NW, p.lds_bytes, s>>>(a);
  } else {
    vq_codebook_kernel<false, BWD><<<(unsigned)p.nblk, 64 * VC_NW, p.lds_bytes, s>>>(a);
  }
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

}  // namespace

bool vq_codebook_supported(int64_t Dv, int64_t K) {
  return K >= 1 && K <= 65536 && Dv >= 1 && Dv <= 512 && K * Dv <= (int64_t(1) << 21);
}

size_t vq_codebook_ws_bytes(int64_t B, int64_t Dv, int64_t T, int64_t K) {
  if (!vq_codebook_supported(Dv, K) || B < 0 || T < 0) return 0;
  return vc_plan(B, Dv, T, K).bytes;
}

int launch_vq_codebook(const float* z, const int32_t* idx, const int64_t* lengths, int64_t B, int64_t Dv, int64_t T,
                       const float* cb, int64_t K, double* count, double* rsum, double* sse, const float* g_zq,
                       const float* dz_scale, const float* dcb_scale, float* dz, float* dcb, void* ws,
                       hipStream_t s) {
  if (!vq_codebook_supported(Dv, K) || B > INT32_MAX || cdiv(T, VC_TP) > INT32_MAX) return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) {
    if ((count && hipMemsetAsync(count, 0, sizeof(double) * K, s) != hipSuccess) ||
        (rsum && hipMemsetAsync(rsum, 0, sizeof(double) * K * Dv, s) != hipSuccess) ||
        (sse && hipMemsetAsync(sse, 0, sizeof(double), s) != hipSuccess) ||
        (dcb && hipMemsetAsync(dcb, 0, sizeof(float) * K * Dv, s) != hipSuccess))
      return VQHMM_ELAUNCH;
    return VQHMM_OK;
  }
  const VcPlan p = vc_plan(B, Dv, T, K);
  VcArgs a;
  a.z = z; a.idx = idx; a.lengths = lengths; a.cb = cb;
  a.g_zq = g_zq; a.dz_scale = dz_scale; a.dz = dz;
  a.B = B; a.T = T; a.tps = p.tps; a.ntile = p.ntile; a.per = p.per;
  a.Dv = (int)Dv; a.K = (int)K;
  a.part = static_cast<double*>(ws);
  const int rc = dz ? vc_go<true>(a, p, s) : vc_go<false>(a, p, s);
  if (rc) return rc;
  const int64_t NE = K * Dv + K + 1;
  vq_codebook_reduce_kernel<<<(unsigned)cdiv(NE, VC_RK), VC_RK * VC_RP, 0, s>>>(a.part, (int)p.nblk, K * Dv, (int)K,
                                                                               count, rsum, sse, dcb_scale, dcb);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

int launch_vq_lookup(const float* cb, int64_t K, int64_t Dv, const int32_t* idx, int64_t B, int64_t T, float* out,
                     hipStream_t s) {
  if (!vq_codebook_supported(Dv, K)) return VQHMM_EUNSUPPORTED;
  if (B == 0 || T == 0) return VQHMM_OK;
  const int64_t tpb = cdiv(T, 256);
  if (B * tpb > INT32_MAX) return VQHMM_EUNSUPPORTED;
  vq_lookup_kernel<<<(unsigned)(B * tpb), 256, 0, s>>>(cb, (int)K, (int)Dv, idx, T, tpb, out);
  VQHMM_LAUNCH_CHECK();
  return VQHMM_OK;
}

}  // namespace vqhmm
