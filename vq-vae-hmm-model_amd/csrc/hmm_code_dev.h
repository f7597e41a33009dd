// Device code shared by the kernels of the stationary HMM on code indices (hmm_code.hip: E-step and sampler;
// hmm_code_decode.hip: Viterbi decode and causal filter): the lane helpers of the "one sequence per wave,
// lane j = state j" map, the range of a fast (linear) step and the prologue that builds the (V, S)
// exp(log_B)^T emission table both tiers read.
#pragma once
#include <math.h>

#include "kernels.h"

namespace vqhmm {

namespace {

constexpr float CE_NEG_INF = -__builtin_huge_valf();
constexpr double CE_LN2 = 0.69314718055994531;
constexpr float CE_LO = 0x1p-30f, CE_HI = 0x1p30f;  // a fast step's mass must stay inside
constexpr int CE_CH = 64;                           // steps per chunk (one code per lane)

__device__ __forceinline__ float ce_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }
__device__ __forceinline__ int ce_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float ce_uni(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ float ce_lane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
template <int CTRL>
__device__ __forceinline__ float ce_dpp(float v) {
  return __builtin_bit_cast(float, dpp_u32<CTRL>(__builtin_bit_cast(uint32_t, v)));
}
struct CeAdd { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct CeMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };
// all-reduce over lanes [0, SP) (wave_sum_dpp's first log2(SP) steps): every lane of the group ends with the
// same bits; lanes in [S, SP) must hold the operation's identity
template <int SP, typename Op>
__device__ __forceinline__ float ce_red(float v, Op op) {
  if constexpr (SP >= 2) v = op(v, ce_dpp<0xB1>(v));    // quad_perm [1,0,3,2]
  if constexpr (SP >= 4) v = op(v, ce_dpp<0x4E>(v));    // quad_perm [2,3,0,1]
  if constexpr (SP >= 8) v = op(v, ce_dpp<0x141>(v));   // row_half_mirror
  if constexpr (SP >= 16) v = op(v, ce_dpp<0x128>(v));  // row_ror:8
  if constexpr (SP >= 32) {
    const float2 r = pair16(v);
    v = op(r.x, r.y);
  }
  return v;
}

// blockIdx.y = the member of a stack of models (hmm_code.hip's batched E-step): its log_B lies lb_stride floats
// and its table bt_stride floats after the previous member's
__global__ __launch_bounds__(256) void code_bt_kernel(const float* __restrict__ log_B, int S, int V,
                                                      float* __restrict__ Bt, int64_t lb_stride = 0,
                                                      int64_t bt_stride = 0) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= (int64_t)S * V) return;
  log_B += blockIdx.y * lb_stride;
  Bt += blockIdx.y * bt_stride;
  const int v = (int)(k / S), s = (int)(k - (int64_t)v * S);
  Bt[k] = __expf(log_B[(int64_t)s * V + v]);
}

inline size_t r256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

}  // namespace vqhmm
