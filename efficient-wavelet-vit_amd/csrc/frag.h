// Register fragments of v_mfma_f32_16x16x32_bf16 (gfx950): lane l = 16 g + r holds row (A) /
// column (B) r, K elements 8 g .. 8 g + 7 of the 32-wide step, as 8 bf16; the 16 x 16 result has
// rows 4 g .. 4 g + 3 of column r in the lane's 4 floats.  What vit.hip, head.hip and the tall-K
// GEMM share to load, form and multiply them.
#pragma once
#include "common.h"
#include "mx8.h"

namespace ewvit {

typedef __attribute__((ext_vector_type(8))) __bf16 vb8;
typedef __attribute__((ext_vector_type(4))) float vf4;

__device__ __forceinline__ vf4 mma(vb8 a, vb8 b, vf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ vb8 pack8(const float *v) {
  vb8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (__bf16)v[e];
  return r;
}
__device__ __forceinline__ void ld8f(const float *p, float *v) {
  const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ vb8 ld8b(const bf16_t *p) { return *reinterpret_cast<const vb8 *>(p); }
__device__ __forceinline__ void unpack8(vb8 b, float *v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)b[e];
}
__device__ __forceinline__ vb8 zero8() {
  vb8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (__bf16)0.f;
  return r;
}
__device__ __forceinline__ float rbf(float v) { return bf2f(f2bf(v)); }
// rows >= R are loaded from row R - 1 (in bounds) and masked after the load: a load under a
// per-lane branch gets its own block and waits, so the epilogues' loads would run one by one
__device__ __forceinline__ int rclamp(int r, int R) { return r < R ? r : R - 1; }

// An MX operand fragment (mx8.h) of one 128-wide K step, quantized in registers: a8(k, dst)
// yields the lane's row at K offsets k .. k + 7 of the step (zeros for rows past the matrix)
template <class A8>
__device__ __forceinline__ MxFrag mx_fill(A8 a8) {
  const int lane = threadIdx.x & 63;
  float v[32];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int q = 0; q < 2; ++q) a8((hh ? mx_k1(lane) : mx_k0(lane)) + 8 * q, v + hh * 16 + q * 8);
  return mx_quant(v);
}

// A GEMM body written once for both operand forms: 128 of K are frag_steps<MX> fragments of
// frag_t<MX> per row tile (4 bf16 k-steps of 32, lane K offset 32 u + 8 (lane >> 4), or one MX step)
template <bool MX> using frag_t = std::conditional_t<MX, MxFrag, vb8>;
template <bool MX> constexpr int frag_steps = MX ? 1 : 4;
__device__ __forceinline__ vf4 mma(const MxFrag &a, const MxFrag &b, vf4 c) { return mx_mma(a, b, c); }

}  // namespace ewvit
