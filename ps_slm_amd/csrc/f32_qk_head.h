// fp32 rotation and Qwen3 head norm shared by csrc/fp32.hip (the rotation kernels, the K-range-slab finishers) and csrc/qk_norm.hip
// (the fp32 row kernels): ONE device function per step, so that a key appended at decode time, a key out of a prefill and a key
// out of the fused q|k|v finisher carry the same bits.
#pragma once
#include "common.h"

namespace tasu_f32 {

// x * cos + rotate_half(x) * sin with the two products and the sum rounded separately, like torch eager (apply_rotary_pos_emb):
// -ffp-contract=fast would otherwise fuse one product into the sum, and not the same one at every call site
__device__ __forceinline__ void rope_pair_eager(float x1, float x2, float c, float s, float& y1, float& y2) {
  // (every product passes through an empty asm before it is used: a pragma `fp contract(off)` here did not survive inlining into
  // f32_sum_slabs_rope_kernel, which came out with a v_pk_fma_f32 where f32_rope_kernel has mul + add)
  float a1 = x1 * c, b1 = x2 * s, a2 = x2 * c, b2 = x1 * s;
  asm volatile("" : "+v"(a1), "+v"(b1), "+v"(a2), "+v"(b2));
  y1 = a1 - b1;
  y2 = a2 + b2;
}

// Thread map of the fp32 head kernels: 32 lanes per (row, head), 4 contiguous elements (one 16-byte vector) per lane; lanes 0-15
// hold dims 0..63, lanes 16-31 dims 64..127, so the rotate-half partner of a lane's vector is lane ^ 16's and the mean is five
// xor-shuffles inside the 32-lane group (a wave serves 2 heads, a 256-thread block 8).
constexpr int QK_LANES = 32, QK_HEADS_PER_BLOCK = 256 / QK_LANES;

__device__ __forceinline__ float group32_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One lane's share of one q / k head in HF's Qwen3RMSNorm on fp32 tensors, then apply_rotary_pos_emb:
//   r = rsqrt(mean_128(x^2) + eps);  y = w * (x * r) (two rounded products);  out = rope(y) (rope_pair_eager).
// x = the lane's 4 elements, w = the head's norm weight at those dims, (cs, sn) = the row's table at the lane's 4 pair indices,
// sub = lane & 31.  The sum of squares: 4 serial FMAs per lane, then the shuffles -- the same order wherever this is inlined.
__device__ __forceinline__ f32x4 f32_qk_head_fwd(const f32x4 x, const float* __restrict__ w, const float* __restrict__ cs,
                                                 const float* __restrict__ sn, float eps, int sub, float& r) {
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) ss = __builtin_fmaf(x[j], x[j], ss);
  ss = group32_sum(ss);
  r = rsqrtf(__builtin_fmaf(ss, 1.0f / 128, eps));          // (the scaling is exact: one rounding, fused or not)
  const f32x4 wv = *(const f32x4*)w, c = *(const f32x4*)cs, s = *(const f32x4*)sn;
  const bool hi = sub >= 16;
  f32x4 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float y = wv[j] * (x[j] * r);
    const float other = __shfl_xor(y, 16, 64);              // the rotate-half partner (dim ^ 64)
    float y1, y2;
    rope_pair_eager(hi ? other : y, hi ? y : other, c[j], s[j], y1, y2);
    out[j] = hi ? y2 : y1;
  }
  return out;
}

}  // namespace tasu_f32
