// Per-head q/k RMSNorm of the Qwen3 decoders (modeling_qwen3.py: Qwen3Attention.q_norm / k_norm, a Qwen3RMSNorm over each 128-wide
// head) between the q|k|v projection and the rotary embedding -- the step none of the fused q|k|v + RoPE GEMM epilogues can take.
//
//   tasu_qk_norm_rope_fwd      out = bf16(rope(w * bf16(pre * r))),  r = rsqrt(mean_128(pre^2) + eps), per row and q / k head;
//                              v heads copied bit for bit; r kept for the backward
//   tasu_qk_norm_bwd           dpre = r (w g - xn mean_128(w g xn)),  xn = pre r, in place on dqkv (g: what the attention backward
//                              leaves there behind its own RoPE backward); v block untouched
//   tasu_qk_norm_rope_append   the forward in place on the decode step's [M, (H+2G)*128], then k and v -> cache[row, pos[row]]
//
// bf16-autocast arithmetic of HF's Qwen3RMSNorm: the statistic and pre * r in fp32, ONE rounding to bf16 (the cast back to the
// input dtype), the product with the fp32 weight and the rotation in fp32, ONE rounding at the store.
//
// Thread map: 16 lanes per (row, head), 8 contiguous elements (one 16-byte vector) per lane; lanes 0-7 hold dims 0..63, lanes 8-15
// dims 64..127, so the rotate-half partner of a lane's vector is lane ^ 8's and the mean is four xor-shuffles inside the 16-lane
// group.  A wave serves 4 heads, a 256-thread block 16; nothing goes through LDS, no atomics.  The forward and the append kernel
// share qk_head_fwd: a key appended at decode time has the bits of the same key out of a prefill.
//
// Cost, DERIVED (not measured here): one read and one write of [M, (H+2G)*128] bf16 per launch (the v block only when out != pre).
//
// The fp32 family (train_config.use_fp16 = false: HF's Qwen3RMSNorm on fp32 tensors with no autocast, nothing rounded to bf16):
//   tasu_f32_qk_norm_rope      out = rope(w * (pre * r)), v heads copied bit for bit, r kept on request; with a cache the rotated
//                              k and the v of row m also go to cache[m, slot[m]] (tasu_f32_rope's layout) -- forward and append
//   tasu_f32_qk_norm_bwd       dpre = r (w g - xn mean_128(w g xn)),  xn = pre r, in place on dqkv behind tasu_f32_rope(inverse = 1)
// Thread map and device function: f32_qk_head.h (32 lanes per (row, head), one 16-byte vector per lane), shared with
// f32_sum_slabs_qk_norm_rope_kernel of csrc/fp32.hip.  Cost, DERIVED: one read and one write of [M, (H+2G)*128] fp32.
//
// The norm weights' gradients (full fine-tuning, both families; called BEFORE the backward kernel overwrites dqkv):
//   tasu_qk_norm_wgrad         dwq[d] = or += sum_{m, q heads} g xn,  dwk: over the k heads;  xn = bf16(pre r): exact products, fp32 sums
//   tasu_f32_qk_norm_wgrad     the same with xn = pre r in fp32
// Two launches, TASU_QK_WGRAD_SPLIT workgroups and one, fixed orders, no atomics (see the kernels).  Cost, DERIVED: one read of the
// q and k blocks of dqkv and pre -- 50 MB in bf16, 101 MB in fp32 at Qwen3-1.7B, M = 4096 -- and 0.5 MB of slabs written and read.
#include "common.h"
#include "f32_qk_head.h"
#include "../../include/tasu_hip.h"

namespace {

constexpr int HD = 128;

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One lane's share of one q / k head: x = its 8 elements of pre, w = the head's norm weight at those dims, (cs, sn) = the row's
// table at the lane's 8 pair indices; sub = lane & 15.  Returns the rotated, rounded vector; r = the head's rstd (all 16 lanes).
__device__ __forceinline__ bf16x8 qk_head_fwd(const bf16x8 x, const float* __restrict__ w, const float* __restrict__ cs,
                                              const float* __restrict__ sn, float eps, int sub, float& r) {
  float xf[8], ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    xf[j] = (float)x[j];
    ss = __builtin_fmaf(xf[j], xf[j], ss);
  }
  ss = group16_sum(ss);
  r = rsqrtf(ss * (1.0f / HD) + eps);
  const f32x4 w0 = *(const f32x4*)w, w1 = *(const f32x4*)(w + 4);
  const f32x4 c0 = *(const f32x4*)cs, c1 = *(const f32x4*)(cs + 4);
  const f32x4 s0 = *(const f32x4*)sn, s1 = *(const f32x4*)(sn + 4);
  const bool hi = sub >= 8;
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float wj = j < 4 ? w0[j & 3] : w1[j & 3];
    const float c = j < 4 ? c0[j & 3] : c1[j & 3], s = j < 4 ? s0[j & 3] : s1[j & 3];
    const float y = wj * bf16_round(xf[j] * r);            // w * x.to(bf16): fp32 product of the fp32 weight
    const float other = __shfl_xor(y, 8, 64);              // the rotate-half partner (dim ^ 64)
    float y1, y2;
    rope_pair_f(hi ? other : y, hi ? y : other, c, s, y1, y2);
    out[j] = (bf16)(hi ? y2 : y1);
  }
  return out;
}

__global__ __launch_bounds__(256) void qk_norm_rope_fwd_kernel(const bf16* __restrict__ pre, const float* __restrict__ wq,
                                                               const float* __restrict__ wk, const float* __restrict__ ct,
                                                               const float* __restrict__ st, bf16* __restrict__ out,
                                                               float* __restrict__ rstd, int M, int H, int G, float eps) {
  const int NH = H + 2 * G, sub = threadIdx.x & 15;
  const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = unit < (long long)M * NH;
  const int row = live ? (int)(unit / NH) : 0, hh = live ? (int)(unit % NH) : 0;
  const size_t off = ((size_t)row * NH + hh) * HD + sub * 8;
  if (hh >= H + G) {                                       // a v head: the projection's bits
    if (live && out != pre) *(bf16x8*)(out + off) = *(const bf16x8*)(pre + off);
    return;                                                // (whole 16-lane groups leave: the shuffles below stay inside a group)
  }
  const bf16x8 x = *(const bf16x8*)(pre + off);
  const float* w = (hh < H ? wq : wk) + sub * 8;
  const int p = (sub & 7) * 8;
  float r;
  const bf16x8 y = qk_head_fwd(x, w, ct + (size_t)row * 64 + p, st + (size_t)row * 64 + p, eps, sub, r);
  if (!live) return;
  *(bf16x8*)(out + off) = y;
  if (rstd && sub == 0) rstd[(size_t)row * (H + G) + hh] = r;
}

__global__ __launch_bounds__(256) void qk_norm_bwd_kernel(bf16* __restrict__ dqkv, const bf16* __restrict__ pre,
                                                          const float* __restrict__ wq, const float* __restrict__ wk,
                                                          const float* __restrict__ rstd, int M, int H, int G) {
  const int NH = H + 2 * G, NQK = H + G, sub = threadIdx.x & 15;
  const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);      // over the q and k heads only
  const bool live = unit < (long long)M * NQK;
  const int row = live ? (int)(unit / NQK) : 0, hh = live ? (int)(unit % NQK) : 0;
  const size_t off = ((size_t)row * NH + hh) * HD + sub * 8;
  const bf16x8 x = *(const bf16x8*)(pre + off), g = *(const bf16x8*)(dqkv + off);
  const float* w = (hh < H ? wq : wk) + sub * 8;
  const f32x4 w0 = *(const f32x4*)w, w1 = *(const f32x4*)(w + 4);
  const float r = rstd[(size_t)row * NQK + hh];
  float wg[8], xn[8], dot = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    wg[j] = (j < 4 ? w0[j & 3] : w1[j & 3]) * (float)g[j];
    xn[j] = (float)x[j] * r;
    dot = __builtin_fmaf(wg[j], xn[j], dot);
  }
  const float mean = group16_sum(dot) * (1.0f / HD);
  bf16x8 d;
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = (bf16)(r * (wg[j] - xn[j] * mean));
  if (live) *(bf16x8*)(dqkv + off) = d;
}

__global__ __launch_bounds__(256) void qk_norm_rope_append_kernel(bf16* __restrict__ qkv, const float* __restrict__ wq,
                                                                  const float* __restrict__ wk, const float* __restrict__ ct,
                                                                  const float* __restrict__ st, bf16* __restrict__ kc,
                                                                  bf16* __restrict__ vc, const int32_t* __restrict__ pos, int M,
                                                                  int H, int G, int ctx, float eps) {
  const int NH = H + 2 * G, sub = threadIdx.x & 15;
  const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = unit < (long long)M * NH;
  const int row = live ? (int)(unit / NH) : 0, hh = live ? (int)(unit % NH) : 0;
  const size_t off = ((size_t)row * NH + hh) * HD + sub * 8;
  const int at = pos[row];
  const bool slot_ok = live && at >= 0 && at < ctx;        // a position outside the cache writes nothing there
  const size_t slot = ((size_t)row * ctx + (slot_ok ? at : 0)) * ((size_t)G * HD);
  if (hh >= H + G) {
    if (slot_ok) *(bf16x8*)(vc + slot + (size_t)(hh - H - G) * HD + sub * 8) = *(const bf16x8*)(qkv + off);
    return;
  }
  const bf16x8 x = *(const bf16x8*)(qkv + off);
  const float* w = (hh < H ? wq : wk) + sub * 8;
  const int p = (sub & 7) * 8;
  float r;
  const bf16x8 y = qk_head_fwd(x, w, ct + (size_t)row * 64 + p, st + (size_t)row * 64 + p, eps, sub, r);
  if (!live) return;
  *(bf16x8*)(qkv + off) = y;
  if (hh >= H && slot_ok) *(bf16x8*)(kc + slot + (size_t)(hh - H) * HD + sub * 8) = y;
}

// ---------------------------------------------------------------------------------------------------------------- fp32 family
using tasu_f32::QK_HEADS_PER_BLOCK;
using tasu_f32::QK_LANES;

__global__ __launch_bounds__(256) void f32_qk_norm_rope_kernel(const float* pre, const float* __restrict__ wq, const float* __restrict__ wk,
                                                               const float* __restrict__ ct, const float* __restrict__ st, float* out,
                                                               float* __restrict__ rstd, int M, int H, int G, float eps,
                                                               float* __restrict__ kc, float* __restrict__ vc,
                                                               const int32_t* __restrict__ slot, int ctx) {
  // (pre / out carry no __restrict__: out == pre is allowed; a lane reads its vector before it stores to the same address)
  const int NH = H + 2 * G, sub = threadIdx.x & (QK_LANES - 1);
  const long long unit = (long long)blockIdx.x * QK_HEADS_PER_BLOCK + threadIdx.x / QK_LANES;
  const bool live = unit < (long long)M * NH;
  const int row = live ? (int)(unit / NH) : 0, hh = live ? (int)(unit % NH) : 0;      // (a spare group computes row 0, head 0 and stores nothing)
  const size_t off = ((size_t)row * NH + hh) * HD + sub * 4;
  const f32x4 x = *(const f32x4*)(pre + off);
  const int at = kc ? slot[row] : -1;
  const bool slot_ok = live && at >= 0 && at < ctx;        // a slot outside the cache writes nothing there
  const size_t cell = ((size_t)row * ctx + (slot_ok ? at : 0)) * ((size_t)G * HD) + sub * 4;
  if (hh >= H + G) {                                       // a v head: the projection's bits (whole 32-lane groups leave)
    if (live && out != pre) *(f32x4*)(out + off) = x;
    if (slot_ok) *(f32x4*)(vc + cell + (size_t)(hh - H - G) * HD) = x;
    return;
  }
  const int p = (sub & 15) * 4;
  float r;
  const f32x4 y = tasu_f32::f32_qk_head_fwd(x, (hh < H ? wq : wk) + sub * 4, ct + (size_t)row * 64 + p, st + (size_t)row * 64 + p, eps, sub, r);
  if (!live) return;
  *(f32x4*)(out + off) = y;
  if (rstd && sub == 0) rstd[(size_t)row * (H + G) + hh] = r;
  if (hh >= H && slot_ok) *(f32x4*)(kc + cell + (size_t)(hh - H) * HD) = y;
}

__global__ __launch_bounds__(256) void f32_qk_norm_bwd_kernel(float* __restrict__ dqkv, const float* __restrict__ pre,
                                                              const float* __restrict__ wq, const float* __restrict__ wk,
                                                              const float* __restrict__ rstd, int M, int H, int G) {
  const int NH = H + 2 * G, NQK = H + G, sub = threadIdx.x & (QK_LANES - 1);
  const long long unit = (long long)blockIdx.x * QK_HEADS_PER_BLOCK + threadIdx.x / QK_LANES;      // over the q and k heads only
  const bool live = unit < (long long)M * NQK;
  const int row = live ? (int)(unit / NQK) : 0, hh = live ? (int)(unit % NQK) : 0;
  const size_t off = ((size_t)row * NH + hh) * HD + sub * 4;
  const f32x4 x = *(const f32x4*)(pre + off), g = *(const f32x4*)(dqkv + off);
  const f32x4 w = *(const f32x4*)((hh < H ? wq : wk) + sub * 4);
  const float r = rstd[(size_t)row * NQK + hh];
  float wg[4], xn[4], dot = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wg[j] = w[j] * g[j];
    xn[j] = x[j] * r;
    dot = __builtin_fmaf(wg[j], xn[j], dot);
  }
  const float mean = tasu_f32::group32_sum(dot) * (1.0f / HD);
  f32x4 d;
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = r * (wg[j] - xn[j] * mean);
  if (live) *(f32x4*)(dqkv + off) = d;
}

// ------------------------------------------------------------------------------------------- q_norm / k_norm weight gradients
// Stage 1: TASU_QK_WGRAD_SPLIT workgroups, whatever the shape.  Workgroup b's group i (16 lanes, or 32 in the fp32 family) walks
// the (row, head) units b * GROUPS + i, + SPLIT * GROUPS, ... over the q and k heads; a lane keeps the sums of its own dims, q and k
// apart (a unit adds to one and +0 to the other: no branch inside a wave).  The groups meet in LDS and are summed in group order
// into the workgroup's slab [2, 128] of ws -- idle workgroups write zeros.  Stage 2: one workgroup sums the slabs in ascending order.
template <int GROUPS>
__device__ __forceinline__ void qk_wgrad_meet(float (*part)[2][HD], float* __restrict__ ws) {
  __syncthreads();
  const int which = threadIdx.x >> 7, d = threadIdx.x & (HD - 1);
  float s = part[0][which][d];
#pragma unroll
  for (int i = 1; i < GROUPS; ++i) s += part[i][which][d];
  ws[(size_t)blockIdx.x * (2 * HD) + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void qk_norm_wgrad_part_kernel(const bf16* __restrict__ dqkv, const bf16* __restrict__ pre,
                                                                 const float* __restrict__ rstd, float* __restrict__ ws, int M,
                                                                 int H, int G) {
  __shared__ float part[16][2][HD];
  const int NH = H + 2 * G, NQK = H + G, sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const long long units = (long long)M * NQK;
  float sq[8], sk[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) sq[j] = sk[j] = 0.f;
  for (long long unit = (long long)blockIdx.x * 16 + grp; unit < units; unit += (long long)TASU_QK_WGRAD_SPLIT * 16) {
    const int row = (int)(unit / NQK), hh = (int)(unit % NQK);
    const size_t off = ((size_t)row * NH + hh) * HD + sub * 8;
    const bf16x8 x = *(const bf16x8*)(pre + off), g = *(const bf16x8*)(dqkv + off);
    const float r = rstd[unit];                            // [M, H+G]: row * NQK + hh
    const bool isq = hh < H;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = (float)g[j] * bf16_round((float)x[j] * r);      // two bf16 values: exact in fp32
      sq[j] += isq ? p : 0.f;
      sk[j] += isq ? 0.f : p;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[grp][0][sub * 8 + j] = sq[j], part[grp][1][sub * 8 + j] = sk[j];
  qk_wgrad_meet<16>(part, ws);
}

__global__ __launch_bounds__(256) void f32_qk_norm_wgrad_part_kernel(const float* __restrict__ dqkv, const float* __restrict__ pre,
                                                                     const float* __restrict__ rstd, float* __restrict__ ws, int M,
                                                                     int H, int G) {
  __shared__ float part[QK_HEADS_PER_BLOCK][2][HD];
  const int NH = H + 2 * G, NQK = H + G, sub = threadIdx.x & (QK_LANES - 1), grp = threadIdx.x / QK_LANES;
  const long long units = (long long)M * NQK;
  f32x4 sq = f32x4{0.f, 0.f, 0.f, 0.f}, sk = sq;
  for (long long unit = (long long)blockIdx.x * QK_HEADS_PER_BLOCK + grp; unit < units;
       unit += (long long)TASU_QK_WGRAD_SPLIT * QK_HEADS_PER_BLOCK) {
    const int row = (int)(unit / NQK), hh = (int)(unit % NQK);
    const size_t off = ((size_t)row * NH + hh) * HD + sub * 4;
    const f32x4 x = *(const f32x4*)(pre + off), g = *(const f32x4*)(dqkv + off);
    const float r = rstd[unit];
    const bool isq = hh < H;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = g[j] * (x[j] * r);
      sq[j] += isq ? p : 0.f;
      sk[j] += isq ? 0.f : p;
    }
  }
  *(f32x4*)&part[grp][0][sub * 4] = sq;
  *(f32x4*)&part[grp][1][sub * 4] = sk;
  qk_wgrad_meet<QK_HEADS_PER_BLOCK>(part, ws);
}

__global__ __launch_bounds__(256) void qk_norm_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dwq,
                                                                float* __restrict__ dwk, int accumulate) {
  const int t = threadIdx.x;
  float s = ws[t];
#pragma unroll 16
  for (int i = 1; i < TASU_QK_WGRAD_SPLIT; ++i) s += ws[(size_t)i * (2 * HD) + t];
  float* dst = t < HD ? dwq + t : dwk + (t - HD);
  *dst = accumulate ? *dst + s : s;
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
inline bool shape_ok(int M, int H, int G) {
  return M > 0 && H > 0 && G > 0 && H % G == 0 && (long long)M * (H + 2 * G) <= 0x7fffffffLL / 16;
}
inline unsigned blocks_for(long long units) { return (unsigned)((units + 15) / 16); }
inline bool f32_shape_ok(int M, int H, int G) {
  return M > 0 && H > 0 && G > 0 && H % G == 0 && (long long)M * (H + 2 * G) <= 0x7fffffffLL / QK_LANES;
}
inline unsigned f32_blocks_for(long long units) { return (unsigned)((units + QK_HEADS_PER_BLOCK - 1) / QK_HEADS_PER_BLOCK); }

}  // namespace

extern "C" int tasu_qk_norm_rope_fwd(const void* pre, const float* wq, const float* wk, const float* cos_tab, const float* sin_tab,
                                     void* out, float* rstd, int M, int H, int G, float eps, void* stream) {
  if (!pre || !wq || !wk || !cos_tab || !sin_tab || !out || !shape_ok(M, H, G) || !(eps >= 0.f)) return TASU_ERR_ARG;
  if (misaligned(pre) || misaligned(wq) || misaligned(wk) || misaligned(cos_tab) || misaligned(sin_tab) || misaligned(out))
    return TASU_ERR_ARG;
  if (out != pre) {                                        // the same buffer, or two that do not overlap
    const size_t bytes = (size_t)M * (H + 2 * G) * HD * sizeof(bf16);
    const uintptr_t a = (uintptr_t)pre, b = (uintptr_t)out;
    if (a < b + bytes && b < a + bytes) return TASU_ERR_ARG;
  }
  TASU_LAUNCH(qk_norm_rope_fwd_kernel, dim3(blocks_for((long long)M * (H + 2 * G))), dim3(256), 0, (hipStream_t)stream,
              (const bf16*)pre, wq, wk, cos_tab, sin_tab, (bf16*)out, rstd, M, H, G, eps);
  return TASU_OK;
}

extern "C" int tasu_qk_norm_bwd(void* dqkv, const void* pre, const float* wq, const float* wk, const float* rstd, int M, int H,
                                int G, void* stream) {
  if (!dqkv || !pre || !wq || !wk || !rstd || dqkv == pre || !shape_ok(M, H, G)) return TASU_ERR_ARG;
  if (misaligned(dqkv) || misaligned(pre) || misaligned(wq) || misaligned(wk)) return TASU_ERR_ARG;
  TASU_LAUNCH(qk_norm_bwd_kernel, dim3(blocks_for((long long)M * (H + G))), dim3(256), 0, (hipStream_t)stream, (bf16*)dqkv,
              (const bf16*)pre, wq, wk, rstd, M, H, G);
  return TASU_OK;
}

extern "C" int tasu_qk_norm_rope_append(void* qkv, const float* wq, const float* wk, const float* cos_tab, const float* sin_tab,
                                        void* kcache, void* vcache, const int32_t* pos, int M, int H, int G, int ctx, float eps,
                                        void* stream) {
  if (!qkv || !wq || !wk || !cos_tab || !sin_tab || !kcache || !vcache || !pos || !shape_ok(M, H, G) || ctx <= 0 || !(eps >= 0.f))
    return TASU_ERR_ARG;
  if (misaligned(qkv) || misaligned(wq) || misaligned(wk) || misaligned(cos_tab) || misaligned(sin_tab) || misaligned(kcache) ||
      misaligned(vcache))
    return TASU_ERR_ARG;
  TASU_LAUNCH(qk_norm_rope_append_kernel, dim3(blocks_for((long long)M * (H + 2 * G))), dim3(256), 0, (hipStream_t)stream,
              (bf16*)qkv, wq, wk, cos_tab, sin_tab, (bf16*)kcache, (bf16*)vcache, pos, M, H, G, ctx, eps);
  return TASU_OK;
}

extern "C" int tasu_f32_qk_norm_rope(const float* pre, const float* wq, const float* wk, const float* cos_tab, const float* sin_tab,
                                     float* out, float* rstd, int M, int H, int G, float eps, float* kcache, float* vcache,
                                     const int32_t* slot, int ctx, void* stream) {
  if (!pre || !wq || !wk || !cos_tab || !sin_tab || !out || !f32_shape_ok(M, H, G) || !(eps >= 0.f)) return TASU_ERR_ARG;
  if (misaligned(pre) || misaligned(wq) || misaligned(wk) || misaligned(cos_tab) || misaligned(sin_tab) || misaligned(out))
    return TASU_ERR_ARG;
  if (kcache && (!vcache || !slot || ctx <= 0 || misaligned(kcache) || misaligned(vcache))) return TASU_ERR_ARG;
  if (out != pre) {                                        // the same buffer, or two that do not overlap
    const size_t bytes = (size_t)M * (H + 2 * G) * HD * sizeof(float);
    const uintptr_t a = (uintptr_t)pre, b = (uintptr_t)out;
    if (a < b + bytes && b < a + bytes) return TASU_ERR_ARG;
  }
  TASU_LAUNCH(f32_qk_norm_rope_kernel, dim3(f32_blocks_for((long long)M * (H + 2 * G))), dim3(256), 0, (hipStream_t)stream, pre, wq, wk,
              cos_tab, sin_tab, out, rstd, M, H, G, eps, kcache, vcache, slot, ctx);
  return TASU_OK;
}

extern "C" int tasu_f32_qk_norm_bwd(float* dqkv, const float* pre, const float* wq, const float* wk, const float* rstd, int M, int H,
                                    int G, void* stream) {
  if (!dqkv || !pre || !wq || !wk || !rstd || dqkv == pre || !f32_shape_ok(M, H, G)) return TASU_ERR_ARG;
  if (misaligned(dqkv) || misaligned(pre) || misaligned(wq) || misaligned(wk)) return TASU_ERR_ARG;
  TASU_LAUNCH(f32_qk_norm_bwd_kernel, dim3(f32_blocks_for((long long)M * (H + G))), dim3(256), 0, (hipStream_t)stream, dqkv, pre, wq, wk,
              rstd, M, H, G);
  return TASU_OK;
}

namespace {
inline bool wgrad_args_ok(const void* dqkv, const void* pre, const float* rstd, const float* dwq, const float* dwk, const float* ws,
                          int64_t ws_floats) {
  if (!dqkv || !pre || !rstd || !dwq || !dwk || !ws || dqkv == pre) return false;
  if (misaligned(dqkv) || misaligned(pre) || misaligned(ws) || ((uintptr_t)rstd & 3) || ((uintptr_t)dwq & 3) || ((uintptr_t)dwk & 3)) return false;
  return ws_floats >= (int64_t)TASU_QK_WGRAD_SPLIT * 2 * HD;
}
}  // namespace

extern "C" int tasu_qk_norm_wgrad(const void* dqkv_bf16, const void* pre_bf16, const float* rstd, float* dwq, float* dwk, float* ws,
                                  int64_t ws_floats, int M, int H, int G, int accumulate, void* stream) {
  if (!wgrad_args_ok(dqkv_bf16, pre_bf16, rstd, dwq, dwk, ws, ws_floats) || !shape_ok(M, H, G)) return TASU_ERR_ARG;
  TASU_LAUNCH(qk_norm_wgrad_part_kernel, dim3(TASU_QK_WGRAD_SPLIT), dim3(256), 0, (hipStream_t)stream, (const bf16*)dqkv_bf16,
              (const bf16*)pre_bf16, rstd, ws, M, H, G);
  TASU_LAUNCH(qk_norm_wgrad_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dwq, dwk, accumulate ? 1 : 0);
  return TASU_OK;
}

extern "C" int tasu_f32_qk_norm_wgrad(const float* dqkv, const float* pre, const float* rstd, float* dwq, float* dwk, float* ws,
                                      int64_t ws_floats, int M, int H, int G, int accumulate, void* stream) {
  if (!wgrad_args_ok(dqkv, pre, rstd, dwq, dwk, ws, ws_floats) || !f32_shape_ok(M, H, G)) return TASU_ERR_ARG;
  TASU_LAUNCH(f32_qk_norm_wgrad_part_kernel, dim3(TASU_QK_WGRAD_SPLIT), dim3(256), 0, (hipStream_t)stream, dqkv, pre, rstd, ws, M, H, G);
  TASU_LAUNCH(qk_norm_wgrad_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dwq, dwk, accumulate ? 1 : 0);
  return TASU_OK;
}
