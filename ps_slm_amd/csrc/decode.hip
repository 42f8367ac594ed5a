// Decode-loop kernels (Multitask/model/ps-slm.py:660-675 -> HF GenerationMixin beam search, 4 beams): KV cache
// fill / append / beam reorder, single-token GQA attention over the cache, and the per-position prologue (embedding row, norm,
// RoPE factors, reorder of the cache row index).  All HBM-bound (weights and KV are read once per step).  The per-row
// log-softmax + top-k lives in topk.hip, the beam bookkeeping in beam.hip.
#include "common.h"
#include "attn_decode_body.h"
#include "../../include/tasu_hip.h"

namespace {
constexpr int HD = 128;

// cache[b*nb, s, :] = k|v block of qkv[(b*S + s), :]: the prompt is stored ONCE per utterance, in the cache row of its
// first beam; the other beams reach it through the row index (kv_index_*).   grid (S, B), block 256
__global__ __launch_bounds__(256) void kv_fill_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ kc, bf16* __restrict__ vc,
                                                      int S, int H, int G, int nb, int ctx) {
  const int s = blockIdx.x, b = blockIdx.y;
  const int LD = (H + 2 * G) * HD, W = G * HD;
  const bf16* src = qkv + ((size_t)b * S + s) * LD + H * HD;
  for (int c = threadIdx.x * 8; c < 2 * W; c += 256 * 8) {
    const bf16x8 v = *(const bf16x8*)(src + c);
    bf16* base = c < W ? kc : vc;
    const int cc = c < W ? c : c - W;
    *(bf16x8*)(base + (((size_t)b * nb) * ctx + s) * W + cc) = v;
  }
}

// Decode-step RoPE + cache append: one block per row; thread t rotates 8-element chunk pairs (x[d], x[d+64]) of the H query
// and G key heads in place and copies the rotated keys and the values into cache[row, pos[row]].
__global__ __launch_bounds__(256) void rope_append_kernel(bf16* __restrict__ qkv, const float* __restrict__ ct,
                                                          const float* __restrict__ st, bf16* __restrict__ kc,
                                                          bf16* __restrict__ vc, const int32_t* __restrict__ pos, int H, int G,
                                                          int ctx) {
  const int row = blockIdx.x;
  const int LD = (H + 2 * G) * HD, W = G * HD;
  bf16* x = qkv + (size_t)row * LD;
  const size_t slot = ((size_t)row * ctx + pos[row]) * W;
  const float* cr = ct + (size_t)row * 64;
  const float* sr = st + (size_t)row * 64;
  for (int u = threadIdx.x; u < (H + G) * 8; u += 256) {       // unit = (head, 8-wide chunk of the low half)
    const int hh = u >> 3, c = (u & 7) * 8;
    bf16* hp = x + hh * HD;
    bf16x8 lo = *(const bf16x8*)(hp + c), hi = *(const bf16x8*)(hp + 64 + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float cs = cr[c + j], sn = sr[c + j];
      const float x1 = (float)lo[j], x2 = (float)hi[j];
      lo[j] = (bf16)(x1 * cs - x2 * sn);
      hi[j] = (bf16)(x2 * cs + x1 * sn);
    }
    *(bf16x8*)(hp + c) = lo;
    *(bf16x8*)(hp + 64 + c) = hi;
    if (hh >= H) {
      bf16* kd = kc + slot + (hh - H) * HD;
      *(bf16x8*)(kd + c) = lo;
      *(bf16x8*)(kd + 64 + c) = hi;
    }
  }
  for (int c = threadIdx.x * 8; c < W; c += 256 * 8) *(bf16x8*)(vc + slot + c) = *(const bf16x8*)(x + (H + G) * HD + c);
}

// Row index of the beam-shared cache: index[m, i] = physical cache row that holds position i of logical row (beam) m.
// init: prompt positions point at the utterance's first beam, generated positions at the row itself.
__global__ __launch_bounds__(256) void kv_index_init_kernel(int32_t* __restrict__ index, int nb, int S, int ctx, int total) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int m = e / ctx, i = e - m * ctx;
  index[e] = i < S ? (m / nb) * nb : m;
}
// beam reorder (HF Cache.reorder_cache) on the index instead of on the cache: dst[m, :lens[m]] = src[src_row[m], :lens[m]];
// positions >= lens[m] keep their value (the identity written by init: a row always appends into itself).  grid (M)
__global__ __launch_bounds__(256) void kv_index_reorder_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                               const int32_t* __restrict__ src_row,
                                                               const int32_t* __restrict__ lens, int ctx) {
  const int m = blockIdx.x;
  const int n = lens[m];
  const int32_t* s = src + (size_t)(src_row ? src_row[m] : m) * ctx;
  for (int i = threadIdx.x; i < n; i += 256) dst[(size_t)m * ctx + i] = s[i];
}

// cache[row, pos[row], :] = k|v block of qkv[row, :]     grid (M), block 128
__global__ __launch_bounds__(128) void kv_append_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ kc, bf16* __restrict__ vc,
                                                        const int32_t* __restrict__ pos, int H, int G, int ctx) {
  const int row = blockIdx.x;
  const int LD = (H + 2 * G) * HD, W = G * HD;
  const bf16* src = qkv + (size_t)row * LD + H * HD;
  const int p = pos[row];
  for (int c = threadIdx.x * 8; c < 2 * W; c += 128 * 8) {
    const bf16x8 v = *(const bf16x8*)(src + c);
    if (c < W)
      *(bf16x8*)(kc + ((size_t)row * ctx + p) * W + c) = v;
    else
      *(bf16x8*)(vc + ((size_t)row * ctx + p) * W + (c - W)) = v;
  }
}

using tasu_attn_dec::DEC_NW;
using tasu_attn_dec::MAX_CTX;
// Single-token GQA attention over the cache: one 8-wave block per (row, kv group); body and design notes: attn_decode_body.h
template <int REP>
__global__ __launch_bounds__(64 * DEC_NW) void attn_decode_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ kc,
                                                                  const bf16* __restrict__ vc,
                                                                  const int32_t* __restrict__ row_index,
                                                                  const int32_t* __restrict__ kstart,
                                                                  const int32_t* __restrict__ lens, bf16* __restrict__ out,
                                                                  int H, int G, int ctx, float scale, int out_frag) {
  extern __shared__ float sp[];
  tasu_attn_dec::attn_decode_body<REP, false>(sp, blockIdx.x, blockIdx.y, qkv, kc, vc, row_index, kstart, lens, out, H, G, ctx, scale,
                                              out_frag);
}

// x[m,:] = table[ids[m], :]  (fp32 embedding rows for the decode step)
__global__ __launch_bounds__(256) void embed_rows_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                                         float* __restrict__ x, int M, int D) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const float* src = table + (size_t)ids[m] * D;
  for (int c = lane * 4; c < D; c += 256) *(f32x4*)(x + (size_t)m * D + c) = *(const f32x4*)(src + c);
}

// Everything a generated position needs before its first layer, in ONE launch (block = beam row m; each piece used to be a
// launch of ~5 us that does microseconds of work):
//   wave 0  x[m, :] = table[ids[m], :] (fp32 embedding row) and xn = RMSNorm(x[m], norm_w) in fragment order (stream_body.h's
//           norm_row_frag: the arithmetic of tasu_rmsnorm_fwd_frag), 64-row chunks;
//   wave 1  RoPE factors cos / sin [m, 64] of position pos[m] (rope.hip's rope_table_kernel arithmetic);
//   all     if m is the first row of its utterance (m % nb == 0): the beam reorder of the utterance's nb rows of the cache row
//           index, IN PLACE -- dst[r, :lens[r]] = src[src_row[r], :lens[r]] -- staged through LDS; a beam's parent is always a
//           row of the same utterance (HF beam search reorders within a batch item), which is what makes one workgroup enough.
constexpr int PROLOGUE_MAX_NB = 5;      // n_beams * ctx ints of LDS: wider searches take the separate set-up launches
template <int NG>
__global__ __launch_bounds__(256) void decode_step_prologue_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                                                   float* __restrict__ x, const float* __restrict__ norm_w,
                                                                   bf16* __restrict__ xn, float eps, const int32_t* __restrict__ pos,
                                                                   float* __restrict__ ct, float* __restrict__ st, float theta,
                                                                   int32_t* __restrict__ index, const int32_t* __restrict__ src_row,
                                                                   const int32_t* __restrict__ lens, int nb, int M, int ctx) {
  extern __shared__ int stage[];                          // [nb][ctx]
  constexpr int D = NG * 256;
  const int m = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave == 0) {
    const float* src = table + (size_t)ids[m] * D;
    for (int c = lane * 4; c < D; c += 256) *(f32x4*)(x + (size_t)m * D + c) = *(const f32x4*)(src + c);
    tasu_stream::norm_row_frag_ptr<NG, false>(src, norm_w, xn + (size_t)(m >> 6) * 64 * D, m & 63, eps);
  } else if (wave == 1) {
    const int half = HD / 2, i = lane;
    const float inv = 1.0f / powf(theta, (float)(2 * i) / (float)(2 * half));
    const float ang = (float)pos[m] * inv;
    float sn, cs;
    sincosf(ang, &sn, &cs);
    ct[m * half + i] = cs;
    st[m * half + i] = sn;
  }
  if (m % nb) return;
  const int rows = min(nb, M - m);
  for (int r = 0; r < rows; ++r) {
    const int n = lens[m + r];
    const int32_t* s = index + (size_t)src_row[m + r] * ctx;
    for (int i = threadIdx.x; i < n; i += 256) stage[r * ctx + i] = s[i];
  }
  __syncthreads();
  for (int r = 0; r < rows; ++r) {
    const int n = lens[m + r];
    for (int i = threadIdx.x; i < n; i += 256) index[(size_t)(m + r) * ctx + i] = stage[r * ctx + i];
  }
}

}  // namespace

extern "C" int tasu_decode_step_prologue(const float* table, const int32_t* ids, float* x, const float* norm_w, void* xn_frag,
                                         float eps, const int32_t* pos, float* cos_tab, float* sin_tab, float theta, int32_t* index,
                                         const int32_t* src_row, const int32_t* lens, int n_beams, int M, int D, int ctx,
                                         void* stream) {
  if (!table || !ids || !x || !norm_w || !xn_frag || !pos || !cos_tab || !sin_tab || !index || !src_row || !lens) return TASU_ERR_ARG;
  if (M <= 0 || n_beams <= 0 || n_beams > PROLOGUE_MAX_NB || ctx <= 0 || ctx > MAX_CTX || D % 256) return TASU_ERR_ARG;
  const size_t lds = (size_t)n_beams * ctx * sizeof(int);
#define TASU_PRO(NG)                                                                                                              \
  case NG:                                                                                                                        \
    TASU_LAUNCH(decode_step_prologue_kernel<NG>, dim3(M), dim3(256), lds, (hipStream_t)stream, table, ids, x, norm_w, (bf16*)xn_frag, \
                eps, pos, cos_tab, sin_tab, theta, index, src_row, lens, n_beams, M, ctx);                                       \
    return TASU_OK;
  switch (D / 256) {
    TASU_PRO(1) TASU_PRO(2) TASU_PRO(6) TASU_PRO(7) TASU_PRO(14)
    default: return TASU_ERR_ARG;
  }
#undef TASU_PRO
}

extern "C" int tasu_kv_fill(const void* qkv, void* kcache, void* vcache, int B, int S, int H, int G, int n_beams, int ctx,
                            void* stream) {
  if (!qkv || !kcache || !vcache || B <= 0 || S <= 0 || S > ctx || H <= 0 || G <= 0 || n_beams <= 0) return TASU_ERR_ARG;
  TASU_LAUNCH(kv_fill_kernel, dim3(S, B), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, (bf16*)kcache, (bf16*)vcache, S,
              H, G, n_beams, ctx);
  return TASU_OK;
}
extern "C" int tasu_kv_append(const void* qkv, void* kcache, void* vcache, const int32_t* pos, int M, int H, int G, int ctx,
                              void* stream) {
  if (!qkv || !kcache || !vcache || !pos || M <= 0 || H <= 0 || G <= 0) return TASU_ERR_ARG;
  TASU_LAUNCH(kv_append_kernel, dim3(M), dim3(128), 0, (hipStream_t)stream, (const bf16*)qkv, (bf16*)kcache, (bf16*)vcache, pos,
              H, G, ctx);
  return TASU_OK;
}
extern "C" int tasu_rope_append(void* qkv, const float* cos_tab, const float* sin_tab, void* kcache, void* vcache,
                                const int32_t* pos, int M, int H, int G, int ctx, void* stream) {
  if (!qkv || !cos_tab || !sin_tab || !kcache || !vcache || !pos || M <= 0 || H <= 0 || G <= 0 || ctx <= 0) return TASU_ERR_ARG;
  TASU_LAUNCH(rope_append_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (bf16*)qkv, cos_tab, sin_tab, (bf16*)kcache,
              (bf16*)vcache, pos, H, G, ctx);
  return TASU_OK;
}
extern "C" int tasu_kv_index_init(int32_t* index, int B, int n_beams, int S, int ctx, void* stream) {
  if (!index || B <= 0 || n_beams <= 0 || S <= 0 || ctx < S) return TASU_ERR_ARG;
  const int total = B * n_beams * ctx;
  TASU_LAUNCH(kv_index_init_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, index, n_beams, S, ctx, total);
  return TASU_OK;
}
extern "C" int tasu_kv_index_reorder(const int32_t* src_index, int32_t* dst_index, const int32_t* src_row, const int32_t* lens,
                                     int M, int ctx, void* stream) {
  if (!src_index || !dst_index || src_index == dst_index || !lens || M <= 0 || ctx <= 0) return TASU_ERR_ARG;
  TASU_LAUNCH(kv_index_reorder_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, src_index, dst_index, src_row, lens, ctx);
  return TASU_OK;
}
extern "C" int tasu_attn_decode(const void* qkv, const void* kcache, const void* vcache, const int32_t* row_index,
                                const int32_t* kstart, const int32_t* lens, void* out, int M, int H, int G, int ctx, float scale,
                                int out_frag, void* stream) {
  if (!qkv || !kcache || !vcache || !kstart || !lens || !out || M <= 0 || H <= 0 || G <= 0 || H % G || ctx <= 0 ||
      ctx > MAX_CTX)
    return TASU_ERR_ARG;
  const int rep = H / G;
  const size_t lds = (size_t)tasu_attn_dec::attn_decode_lds_floats(rep, ctx) * sizeof(float);
  if (lds > 160 * 1024) return TASU_ERR_ARG;
#define DEC_CASE(R)                                                                                                   \
  case R: {                                                                                                           \
    static bool attr_set = false;                                                                                     \
    if (!attr_set) {                                                                                                  \
      (void)hipFuncSetAttribute((const void*)attn_decode_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize,        \
                                160 * 1024);                                                                          \
      attr_set = true;                                                                                                \
    }                                                                                                                 \
    TASU_LAUNCH(attn_decode_kernel<R>, dim3(M, G), dim3(64 * DEC_NW), lds, (hipStream_t)stream, (const bf16*)qkv,      \
                (const bf16*)kcache, (const bf16*)vcache, row_index, kstart, lens, (bf16*)out, H, G, ctx, scale, out_frag);       \
    return TASU_OK;                                                                                                   \
  }
  switch (rep) {
    DEC_CASE(1) DEC_CASE(2) DEC_CASE(4) DEC_CASE(6) DEC_CASE(7) DEC_CASE(8)
    default:
      return TASU_ERR_ARG;
  }
#undef DEC_CASE
}
#ifdef TASU_ATTN_TRACE
extern "C" int tasu_attn_trace_read(uint64_t* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(tasu_attn_dec::g_attn_trace), 16 * sizeof(uint64_t)) == hipSuccess ? 0 : 2;
}
#endif
extern "C" int tasu_embed_rows(const float* table, const int32_t* ids, float* x, int M, int D, void* stream) {
  if (!table || !ids || !x || M <= 0 || D <= 0 || D % 4) return TASU_ERR_ARG;
  TASU_LAUNCH(embed_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, table, ids, x, M, D);
  return TASU_OK;
}
