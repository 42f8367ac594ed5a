// Weight gradients of the decoder's own tensors (full fine-tuning of the LLM, train_config.freeze_llm = false):
//   tasu_gemm_tn_bf16    C[N, K] (fp32) = or += sum_r A[r, n] . B[r, k]     dW = dY^T X of a Linear, both operands ROW-major as the
//                                                                            step leaves them ([rows, out] and [rows, in], bf16)
//   tasu_rmsnorm_wgrad   dw[j] = or += sum_r dy[r, j] . x[r, j] . rstd[r]    the weight gradient of Qwen2RMSNorm
//   tasu_colsum_bf16_split  out[c] = or += sum_r x[r, c]                     the q|k|v bias gradient (the same two-stage reduction)
// The reduction runs over the token rows, so BOTH operands of the GEMM are "K-major" for the MFMA: no transposed copy is made in
// HBM (the composed route -- two tasu_transpose_bf16 + the NT GEMM -- moves every operand twice more); a stage of 64 rows of each
// operand goes into LDS as it lies (LDS-DMA, whole 128-byte lines) and both are read back as MFMA fragments with the hardware
// transpose read, the image and addressing of rank_gemm_tn_kernel (gemm_rank.hip).  Workgroup = 4 waves = a 128 x 128 output tile
// (each wave 64 x 64: 16 accumulators), two stages in flight (the DMA of stage s + 1 runs under the MFMAs of stage s).  An output
// with few tiles (o_proj at Qwen2.5-1.5B: 12 x 12) fills the chip by cutting the rows into `nsplit` ranges, one fp32 slab each,
// which a second kernel sums in slab order: deterministic, no atomics.
#include "common.h"
#include "../../include/tasu_hip.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int TS = 64;                                  // rows (the reduction) per stage
constexpr int IMG = TS * 128;                           // one image: 64 rows x 64 columns bf16, 16-byte chunk c of row r at c ^ (r & 7)
constexpr int STAGE = 4 * IMG;                          // A columns 0..63 | A 64..127 | B 0..63 | B 64..127
constexpr int TN_LDS = 2 * STAGE;

// wave `img` of the workgroup stages image `img` of one stage: 8 DMA instructions of 8 rows x 128 bytes.  Rows past R - 1 read row
// R - 1 (and are zeroed in LDS afterwards: tn_zero_tail), 16-byte column chunks past the operand's width read chunk 0 of the row
// (their products land in accumulators that are never stored).
__device__ __forceinline__ void tn_stage_load(const bf16* __restrict__ src, int ld, int ncols, int col0, int r0, int R, char* img, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int kr = i * 8 + (lane >> 3), c = (lane & 7) ^ (kr & 7);
    const int col = col0 + c * 8;
    const bf16* g = src + (size_t)min(r0 + kr, R - 1) * ld + (col < ncols ? col : 0);
    __builtin_amdgcn_global_load_lds((glb_void*)g, (lds_void*)(img + i * 1024), 16, 0, 0);
  }
}

__device__ __forceinline__ void tn_zero_tail(char* img, int valid, int lane) {
  for (int kr = valid + (lane >> 3); kr < TS; kr += 8) *(u32x4*)(img + kr * 128 + (lane & 7) * 16) = u32x4{0u, 0u, 0u, 0u};
}

// grid (tiles_n * tiles_k, nsplit).  out: C itself (nsplit == 1; ld_out = ldc, accumulate honoured) or slab blockIdx.y of the
// workspace (ld_out = K, slab stride N * K, plain stores).
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(const bf16* __restrict__ A, int lda, const bf16* __restrict__ B, int ldb,
                                                         float* __restrict__ out, int ld_out, size_t slab_stride, int R, int N, int K,
                                                         int tiles_k, int nsplit, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tn = blockIdx.x / tiles_k, tk = blockIdx.x % tiles_k;
  const int n0 = tn * 128, k0 = tk * 128;
  const int nstages = (R + TS - 1) / TS;
  const int s_lo = (int)((long long)nstages * blockIdx.y / nsplit), s_hi = (int)((long long)nstages * (blockIdx.y + 1) / nsplit);
  // this wave's image of every stage
  const bool is_a = wave < 2;
  const bf16* src = is_a ? A : B;
  const int ld = is_a ? lda : ldb, ncols = is_a ? N : K, col0 = (is_a ? n0 : k0) + (wave & 1) * 64;
  const int my_img = wave * IMG;
  // ... and the images it computes from: output rows n0 + wn * 64 .., columns k0 + wk * 64 ..
  const int wn = wave >> 1, wk = wave & 1;
  const int q = lane >> 4, l15 = lane & 15, pp = lane & 3, qq = (lane >> 2) & 3;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (s_lo < s_hi) {
    tn_stage_load(src, ld, ncols, col0, s_lo * TS, R, smem + my_img, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (R - s_lo * TS < TS) tn_zero_tail(smem + my_img, R - s_lo * TS, lane);
    __syncthreads();
  }
  for (int s = s_lo; s < s_hi; ++s) {
    char* cur = smem + ((s - s_lo) & 1) * STAGE;
    char* nxt = smem + ((s - s_lo + 1) & 1) * STAGE;
    if (s + 1 < s_hi) tn_stage_load(src, ld, ncols, col0, (s + 1) * TS, R, nxt + my_img, lane);
    const char* ia = cur + wn * IMG;
    const char* ib = cur + (2 + wk) * IMG;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      // lane group q takes reduction rows {4q .. 4q + 3, 16 + 4q .. 16 + 4q + 3} of the 32-block for BOTH operands
      const int ra = kk * 32 + 4 * q + qq, rb = ra + 16;
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ch = i * 2 + (pp >> 1), inner = (pp & 1) * 8;
        const int oa = ra * 128 + ((ch ^ (ra & 7)) << 4) + inner, ob = rb * 128 + ((ch ^ (rb & 7)) << 4) + inner;
        union { s16x4 h[2]; bf16x8 b; } u, v;
        u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(ia + oa));
        u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(ia + ob));
        v.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(ib + oa));
        v.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(ib + ob));
        fa[i] = u.b, fb[i] = v.b;
      }
      // acc[i][j][r] = C[n0 + wn * 64 + i * 16 + (lane & 15)][k0 + wk * 64 + j * 16 + (lane >> 4) * 4 + r]
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(fb[j], fa[i], acc[i][j]);
    }
    // the next stage has landed (this wave's image) and, for a short last stage, lost its rows past R; behind the barrier every
    // wave is done reading `cur`, which the DMA of the iteration after next overwrites
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (s + 1 < s_hi && R - (s + 1) * TS < TS) tn_zero_tail(nxt + my_img, R - (s + 1) * TS, lane);
    __syncthreads();
  }
  float* dst = out + (size_t)blockIdx.y * slab_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + i * 16 + l15;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + wk * 64 + j * 16 + q * 4;
      if (k >= K) continue;                              // K % 4 == 0: the four columns are inside or outside together
      f32x4* p = (f32x4*)(dst + (size_t)n * ld_out + k);
      f32x4 v = acc[i][j];
      if (accumulate) {
        const f32x4 o = *p;
        v[0] += o[0], v[1] += o[1], v[2] += o[2], v[3] += o[3];
      }
      *p = v;
    }
  }
}

// C[n, k] = or += slab 0 + slab 1 + ... in that order; one thread per four columns
__global__ __launch_bounds__(256) void sum_tn_slabs_kernel(const float* __restrict__ ws, int nsplit, size_t slab_stride, float* __restrict__ C,
                                                           int ldc, int N, int K, int accumulate) {
  const int kq = K >> 2;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)N * kq) return;
  const int n = (int)(idx / kq), k = (int)(idx % kq) * 4;
  const float* p = ws + (size_t)n * K + k;
  f32x4 s = *(const f32x4*)p;
  for (int i = 1; i < nsplit; ++i) {
    const f32x4 v = *(const f32x4*)(p + i * slab_stride);
    s[0] += v[0], s[1] += v[1], s[2] += v[2], s[3] += v[3];
  }
  f32x4* o = (f32x4*)(C + (size_t)n * ldc + k);
  if (accumulate) {
    const f32x4 v = *o;
    s[0] += v[0], s[1] += v[1], s[2] += v[2], s[3] += v[3];
  }
  *o = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// RMSNorm weight gradient, stage 1: grid (ceil(D / 256), TASU_RMS_WGRAD_SPLIT).  A block owns 256 columns (lane -> four of them)
// and the rows r = y, y + SPLIT, ... of its slab; its four waves take every fourth of those and meet in LDS in wave order.
// NORM = false: plain column sums of dy (leading dimension ld) -- a bias gradient over thousands of rows, same two stages.
template <bool NORM>
__global__ __launch_bounds__(256) void rmsnorm_wgrad_part_kernel(const bf16* __restrict__ dy, int ld, const float* __restrict__ x,
                                                                 const float* __restrict__ rstd, const int32_t* __restrict__ src_rows,
                                                                 float* __restrict__ ws, int R, int D) {
  __shared__ f32x4 part[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 256 + lane * 4;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c < D) {
    for (int r = blockIdx.y + wave * TASU_RMS_WGRAD_SPLIT; r < R; r += 4 * TASU_RMS_WGRAD_SPLIT) {
      const f32x4 d = __builtin_convertvector(*(const bf16x4*)(dy + (size_t)r * ld + c), f32x4);
      if constexpr (NORM) {
        const int xr = src_rows ? src_rows[r] : r;
        if (xr < 0) continue;
        const f32x4 v = *(const f32x4*)(x + (size_t)xr * D + c);
        const float rs = rstd[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += d[j] * v[j] * rs;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += d[j];
      }
    }
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < D) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const f32x4 v = part[w][lane];
      s[0] += v[0], s[1] += v[1], s[2] += v[2], s[3] += v[3];
    }
    *(f32x4*)(ws + (size_t)blockIdx.y * D + c) = s;
  }
}

// stage 2: dw[j] = or += the slabs' partial sums in slab order
__global__ __launch_bounds__(256) void rmsnorm_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, int D, int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  float s = ws[j];
  for (int i = 1; i < TASU_RMS_WGRAD_SPLIT; ++i) s += ws[(size_t)i * D + j];
  dw[j] = accumulate ? dw[j] + s : s;
}

}  // namespace

// how many row ranges tasu_gemm_tn_bf16 should cut R into so that about two workgroups per CU exist (host code, no launch)
extern "C" int tasu_gemm_tn_bf16_split(int R, int N, int K) {
  if (R <= 0 || N <= 0 || K <= 0) return -1;
  const long long tiles = (long long)((N + 127) / 128) * ((K + 127) / 128);
  const int nstages = (R + TS - 1) / TS;
  long long want = 512 / tiles;
  if (want > TASU_GEMM_TN_MAX_SPLIT) want = TASU_GEMM_TN_MAX_SPLIT;
  if (want > nstages) want = nstages;
  return want < 1 ? 1 : (int)want;
}

extern "C" int tasu_gemm_tn_bf16(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int R, int N, int K, int accumulate,
                                 int nsplit, float* ws, int64_t ws_floats, void* stream) {
  if (!A || !B || !C || R <= 0 || N <= 0 || K <= 0 || N % 8 || K % 8 || lda % 8 || ldb % 8 || ldc % 4 || lda < N || ldb < K || ldc < K)
    return TASU_ERR_ARG;
  if (((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)C & 15)) return TASU_ERR_ARG;
  const int nstages = (R + TS - 1) / TS;
  if (nsplit < 1 || nsplit > TASU_GEMM_TN_MAX_SPLIT || nsplit > nstages) return TASU_ERR_ARG;
  const size_t slab = (size_t)N * K;
  if (nsplit > 1 && (!ws || ((uintptr_t)ws & 15) || ws_floats < (int64_t)(slab * nsplit))) return TASU_ERR_ARG;
  const long long tiles_n = (N + 127) / 128, tiles_k = (K + 127) / 128;
  if (tiles_n * tiles_k > 0x7fffffffLL) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)gemm_tn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS);
    attr_set = true;
  }
  const dim3 grid((unsigned)(tiles_n * tiles_k), nsplit);
  if (nsplit == 1) {
    TASU_LAUNCH(gemm_tn_kernel, grid, dim3(256), TN_LDS, st, (const bf16*)A, lda, (const bf16*)B, ldb, C, ldc, (size_t)0, R, N, K, (int)tiles_k, 1,
                accumulate ? 1 : 0);
    return TASU_OK;
  }
  TASU_LAUNCH(gemm_tn_kernel, grid, dim3(256), TN_LDS, st, (const bf16*)A, lda, (const bf16*)B, ldb, ws, K, slab, R, N, K, (int)tiles_k, nsplit, 0);
  const size_t quads = slab / 4;
  TASU_LAUNCH(sum_tn_slabs_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, (const float*)ws, nsplit, slab, C, ldc, N, K,
              accumulate ? 1 : 0);
  return TASU_OK;
}

extern "C" int tasu_rmsnorm_wgrad(const void* dy_bf16, const float* x, const float* rstd, const int32_t* src_rows, float* dw, float* ws, int R,
                                  int D, int accumulate, void* stream) {
  if (!dy_bf16 || !x || !rstd || !dw || !ws || R <= 0 || D <= 0 || D % 4) return TASU_ERR_ARG;
  if (((uintptr_t)dy_bf16 & 7) || ((uintptr_t)x & 15) || ((uintptr_t)ws & 15)) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  TASU_LAUNCH(rmsnorm_wgrad_part_kernel<true>, dim3((D + 255) / 256, TASU_RMS_WGRAD_SPLIT), dim3(256), 0, st, (const bf16*)dy_bf16, D, x, rstd,
              src_rows, ws, R, D);
  TASU_LAUNCH(rmsnorm_wgrad_sum_kernel, dim3((D + 255) / 256), dim3(256), 0, st, (const float*)ws, dw, D, accumulate ? 1 : 0);
  return TASU_OK;
}

extern "C" int tasu_colsum_bf16_split(const void* x, int ld, float* out, float* ws, int R, int C, int accumulate, void* stream) {
  if (!x || !out || !ws || R <= 0 || C <= 0 || C % 4 || ld % 4 || ld < C) return TASU_ERR_ARG;
  if (((uintptr_t)x & 7) || ((uintptr_t)ws & 15)) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  TASU_LAUNCH(rmsnorm_wgrad_part_kernel<false>, dim3((C + 255) / 256, TASU_RMS_WGRAD_SPLIT), dim3(256), 0, st, (const bf16*)x, ld,
              (const float*)nullptr, (const float*)nullptr, (const int32_t*)nullptr, ws, R, C);
  TASU_LAUNCH(rmsnorm_wgrad_sum_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const float*)ws, out, C, accumulate ? 1 : 0);
  return TASU_OK;
}
