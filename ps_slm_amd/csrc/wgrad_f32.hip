// Weight gradients of the decoder's own tensors on the fp32 TRAINING step (train_config.freeze_llm = false with use_fp16 = false:
// Multitask/model/ps-slm.py:105-108 leaves every parameter of Qwen2ForCausalLM trainable, Multitask/utils/deepspeed_utils.py:205-236
// runs loss.backward() outside autocast).  The fp32 siblings of csrc/wgrad.hip:
//   tasu_f32_gemm_tn         C[N, K] = or += sum_r A[r, n] . B[r, k]             dW = dY^T X of a Linear, both operands fp32 and ROW-major
//   tasu_f32_rmsnorm_wgrad   dw[j] = or += sum_r dy[r, j] . x[r, j] . rstd[r]    the weight gradient of Qwen2RMSNorm
//   tasu_f32_colsum_split    out[c] = or += sum_r x[r, c]                         the q|k|v bias gradient (the same two-stage reduction)
// The reduction runs over the token rows.  v_mfma_f32_16x16x4_f32 takes from lane l the element [r0 + l / 16][c0 + l % 16] of BOTH
// operands -- four reduction rows, sixteen floats of each -- so both fragments are plain reads of row-major LDS tiles: no transposed
// copy in HBM, no transpose step in LDS.  The sixteen "columns" of a fragment need not be adjacent in memory either: lane c takes
// columns 4 c .. 4 c + 3 of a 64-wide strip as ONE 16-byte read and uses them as the c-th column of four MFMA sub-tiles (a fixed
// permutation of the output's rows / columns, undone by the store addressing), 4x fewer LDS instructions than one float per MFMA.
// Workgroup = 4 waves = a 128 x 128 output tile (each wave 64 x 64: 16 accumulators); a stage is 16 reduction rows of each operand
// (16 KiB), prefetched into registers under the previous stage's MFMAs (csrc/fp32.hip's f32_gemm_kernel scheme).  An output with few
// tiles fills the chip by cutting the rows into `nsplit` ranges, one fp32 slab each, which a second kernel sums in slab order:
// deterministic, no atomics.
#include "common.h"
#include "../../include/tasu_hip.h"

namespace {

constexpr int TS = 16;                                  // reduction rows per stage
constexpr int BT = 128;                                 // output tile (both ways) = columns of each operand per stage

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// four floats of row `row`, columns col .. col + 3 of an operand; zeros for rows >= R (whatever the buffer holds there never reaches
// C) and for column quads outside the operand (widths are multiples of 4: a quad is inside or outside as a whole); nothing outside
// [R, ncols] is read
__device__ __forceinline__ f32x4 tn_load(const float* __restrict__ src, int ld, int row, int R, int col, int ncols) {
  if (row < R && col < ncols) return *(const f32x4*)(src + (size_t)row * ld + col);
  return f32x4{0.f, 0.f, 0.f, 0.f};
}

// grid (tiles_n * tiles_k, nsplit).  out: C itself (nsplit == 1; ld_out = ldc, accumulate honoured) or slab blockIdx.y of the
// workspace (ld_out = K, slab stride N * K, plain stores).
__global__ __launch_bounds__(256, 2) void f32_gemm_tn_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                             float* __restrict__ out, int ld_out, size_t slab_stride, int R, int N, int K,
                                                             int tiles_k, int nsplit, int accumulate) {
  __shared__ __attribute__((aligned(16))) float sA[2][TS][BT];
  __shared__ __attribute__((aligned(16))) float sB[2][TS][BT];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int tn = blockIdx.x / tiles_k, tk = blockIdx.x % tiles_k;
  const int n0 = tn * BT, k0 = tk * BT;
  const int nstages = (R + TS - 1) / TS;
  const int s_lo = (int)((long long)nstages * blockIdx.y / nsplit), s_hi = (int)((long long)nstages * (blockIdx.y + 1) / nsplit);
  const int lr = t >> 5, lc = (t & 31) * 4;             // this thread's rows lr, lr + 8 and first column of the 16 x 128 stage tiles
  const int wn = wave >> 1, wk = wave & 1, q = lane >> 4, l15 = lane & 15;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 ra0, ra1, rb0, rb1;
  auto fetch = [&](int s) {
    const int r = s * TS + lr;
    ra0 = tn_load(A, lda, r, R, n0 + lc, N), ra1 = tn_load(A, lda, r + 8, R, n0 + lc, N);
    rb0 = tn_load(B, ldb, r, R, k0 + lc, K), rb1 = tn_load(B, ldb, r + 8, R, k0 + lc, K);
  };
  if (s_lo < s_hi) fetch(s_lo);
  int buf = 0;
  for (int s = s_lo; s < s_hi; ++s) {
    *(f32x4*)&sA[buf][lr][lc] = ra0, *(f32x4*)&sA[buf][lr + 8][lc] = ra1;
    *(f32x4*)&sB[buf][lr][lc] = rb0, *(f32x4*)&sB[buf][lr + 8][lc] = rb1;
    __syncthreads();
    if (s + 1 < s_hi) fetch(s + 1);                     // the next stage's 16 KiB are in flight under this one's MFMAs
#pragma unroll
    for (int rr = 0; rr < TS / 4; ++rr) {
      // lane (q, l15): reduction row 4 rr + q, columns 4 l15 .. + 3 of this wave's 64-wide strips
      const f32x4 fa = *(const f32x4*)&sA[buf][rr * 4 + q][wn * 64 + l15 * 4];
      const f32x4 fb = *(const f32x4*)&sB[buf][rr * 4 + q][wk * 64 + l15 * 4];
      // acc[i][j][r] = C[n0 + wn * 64 + 4 l15 + i][k0 + wk * 64 + 4 (4 q + r) + j]
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma4(fb[j], fa[i], acc[i][j]);
    }
    buf ^= 1;                                           // (the other buffer was last read before the barrier above)
  }
  float* dst = out + (size_t)blockIdx.y * slab_stride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + l15 * 4 + i;
    if (n >= N) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = k0 + wk * 64 + (q * 4 + r) * 4;
      if (k >= K) continue;                              // K % 4 == 0: the four columns are inside or outside together
      f32x4* p = (f32x4*)(dst + (size_t)n * ld_out + k);
      f32x4 v = f32x4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
      if (accumulate) {
        const f32x4 o = *p;
        v[0] += o[0], v[1] += o[1], v[2] += o[2], v[3] += o[3];
      }
      *p = v;
    }
  }
}

// C[n, k] = or += slab 0 + slab 1 + ... in that order; one thread per four columns
__global__ __launch_bounds__(256) void f32_sum_tn_slabs_kernel(const float* __restrict__ ws, int nsplit, size_t slab_stride, float* __restrict__ C,
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
// rstd[r] = 1 / sqrt(mean(x[r]^2) + eps) (modeling_qwen2.py:41-48), one wave per row; the sum of squares in double, so that the
// weight gradient's only roundings are those of its own three-factor terms
__global__ __launch_bounds__(256) void f32_row_rstd_kernel(const float* __restrict__ x, float* __restrict__ rstd, int R, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  const float* p = x + (size_t)row * D;
  double ss = 0.0;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = *(const f32x4*)(p + c);
    ss += (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (lane == 0) rstd[row] = (float)(1.0 / sqrt(ss / (double)D + (double)eps));
}

// RMSNorm weight gradient, stage 1: grid (ceil(D / 256), TASU_RMS_WGRAD_SPLIT).  A block owns 256 columns (lane -> four of them)
// and the rows r = y, y + SPLIT, ... of its slab; its four waves take every fourth of those and meet in LDS in wave order.
// NORM = false: plain column sums of dy (leading dimension ld) -- a bias gradient over thousands of rows, same two stages.
template <bool NORM>
__global__ __launch_bounds__(256) void f32_rmsnorm_wgrad_part_kernel(const float* __restrict__ dy, int ld, const float* __restrict__ x,
                                                                     const float* __restrict__ rstd, float* __restrict__ ws, int R, int D) {
  __shared__ f32x4 part[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.x * 256 + lane * 4;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c < D) {
    for (int r = blockIdx.y + wave * TASU_RMS_WGRAD_SPLIT; r < R; r += 4 * TASU_RMS_WGRAD_SPLIT) {
      const f32x4 d = *(const f32x4*)(dy + (size_t)r * ld + c);
      if constexpr (NORM) {
        const f32x4 v = *(const f32x4*)(x + (size_t)r * D + c);
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
__global__ __launch_bounds__(256) void f32_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, int D, int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  float s = ws[j];
  for (int i = 1; i < TASU_RMS_WGRAD_SPLIT; ++i) s += ws[(size_t)i * D + j];
  dw[j] = accumulate ? dw[j] + s : s;
}

}  // namespace

// how many row ranges tasu_f32_gemm_tn should cut R into so that about two workgroups per CU exist (host code, no launch)
extern "C" int tasu_f32_gemm_tn_split(int R, int N, int K) {
  if (R <= 0 || N <= 0 || K <= 0) return -1;
  const long long tiles = (long long)((N + BT - 1) / BT) * ((K + BT - 1) / BT);
  const int nstages = (R + TS - 1) / TS;
  long long want = 512 / tiles;
  if (want > TASU_F32_GEMM_TN_MAX_SPLIT) want = TASU_F32_GEMM_TN_MAX_SPLIT;
  if (want > nstages) want = nstages;
  return want < 1 ? 1 : (int)want;
}

extern "C" int tasu_f32_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int R, int N, int K, int accumulate,
                                int nsplit, float* ws, int64_t ws_floats, void* stream) {
  if (!A || !B || !C || R <= 0 || N <= 0 || K <= 0 || N % 4 || K % 4 || lda % 4 || ldb % 4 || ldc % 4 || lda < N || ldb < K || ldc < K)
    return TASU_ERR_ARG;
  if (((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)C & 15)) return TASU_ERR_ARG;
  const int nstages = (R + TS - 1) / TS;
  if (nsplit < 1 || nsplit > TASU_F32_GEMM_TN_MAX_SPLIT || nsplit > nstages) return TASU_ERR_ARG;
  const size_t slab = (size_t)N * K;
  if (nsplit > 1 && (!ws || ((uintptr_t)ws & 15) || ws_floats < (int64_t)(slab * nsplit))) return TASU_ERR_ARG;
  const long long tiles_n = (N + BT - 1) / BT, tiles_k = (K + BT - 1) / BT;
  if (tiles_n * tiles_k > 0x7fffffffLL) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(tiles_n * tiles_k), nsplit);
  if (nsplit == 1) {
    TASU_LAUNCH(f32_gemm_tn_kernel, grid, dim3(256), 0, st, A, lda, B, ldb, C, ldc, (size_t)0, R, N, K, (int)tiles_k, 1, accumulate ? 1 : 0);
    return TASU_OK;
  }
  TASU_LAUNCH(f32_gemm_tn_kernel, grid, dim3(256), 0, st, A, lda, B, ldb, ws, K, slab, R, N, K, (int)tiles_k, nsplit, 0);
  const size_t quads = slab / 4;
  TASU_LAUNCH(f32_sum_tn_slabs_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, (const float*)ws, nsplit, slab, C, ldc, N, K,
              accumulate ? 1 : 0);
  return TASU_OK;
}

extern "C" int tasu_f32_rmsnorm_wgrad(const float* dy, const float* x, const float* rstd, float* dw, float* ws, int64_t ws_floats, int R, int D,
                                      float eps, int accumulate, void* stream) {
  if (!dy || !x || !dw || !ws || R <= 0 || D <= 0 || D % 4) return TASU_ERR_ARG;
  if (((uintptr_t)dy & 15) || ((uintptr_t)x & 15) || ((uintptr_t)ws & 15)) return TASU_ERR_ARG;
  const int64_t slabs = (int64_t)TASU_RMS_WGRAD_SPLIT * D;
  if (ws_floats < slabs + (rstd ? 0 : R)) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (!rstd) {                                           // recomputed from x and eps, as tasu_f32_rmsnorm_bwd does: behind the slabs
    float* rs = ws + slabs;
    TASU_LAUNCH(f32_row_rstd_kernel, dim3((R + 3) / 4), dim3(256), 0, st, x, rs, R, D, eps);
    rstd = rs;
  }
  TASU_LAUNCH(f32_rmsnorm_wgrad_part_kernel<true>, dim3((D + 255) / 256, TASU_RMS_WGRAD_SPLIT), dim3(256), 0, st, dy, D, x, rstd, ws, R, D);
  TASU_LAUNCH(f32_wgrad_sum_kernel, dim3((D + 255) / 256), dim3(256), 0, st, (const float*)ws, dw, D, accumulate ? 1 : 0);
  return TASU_OK;
}

extern "C" int tasu_f32_colsum_split(const float* x, int ld, float* out, float* ws, int R, int C, int accumulate, void* stream) {
  if (!x || !out || !ws || R <= 0 || C <= 0 || C % 4 || ld % 4 || ld < C) return TASU_ERR_ARG;
  if (((uintptr_t)x & 15) || ((uintptr_t)ws & 15)) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  TASU_LAUNCH(f32_rmsnorm_wgrad_part_kernel<false>, dim3((C + 255) / 256, TASU_RMS_WGRAD_SPLIT), dim3(256), 0, st, x, ld, (const float*)nullptr,
              (const float*)nullptr, ws, R, C);
  TASU_LAUNCH(f32_wgrad_sum_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const float*)ws, out, C, accumulate ? 1 : 0);
  return TASU_OK;
}
