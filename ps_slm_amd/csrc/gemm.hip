// bf16 "NT" GEMM for gfx950:  C[M,N] (+)= A[M,K] . B[N,K]^T (+ bias[N])
//
// Both operands are K-contiguous (A = activations, token-major; B = an nn.Linear weight [out,in] or its
// pre-transposed copy for dgrad), so the SAME kernel serves forward, dgrad (against the resident W^T copy)
// and wgrad (against transposed activations).  Replaces every torch.nn.functional.linear on the reference
// hot path (transformers modeling_qwen2.py q/k/v/o/gate/up/down/lm_head; Multitask/model/projector.py:141-143).
//
// Structure: 128x128 tile, BK = 64, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16x32 tiles.
// A/B tiles go global -> LDS with global_load_lds_dwordx4 (no VGPR round trip), double-buffered, one barrier
// per K-step.  The LDS image is lane-linear (a glds constraint), so the bank-conflict swizzle is applied on
// the per-lane SOURCE address and again on the ds_read_b128 address (16-B chunk c of row r lives at chunk
// c ^ ((r>>1)&7): conflict-free for the 16x16x32 operand read).  The MFMA is issued with the weight fragment
// as the A operand so that every lane ends up with 4 CONSECUTIVE output columns of one row (8-/16-byte
// stores).  blockIdx is remapped so that each XCD (private L2) works on a contiguous band of tiles.
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "common.h"
#include "gemm_dispatch.h"

namespace {

constexpr int BK = 64;

struct GemmArgs {
  const bf16* A;
  const bf16* B;
  void* C;
  const float* R;
  const bf16* bias;
  int M, N, K;
  int lda, ldb, ldc;
  int tiles_m, tiles_n;
  int ksplit;           // > 1: blockIdx covers tiles x ksplit, every block reduces K-steps [ks*per, (ks+1)*per)
  float* partial;       // [tiles][ksplit][BM*BN] fp32 partial tiles (register-image order)
  int* counters;        // [tiles] arrival counters, zero between launches (the last arriver resets its tile's)
};

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

// BM x BN block tile (BM, BN multiples of 32), 2x2 waves, wave tile (BM/2) x (BN/2) = MI x NI MFMA tiles.
// BN = 96 exists for N = 1536 at M = 4096: 32 x 16 = 512 tiles = exactly two per CU (128x128 would give 384 tiles and
// leave half of the CUs with one block).
// 256 x 256 / 8 waves (2 x 4, wave tile 128 x 64, one block per CU) halves the L2 -> LDS bytes per FLOP of the 128-wide
// tiles ((BM+BN)/(BM*BN): 1/128 vs 1/64); the 128-wide tiles run at roughly the chip's L2 bandwidth (2 x 32 KB per
// K-step per CU), which is what caps them near 1 PFLOP/s.
//
// SPLITK: grids that cannot fill the chip with whole tiles (M = 4096 x N = 1536 is 128 tiles of 256 x 192) split the K
// range over `ksplit` blocks per tile.  Every block writes its fp32 partial tile to the workspace, fences at agent
// scope (the 8 XCD L2s are not coherent with each other without it) and takes a ticket from the tile's arrival counter;
// the LAST arriver adds the partials in split order (ksplit == 2: own + other, which is order-independent) and runs the
// normal epilogue.  No spinning, so no co-residency requirement; bitwise deterministic.
template <int BM, int BN, int NWM, int NWN, int OUT_MODE, bool HAS_BIAS, int SCHED, bool SPLITK = false>
__global__ __launch_bounds__(64 * NWM * NWN, 2) void gemm_nt_kernel(GemmArgs p) {
  constexpr int NW = NWM * NWN, NT = 64 * NW;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int WM = BM / NWM, WN = BN / NWN, MI = WM / 16, NI = WN / 16;
  constexpr int PA = BM / 8 / NW, PB = BN / 8 / NW;   // 1-KiB pieces (8 rows x 128 B) staged per wave and K-step
  static_assert(PA * NW * 8 == BM && PB * NW * 8 == BN, "tile rows must split evenly over the waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave / NWN, wc = wave % NWN;
  (void)NT;

  // ---- XCD-aware, bijective block -> tile map, then an 8-row-group raster for L2 reuse of the B panel.
  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  int ks = 0;
  if (SPLITK) {
    ks = logical % p.ksplit;
    logical /= p.ksplit;
  }
  const int tile_id = logical;
  constexpr int GROUP_M = 8;
  const int per_group = GROUP_M * p.tiles_n;
  const int gid = logical / per_group;
  const int first_m = gid * GROUP_M;
  const int gsz = min(p.tiles_m - first_m, GROUP_M);
  const int in_g = logical - gid * per_group;
  const int tm = first_m + in_g % gsz;
  const int tn = in_g / gsz;
  const int row0 = tm * BM, col0 = tn * BN;

  // ---- per-lane global source pointers for the pieces this wave stages (4 of A, 4 of B per K-step).
  // piece pc = 8 tile rows x 128 B; lane l -> tile row pc*8 + (l>>3), LDS chunk l&7, which must hold
  // global chunk (l&7) ^ ((row>>1)&7).
  const bf16* ga[PA];
  const bf16* gb[PB];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int r = (wave * PA + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    ga[i] = p.A + (size_t)min(row0 + r, p.M - 1) * p.lda + c * 8 - (i & 3) * 512;   // - the immediate offset of stage()
  }
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int r = (wave * PB + i) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    gb[i] = p.B + (size_t)min(col0 + r, p.N - 1) * p.ldb + c * 8 - (i & 3) * 512;
  }

  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * STAGE_BYTES;
    const int koff = kt * BK;
    // one M0 (LDS base) per four pieces: the immediate offset (i & 3) KiB moves the LDS address and the global address
    // alike, and the per-lane pointers were lowered by the same amount (see gemm_pipe.hip)
    auto one_a = [&](auto ic) {
      constexpr int i = decltype(ic)::value;
      __builtin_amdgcn_global_load_lds((glb_void*)(ga[i] + koff), (lds_void*)(base + (wave * PA + (i & ~3)) * 1024), 16,
                                       (i & 3) * 1024, 0);
    };
    auto one_b = [&](auto ic) {
      constexpr int i = decltype(ic)::value;
      __builtin_amdgcn_global_load_lds((glb_void*)(gb[i] + koff), (lds_void*)(base + A_BYTES + (wave * PB + (i & ~3)) * 1024), 16,
                                       (i & 3) * 1024, 0);
    };
    [&]<int... I>(std::integer_sequence<int, I...>) { (one_a(std::integral_constant<int, I>{}), ...); }(std::make_integer_sequence<int, PA>{});
    [&]<int... I>(std::integer_sequence<int, I...>) { (one_b(std::integral_constant<int, I>{}), ...); }(std::make_integer_sequence<int, PB>{});
  };

  // ---- per-lane LDS read offsets (bytes) for the two 32-deep k sub-steps.
  const int sw = (lane >> 1) & 7;
  int roff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) roff[kk] = (lane & 15) * 128 + (((kk * 4 + (lane >> 4)) ^ sw) << 4);

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int kbeg = 0, nk = p.K / BK;
  if (SPLITK) {
    const int per = (nk + p.ksplit - 1) / p.ksplit;
    kbeg = ks * per;
    nk = min(nk, kbeg + per);
  }
  if (kbeg < nk) stage(0, kbeg);
  __syncthreads();
  for (int kt = kbeg; kt < nk; ++kt) {
    const int cur = (kt - kbeg) & 1;
    if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
    const char* sa = smem + cur * STAGE_BYTES + (wr * WM) * 128;
    const char* sb = smem + cur * STAGE_BYTES + A_BYTES + (wc * WN) * 128;
    // all fragment reads of the K-step are issued up front (both 32-deep sub-steps): the second half lands under
    // the first half's MFMAs instead of stalling the wave between the two halves.
    bf16x8 fa[2][MI], fb[2][NI];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[kk][i] = *(const bf16x8*)(sa + i * 16 * 128 + roff[kk]);
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[kk][j] = *(const bf16x8*)(sb + j * 16 * 128 + roff[kk]);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = mfma16(fb[kk][j], fa[kk][i], acc[i][j]);
    if (SCHED == 1) {
      // pin the issue order (hipcc otherwise re-serialises reads -> wait -> MFMAs per half): first half's reads, then
      // the second half's reads interleaved one per two MFMAs of the first half, then the remaining MFMAs.
      __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);
#pragma unroll
      for (int r = 0; r < MI + NI; ++r) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * MI * NI - 2 * (MI + NI), 0);
    }
    __syncthreads();
  }

  if (SPLITK) {
    constexpr int TILE_F = BM * BN;
    float* mine = p.partial + ((size_t)tile_id * p.ksplit + ks) * TILE_F;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) *(f32x4*)(mine + ((i * NI + j) * NT + tid) * 4) = acc[i][j];
    __threadfence();                       // release: partial tile visible device-wide before the ticket
    __syncthreads();
    int* flag = (int*)smem;
    if (tid == 0) flag[0] = atomicAdd(p.counters + tile_id, 1);
    __syncthreads();
    if (flag[0] != p.ksplit - 1) return;   // not the last arriver of this tile
    __threadfence();                       // acquire: the other blocks' partials
    if (tid == 0) p.counters[tile_id] = 0; // leave the counter ready for the next launch
    const float* base = p.partial + (size_t)tile_id * p.ksplit * TILE_F;
    if (p.ksplit == 2) {
      const float* other = base + (size_t)(1 - ks) * TILE_F;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] += *(const f32x4*)(other + ((i * NI + j) * NT + tid) * 4);
    } else {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          f32x4 s = *(const f32x4*)(base + ((i * NI + j) * NT + tid) * 4);
          for (int k2 = 1; k2 < p.ksplit; ++k2) s += *(const f32x4*)(base + (size_t)k2 * TILE_F + ((i * NI + j) * NT + tid) * 4);
          acc[i][j] = s;
        }
    }
  }

  // ---- epilogue.  acc[i][j][r] = C[m][n], m = row0 + wr*WM + i*16 + (lane&15),
  //                                        n = col0 + wc*WN + j*16 + (lane>>4)*4 + r.
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = row0 + wr * WM + i * 16 + (lane & 15);
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = col0 + wc * WN + j * 16 + (lane >> 4) * 4;
      if (n >= p.N) continue;
      f32x4 v = acc[i][j];
      if (HAS_BIAS) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < p.N) v[r] += (float)p.bias[n + r];
      }
      const size_t off = (size_t)m * p.ldc + n;
      const bool full = (n + 4 <= p.N);
      if (OUT_MODE == TASU_GEMM_OUT_BF16) {
        bf16* c = (bf16*)p.C + off;
        bf16x4 o = __builtin_convertvector(v, bf16x4);
        if (full && ((off & 3) == 0)) {
          *(bf16x4*)c = o;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < p.N) c[r] = o[r];
        }
      } else if (OUT_MODE == TASU_GEMM_OUT_F32) {
        float* c = (float*)p.C + off;
        if (full && ((off & 3) == 0)) {
          *(f32x4*)c = v;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < p.N) c[r] = v[r];
        }
      } else {  // TASU_GEMM_OUT_F32_RESID_BF16R: C(fp32) = R(fp32) + bf16_round(result)  (autocast residual add)
        float* c = (float*)p.C + off;
        const float* rs = p.R + off;
        f32x4 rr = __builtin_convertvector(__builtin_convertvector(v, bf16x4), f32x4);
        if (full && ((off & 3) == 0)) {
          const f32x4 old = *(const f32x4*)rs;
          *(f32x4*)c = old + rr;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < p.N) c[r] = rs[r] + rr[r];
        }
      }
    }
  }
}

template <int BM, int BN, int NWM, int NWN, int OUT_MODE, bool HAS_BIAS, int SCHED, bool SPLITK = false>
int launch(GemmArgs a, hipStream_t st) {
  constexpr int LDS = 2 * (BM + BN) * BK * 2;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)gemm_nt_kernel<BM, BN, NWM, NWN, OUT_MODE, HAS_BIAS, SCHED, SPLITK>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    attr_set = true;
  }
  a.tiles_m = (a.M + BM - 1) / BM;
  a.tiles_n = (a.N + BN - 1) / BN;
  ++tasu_gemm::gemm_launches();
  TASU_LAUNCH((gemm_nt_kernel<BM, BN, NWM, NWN, OUT_MODE, HAS_BIAS, SCHED, SPLITK>),
              dim3(a.tiles_m * a.tiles_n * (SPLITK ? a.ksplit : 1)), dim3(64 * NWM * NWN), LDS, st, a);
  return TASU_OK;
}

template <int OUT_MODE, bool HAS_BIAS>
int launch_tiled(const GemmArgs& a, int bn, hipStream_t st) {
  if (bn == 256) return launch<256, 256, 2, 4, OUT_MODE, HAS_BIAS, 1>(a, st);
  if (bn == 192)
    return a.ksplit > 1 ? launch<256, 192, 2, 4, OUT_MODE, HAS_BIAS, 1, true>(a, st)
                        : launch<256, 192, 2, 4, OUT_MODE, HAS_BIAS, 1>(a, st);
  if (tasu_gemm::lab_switches().sched == 1)
    return bn == 96 ? launch<128, 96, 2, 2, OUT_MODE, HAS_BIAS, 1>(a, st) : launch<128, 128, 2, 2, OUT_MODE, HAS_BIAS, 1>(a, st);
  return bn == 96 ? launch<128, 96, 2, 2, OUT_MODE, HAS_BIAS, 0>(a, st) : launch<128, 128, 2, 2, OUT_MODE, HAS_BIAS, 0>(a, st);
}

// Launches what plan_nt (gemm_dispatch.h) decided for the problem in `a` (make_args; a.relu is the one epilogue option here and
// reaches the gemm_pipe / gemm_pp kernels only).  workspace: that of tasu_gemm_nt_bf16_ws, or nullptr.
int run_nt(const tasu_gemm::Plan& p, const tasu_gemm::Args& a, int out_mode, void* workspace, size_t ws_bytes, hipStream_t st) {
  switch (p.kind) {
    case TASU_GEMM_PLAN_PP256:
    case TASU_GEMM_PLAN_PP256_STREAMK:
      return tasu_gemm_pp_dispatch(a, out_mode, st, p.streamk ? workspace : nullptr, p.streamk ? ws_bytes : 0, p.sk_rem);
    case TASU_GEMM_PLAN_PP256_PLUS_PIPE128:
    case TASU_GEMM_PLAN_PP256_PLUS_PIPE192: {
      tasu_gemm::Args main = a, tail = a;
      main.n1 = tail.n0 = p.n_main;
      const int rc = tasu_gemm_pp_dispatch(main, out_mode, st, nullptr, 0, p.sk_rem);
      return rc ? rc : tasu_gemm_pipe_dispatch(tail, out_mode, p.bn, st);
    }
    case TASU_GEMM_PLAN_PIPE128:
    case TASU_GEMM_PLAN_PIPE192:
    case TASU_GEMM_PLAN_PIPE96:
      return tasu_gemm_pipe_dispatch(a, out_mode, p.bn, st);
    case TASU_GEMM_PLAN_TILE192_SPLITK:
    case TASU_GEMM_PLAN_TILES:
      break;
    default:
      return TASU_ERR_ARG;
  }
  GemmArgs g{a.A, a.B, a.C, a.R, a.bias, a.M, a.N, a.K, a.lda, a.ldb, a.ldc, 0, 0, p.ksplit, nullptr, nullptr};
  if (p.ksplit > 1) {
    g.counters = (int*)workspace;
    g.partial = (float*)((char*)workspace + TASU_GEMM_WS_COUNTERS * sizeof(int));
  }
  const bool hb = a.bias != nullptr;
  switch (out_mode) {
    case TASU_GEMM_OUT_BF16:
      return hb ? launch_tiled<TASU_GEMM_OUT_BF16, true>(g, p.bn, st) : launch_tiled<TASU_GEMM_OUT_BF16, false>(g, p.bn, st);
    case TASU_GEMM_OUT_F32:
      return hb ? launch_tiled<TASU_GEMM_OUT_F32, true>(g, p.bn, st) : launch_tiled<TASU_GEMM_OUT_F32, false>(g, p.bn, st);
    case TASU_GEMM_OUT_F32_RESID_BF16R:
      return hb ? launch_tiled<TASU_GEMM_OUT_F32_RESID_BF16R, true>(g, p.bn, st)
                : launch_tiled<TASU_GEMM_OUT_F32_RESID_BF16R, false>(g, p.bn, st);
    default:
      return TASU_ERR_ARG;
  }
}

// The pointer half of the contract of tasu_gemm_nt_bf16_ws (the shape half is plan_nt's)
int check_operands(const void* A, int lda, const void* B, int ldb, const void* C, const float* resid, int out_mode, const void* workspace) {
  if (!A || !B || !C || lda % 8 != 0 || ldb % 8 != 0) return TASU_ERR_ARG;
  if (((uintptr_t)A & 15) || ((uintptr_t)B & 15) || ((uintptr_t)workspace & 15)) return TASU_ERR_ARG;
  if (out_mode == TASU_GEMM_OUT_F32_RESID_BF16R && !resid) return TASU_ERR_ARG;
  return TASU_OK;
}

// Plan, then launch the plan.  out_mode: TASU_GEMM_OUT_* or tasu_gemm::OUT_DSWIGLU (`resid` is then the saved gate|up matrix, bf16
// [M, 2N], C = dgu [M, 2N]; kUnsupported where the plan is not a gemm_pipe / gemm_pp kernel, and tasu_gemm_dswiglu runs the two-kernel
// form).  relu_fused (optional): the caller wants C = bf16(max(acc + bias, 0)); set to whether the plan's kernels do that in their
// epilogue (those of gemm_pipe / gemm_pp) or the caller has to (the tiles of this file).
int gemm_policy(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* bias, const float* resid, int M, int N, int K,
                int out_mode, void* workspace, int64_t workspace_bytes, void* stream, bool* relu_fused = nullptr) {
  int rc = check_operands(A, lda, B, ldb, C, resid, out_mode, workspace);
  if (rc) return rc;
  const size_t ws_bytes = workspace ? (size_t)workspace_bytes : 0;
  tasu_gemm::Plan p;
  rc = tasu_gemm::plan_nt(M, N, K, out_mode, ws_bytes, tasu_pp::cu_count(), tasu_gemm::lab_switches(), &p);
  if (rc) return rc;
  tasu_gemm::Args a = tasu_gemm::make_args(A, lda, B, ldb, C, ldc, bias, resid, M, N, K);
  if (relu_fused) a.relu = *relu_fused = p.kind != TASU_GEMM_PLAN_TILES && p.kind != TASU_GEMM_PLAN_TILE192_SPLITK;
  return run_nt(p, a, out_mode, workspace, ws_bytes, (hipStream_t)stream);
}

}  // namespace

namespace tasu_gemm {
long long& gemm_launches() {
  static long long n = 0;
  return n;
}
}  // namespace tasu_gemm

extern "C" int64_t tasu_gemm_launch_count(void) { return (int64_t)tasu_gemm::gemm_launches(); }

extern "C" int tasu_relu_fwd(const void* x, void* y, int64_t n, void* stream);
// C = bf16(relu(bf16(A . B^T + bias))): PositionwiseFeedForward's w_1 + ReLU (SenseVoice.py:71-73) in one launch -- the ReLU in
// the GEMM kernels' epilogue (max before the one bf16 rounding: the same bits as rounding first); shapes the small-tile kernels
// of gemm.hip serve (at most 128 rows) run the GEMM and tasu_relu_fwd in place.
extern "C" int tasu_gemm_bias_relu_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* bias, int M, int N,
                                        int K, void* workspace, int64_t workspace_bytes, void* stream) {
  bool fused = false;
  const int rc = gemm_policy(A, lda, B, ldb, C, ldc, bias, nullptr, M, N, K, TASU_GEMM_OUT_BF16, workspace, workspace_bytes, stream, &fused);
  if (rc || fused) return rc;
  if (ldc != N) return TASU_ERR_ARG;                       // (the in-place ReLU walks a dense matrix)
  return tasu_relu_fwd(C, C, (int64_t)M * N, stream);
}

extern "C" int tasu_gemm_nt_bf16_ws(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* bias,
                                    const float* resid, int M, int N, int K, int out_mode, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  if (out_mode != TASU_GEMM_OUT_BF16 && out_mode != TASU_GEMM_OUT_F32 && out_mode != TASU_GEMM_OUT_F32_RESID_BF16R) return TASU_ERR_ARG;
  return gemm_policy(A, lda, B, ldb, C, ldc, bias, resid, M, N, K, out_mode, workspace, workspace_bytes, stream);
}

// The dispatcher's decision for a problem, without launching anything (no GPU needed; include/tasu_hip.h)
extern "C" int tasu_gemm_plan(int M, int N, int K, int out_mode, int with_workspace) {
  if (out_mode != TASU_GEMM_OUT_BF16 && out_mode != TASU_GEMM_OUT_F32 && out_mode != TASU_GEMM_OUT_F32_RESID_BF16R) return -1;
  tasu_gemm::Plan p;
  const int rc = tasu_gemm::plan_nt(M, N, K, out_mode, with_workspace ? ((size_t)64 << 20) + 16384 : 0, tasu_pp::cu_count(),
                                    tasu_gemm::lab_switches(), &p);
  return rc == TASU_OK ? p.kind : -1;
}

extern "C" int tasu_swiglu_bwd(const void* dact, const void* gu, void* dgu, int M, int I, void* stream);

// Down projection's input gradient with the SwiGLU backward in the GEMM's epilogue (include/tasu_hip.h)
extern "C" int tasu_gemm_dswiglu(const void* dy, int lddy, const void* WdT, int ldw, const void* gu, void* dgu, void* dact_ws, int M,
                                 int I, int K, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!dy || !WdT || !gu || !dgu || M <= 0 || I <= 0 || I % 8 || K <= 0 || K % BK || lddy % 8 || ldw % 8) return TASU_ERR_ARG;
  if (((uintptr_t)dy & 15) || ((uintptr_t)WdT & 15) || ((uintptr_t)gu & 15) || ((uintptr_t)dgu & 15)) return TASU_ERR_ARG;
  // The form with the SwiGLU backward in the GEMM's epilogue (dact never reaches memory) exists in the LAB build only
  // (TASU_GEMM_DSWIGLU=1 there): measured in the step it was worth 0.09 ms of 29 -- the epilogue's gate|up reads and dgu writes
  // (294 MB per call) run while the CU's MFMA pipes idle, with every CU in its epilogue at the same time, so the GEMM grows by
  // what the separate kernel took (55 us at 6.6 TB/s).  It pays once an epilogue runs under the next tile's K loop.
#ifdef TASU_LAB
  const char* const fused_env = tasu_lab_env("TASU_GEMM_DSWIGLU");   // (read per call: A/B runs in one process)
  if (fused_env && fused_env[0] == '1') {
    const int rc = gemm_policy(dy, lddy, WdT, ldw, dgu, 2 * I, nullptr, (const float*)gu, M, I, K, tasu_gemm::OUT_DSWIGLU, workspace,
                               workspace_bytes, stream);
    if (rc != tasu_gemm::kUnsupported) return rc;
  }
#endif
  if (!dact_ws || ((uintptr_t)dact_ws & 15)) return TASU_ERR_ARG;
  const int rc = gemm_policy(dy, lddy, WdT, ldw, dact_ws, I, nullptr, nullptr, M, I, K, TASU_GEMM_OUT_BF16, workspace, workspace_bytes,
                             stream);
  return rc ? rc : tasu_swiglu_bwd(dact_ws, gu, dgu, M, I, stream);
}

extern "C" int tasu_gemm_nt_bf16(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* bias,
                                 const float* resid, int M, int N, int K, int out_mode, void* stream) {
  return tasu_gemm_nt_bf16_ws(A, lda, B, ldb, C, ldc, bias, resid, M, N, K, out_mode, nullptr, 0, stream);
}
