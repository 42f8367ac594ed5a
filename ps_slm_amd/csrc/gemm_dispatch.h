// Host side of the bf16 NT GEMM dispatchers (gemm.hip, gemm_pipe.hip, gemm_pp.hip): WHAT runs is decided here, by pure
// functions of the problem's shape -- plan_nt for tasu_gemm_nt_bf16_ws and its relatives, plan_gate_up for
// tasu_gemm_gate_up_swiglu_ws -- and the entry points launch exactly the Plan they were handed (run_nt in gemm.hip, the gate|up
// entry point in gemm_pipe.hip).  tasu_gemm_plan / tasu_gemm_gate_up_plan return the same Plan's kind without a GPU.
// The planners take no operand pointers, call no HIP function (the CU count is an argument; tasu_pp::cu_count() is the one
// place that asks the runtime), touch no static state and do not allocate.
// The two cost models are NOT one model in two spellings: plan_nt counts tile area per round, plan_gate_up counts rounds of
// 256 x 256 tiles; they round differently, so merging them moves plan boundaries and needs measurements.
#pragma once
#include <stdlib.h>

#include "gemm_epilogue.h"

namespace tasu_gemm {

constexpr int kUnsupported = -1000;    // plan_nt: OUT_DSWIGLU on a shape the gemm_pipe / gemm_pp kernels do not serve

// The tuning switches of the two policies (lab build only: tasu_lab_env returns NULL in the shipped library, which therefore
// always holds the defaults below), read once per process.  TASU_GEMM_DSWIGLU and TASU_GEMM_QKV_ROPE are not here: they are read
// per call so that A/B runs can switch them inside one process.
struct LabSwitches {
  bool pp_on = true;        // TASU_GEMM_PP=0: never the 256 x 256 kernel
  bool nsplit_on = true;    // TASU_GEMM_NSPLIT=0: no column split (whole rounds of big tiles + the rest on small ones)
  int bn = 0;               // TASU_GEMM_BN: forced tile width (96, 128, 192, 256)
  int kernel = 0;           // TASU_GEMM_KERNEL: 0 = heuristic, 1 (v...) = always the tiles of gemm.hip, 2 (p...) = always gemm_pipe.hip
  int ksplit = 0;           // TASU_GEMM_KSPLIT: forced split of the 256 x 192 tiles
  double pp_eff = 1.26;     // TASU_GEMM_PP_EFF: per-FLOP efficiency of the 256 x 256 tile against 256 x 128 (tuning runs)
  int sched = 0;            // TASU_GEMM_SCHED: 1 = the pinned issue order for the 128-row tiles of gemm.hip
  // Library default of sk_plan's max_rem.  Measured (profiles/r03_gemm_streamk.txt): the round trip of the partial tiles costs
  // ~35 us per launch; it pays for fewer tiles than CUs behind a long K (d_gate_up: 96 tiles, K = 17920: 203 -> 181 us), not for
  // shapes that only lose a fraction of their last round (d_down 2.19 rounds, gate|up 4.4, lm_head 18.6: slower by 5-25 us) --
  // so those keep whole tiles unless TASU_GEMM_SK_MAXREM says otherwise.  TASU_GEMM_SK=0 (-> -1) disables the schedule altogether.
  double sk_max_rem = 0.0;
  int gu_kernel = 0;        // TASU_GEMM_GU_KERNEL: 1 (pipe) / 2 (pp) = that gate|up kernel whatever the policy says
};

inline const LabSwitches& lab_switches() {
  static const LabSwitches s = [] {
    LabSwitches l;
    const char* e;
    if ((e = tasu_lab_env("TASU_GEMM_PP"))) l.pp_on = e[0] != '0';
    if ((e = tasu_lab_env("TASU_GEMM_NSPLIT"))) l.nsplit_on = e[0] != '0';
    if ((e = tasu_lab_env("TASU_GEMM_BN"))) l.bn = atoi(e);
    if ((e = tasu_lab_env("TASU_GEMM_KERNEL"))) l.kernel = e[0] == 'p' ? 2 : (e[0] == 'v' ? 1 : 0);
    if ((e = tasu_lab_env("TASU_GEMM_KSPLIT"))) l.ksplit = atoi(e);
    if ((e = tasu_lab_env("TASU_GEMM_PP_EFF"))) l.pp_eff = atof(e);
    if ((e = tasu_lab_env("TASU_GEMM_SCHED"))) l.sched = atoi(e);
    if ((e = tasu_lab_env("TASU_GEMM_SK_MAXREM"))) l.sk_max_rem = atof(e);
    if ((e = tasu_lab_env("TASU_GEMM_SK")) && e[0] == '0') l.sk_max_rem = -1.0;
    if ((e = tasu_lab_env("TASU_GEMM_GU_KERNEL"))) l.gu_kernel = e[0] == 'p' && e[1] == 'p' ? 2 : 1;
    return l;
  }();
  return s;
}

// What one call launches.  kind is a TASU_GEMM_PLAN_* (plan_nt) or a TASU_GEMM_GU_PLAN_* (plan_gate_up) of include/tasu_hip.h.
struct Plan {
  int kind = 0;
  int bn = 0;              // tile width: the gemm_pipe launch's (PIPE*, and the tail launch of PP256_PLUS_PIPE*), or gemm.hip's (TILE*)
  int ksplit = 1;          // TILE192_SPLITK: blocks per 256 x 192 tile
  int n_main = 0;          // column split: the 256 x 256 launch covers output (gate|up: act) columns [0, n_main), 0 = all of them
  int n_tail = 0;          // ... and the second launch the remaining n_tail columns
  bool streamk = false;    // the 256 x 256 launch gets the workspace and cuts its trailing tiles along K
  double sk_rem = -2.0;    // ... with this max_rem of sk_plan (-2 = the library default, LabSwitches::sk_max_rem)
};

inline bool sk_workspace_fits(size_t ws_bytes, int cus) {
  return ws_bytes >= TASU_GEMM_WS_COUNTERS * sizeof(int) + (size_t)cus * 262144;
}

// Tile choice of gemm.hip's own kernels: both 128-row configurations run 2 blocks per CU (512 slots on 256 CUs).  When the grid
// is at most two waves of blocks, the tail efficiency tiles / (waves * 512) decides (N = 1536 at M = 4096: 384 tiles of 128x128
// fill 75 % of the slots, 512 tiles of 128x96 fill all of them: measured +11...+17 %); larger grids keep the wider tile, whose
// MFMA per LDS read ratio is better (measured: N = 8960 loses 10 % with the narrow tile).
inline int pick_bn(int M, int N, const LabSwitches& lab) {
  if (lab.bn == 96 || lab.bn == 128 || lab.bn == 192 || lab.bn == 256) return lab.bn;
  // 256 x 256 (one block per CU): worth it when the grid is many rounds of 256 blocks, or (almost) exactly one round
  // (measured on MI355X, M = 4096 / 8192: gate_up +15 %, lm_head +8 %, M = 8192 x N = 1536..2048 +10...18 %;
  //  560- and 784-tile grids lose 2...3 % against the 128-wide tiles and stay there).
  const long t256 = (long)((M + 255) / 256) * ((N + 255) / 256);
  if (t256 >= 1024 || (t256 >= 192 && t256 <= 256)) return 256;
  const long slots = 512;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128), t96 = (long)((M + 127) / 128) * ((N + 95) / 96);
  const long w128 = (t128 + slots - 1) / slots, w96 = (t96 + slots - 1) / slots;
  if (w128 > 2) return 128;
  const double e128 = (double)t128 / (double)(w128 * slots), e96 = (double)t96 / (double)(w96 * slots) / 1.08;
  return e96 > e128 ? 96 : 128;
}

// Split-K plan for the 256 x 192 tile: ksplit blocks per tile so that tiles * ksplit is (close to) one round of 256
// blocks, every split keeping >= 16 K-steps.  Returns 1 when the workspace is missing or too small.
inline int plan_ksplit(int M, int N, int K, size_t ws_bytes, const LabSwitches& lab) {
  const long tiles = (long)((M + 255) / 256) * ((N + 191) / 192);
  int ks = lab.ksplit > 0 ? lab.ksplit : (int)(256 / tiles);
  const int nk = K / 64;
  if (ks > nk / 16) ks = nk / 16;
  if (ks > 8) ks = 8;
  if (ks < 1) ks = 1;
  if (tiles > TASU_GEMM_WS_COUNTERS) return 1;
  while (ks > 1 && TASU_GEMM_WS_COUNTERS * sizeof(int) + (size_t)tiles * ks * 256 * 192 * 4 > ws_bytes) --ks;
  return ks;
}

// The plan of C[M, N] = A[M, K] . B[N, K]^T for out_mode (a TASU_GEMM_OUT_*, or OUT_DSWIGLU: served by the gemm_pipe / gemm_pp
// kernels only, kUnsupported otherwise), a workspace of ws_bytes (0 = none) and cus compute units.  TASU_OK and *plan, or an error.
// ---- kernel / tile policy (MI355X, cold weight operands as inside the training step; tools/bench_gemm.py --cold):
//  * the pipelined kernel with loader waves (gemm_pipe.hip; tiles 256 x 128, 128 x 192, 256 x 96) is the fastest on
//    every decoder, lm_head and projector shape (qkv 700 -> 822, gate_up 780 -> 837, d_down 690 -> 772, d_lm_head
//    975 -> 1149 TFLOP/s ...); the tile is the one that fills whole rounds of 256 one-per-CU blocks at the least cost;
//  * grids that cover less than half of the CUs behind K >= 16384 and too few K-tile pairs per CU for the stream-K schedule
//    (below) split K over the 256 x 192 tiles of gemm.hip instead (256 / 512 x 1536 x 17920: 130 / 150 us against 190 on
//    the loader-wave tiles; at K = 8960 the loader-wave tiles win: 1024 rows 94 against 162 us);
//  * problems of at most 64 rows keep the 128-row tiles of gemm.hip (128 x 1536 x 8960: 73 us on 256 x 96 tiles, 122 there).
inline int plan_nt(int M, int N, int K, int out_mode, size_t ws_bytes, int cus, const LabSwitches& lab, Plan* plan) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64 != 0) return TASU_ERR_ARG;
  const bool dsw = out_mode == OUT_DSWIGLU;
  Plan p;
  int use_pipe_bn = 0;
  if (lab.kernel == 2) {
    use_pipe_bn = (lab.bn == 96 || lab.bn == 128 || lab.bn == 192) ? lab.bn : -1;
  } else if (lab.kernel == 0 && lab.bn == 0 && M > 64) {
    use_pipe_bn = -1;
  }
  if (use_pipe_bn != 0) {
    const long tm = (M + 255) / 256;
    const long t128 = tm * ((N + 127) / 128), t96 = tm * ((N + 95) / 96);
    const long t256 = tm * ((N + 255) / 256);
    const bool pp_ok = lab.pp_on && lab.kernel == 0 && K >= 256 && K % 128 == 0;
    const bool sk = pp_ok && sk_plan(t256, K / 128, cus, sk_workspace_fits(ws_bytes, cus), lab.sk_max_rem) > 0;
    if (!dsw && !sk && lab.kernel == 0 && M > 128 && t96 < 128 && K >= 16384 && plan_ksplit(M, N, K, ws_bytes, lab) > 1) {
      use_pipe_bn = 0;                              // falls through to the split-K tile below
    } else {
      if (use_pipe_bn < 0) {
        // time ~ rounds of one-block-per-CU grids x tile area / per-FLOP efficiency of the tile (8192^3, cold: 256 x 128
        // 1300, 128 x 192 1123, 256 x 96 ~1040 TFLOP/s).  N = 1536 at M = 4096 -> 256 tiles of 128 x 192 (+7 % over
        // 256 x 96: fewer staged bytes and fragment reads per FLOP); wide grids -> 256 x 128.
        auto cost = [](long tiles, double area, double eff) { return (double)((tiles + 255) / 256) * area / eff; };
        const long t192 = (long)((M + 127) / 128) * ((N + 191) / 192);
        const double c128 = cost(t128, 256.0 * 128, 1.00), c192 = cost(t192, 128.0 * 192, 0.86), c96 = cost(t96, 256.0 * 96, 0.80);
        use_pipe_bn = c128 <= c192 && c128 <= c96 ? 128 : (c192 <= c96 ? 192 : 96);
        // the 256 x 256 eight-wave kernel (gemm_pp.hip): 2/3 of the L2 -> LDS bytes per FLOP of the 256 x 128 tile.  Measured on
        // whole rounds at K = 1536 (4096 x 16384: 1232 vs 995 TFLOP/s) its per-FLOP efficiency is 1.24 x that tile's, so it wins
        // wherever its coarser rounds do not eat that up (gate|up, lm_head; d_down's 3 rounds against 5: a tie on paper, +0.5 %
        // on the step measured with TASU_GEMM_PP_EFF = 1.26 against 1.19 on one box; not the one-round N = 1536 grids)
        if (pp_ok) {
          // stream-K (gemm_pp.hip; needs the workspace): the 256 x 256 tiles fill FRACTIONAL rounds -- every workgroup gets the
          // same number of K-tile pairs -- for the price of the partial tiles' round trip (~35 us per launch whatever K is:
          // 1e8 / K in the units of this model).  That serves d_gate_up (96 tiles on 256 CUs, K = 17920: 203 -> 181 us); at
          // K = 8960 (down) the 128 x 192 one-round grid still wins (100 vs 108 us).
          const double c256_whole = cost(t256, 256.0 * 256, lab.pp_eff);
          const double c256_sk = sk ? (double)t256 / cus * 256.0 * 256 / lab.pp_eff + 1.0e8 / K : 1e30;
          const double c256 = c256_sk < c256_whole ? c256_sk : c256_whole;
          const double best = use_pipe_bn == 128 ? c128 : (use_pipe_bn == 192 ? c192 : c96);
          if (c256 < best) {
            p.kind = TASU_GEMM_PLAN_PP256;
            if (c256_sk < c256_whole) {
              p.kind = TASU_GEMM_PLAN_PP256_STREAMK;
              p.streamk = true;
              return *plan = p, TASU_OK;
            }
            // a mostly empty last round of big tiles (d_down: 560 tiles = 2.19 rounds): whole rounds on the big tiles, the
            // remaining columns on the small tiles in a second launch (TASU_GEMM_NSPLIT=0 disables)
            const long tn = (N + 255) / 256, full = (tm * tn) / 256, tn_main = full * 256 / tm;
            if (lab.nsplit_on && full >= 1 && tn_main > 0 && tn_main < tn) {
              const int n_main = (int)tn_main * 256, n_tail = N - n_main;
              const long u128 = tm * ((n_tail + 127) / 128), u192 = (long)((M + 127) / 128) * ((n_tail + 191) / 192);
              const double tail128 = cost(u128, 256.0 * 128, 1.00), tail192 = cost(u192, 128.0 * 192, 0.86);
              const double c_split = (double)full * 256.0 * 256 / lab.pp_eff + (tail128 < tail192 ? tail128 : tail192) + 0.05 * 256.0 * 256;
              if (c_split < c256) {
                p.kind = tail128 < tail192 ? TASU_GEMM_PLAN_PP256_PLUS_PIPE128 : TASU_GEMM_PLAN_PP256_PLUS_PIPE192;
                p.bn = tail128 < tail192 ? 128 : 192;
                p.n_main = n_main;
                p.n_tail = n_tail;
              }
            }
            return *plan = p, TASU_OK;
          }
        }
      }
      p.kind = use_pipe_bn == 128 ? TASU_GEMM_PLAN_PIPE128 : (use_pipe_bn == 192 ? TASU_GEMM_PLAN_PIPE192 : TASU_GEMM_PLAN_PIPE96);
      p.bn = use_pipe_bn;
      return *plan = p, TASU_OK;
    }
  }
  if (dsw) return kUnsupported;
  // the deep small-grid case above, or the 128-row tiles
  p.bn = lab.kernel == 0 && lab.bn == 0 && M > 128 ? 192 : pick_bn(M, N, lab);
  if (p.bn == 192) p.ksplit = plan_ksplit(M, N, K, ws_bytes, lab);
  p.kind = p.ksplit > 1 ? TASU_GEMM_PLAN_TILE192_SPLITK : TASU_GEMM_PLAN_TILES;
  return *plan = p, TASU_OK;
}

// The plan of tasu_gemm_gate_up_swiglu_ws (gu[M, 2I], act[M, I]; kind = a TASU_GEMM_GU_PLAN_*).  In units of one round of
// 256 x 256 tiles (128 act columns) on every CU: 256 x 256 tiles (gemm_pp.hip) where their coarser rounds cost less than the
// per-FLOP efficiency they bring (4096 x 17920 x 1536: 257 -> 218 us); and when the last round of big tiles would be mostly
// empty (1120 tiles on 256 CUs: 4.375 rounds), whole rounds on the big tiles + the remaining columns on the 256 x 128 tiles
// (64 act columns, gemm_pipe.hip) in a second launch (4 rounds + 192 tiles of 256 x 128).
inline int plan_gate_up(int M, int I, int K, size_t ws_bytes, int cu_count, const LabSwitches& lab, Plan* plan) {
  if (M <= 0 || I <= 0 || I % 4 || K <= 0 || K % 64) return TASU_ERR_ARG;
  Plan p;
  p.kind = TASU_GEMM_GU_PLAN_PIPE;
  const bool pp_ok = I % 128 == 0 && K >= 256 && K % 128 == 0;
  if (!pp_ok || lab.gu_kernel == 1) return *plan = p, TASU_OK;
  const long tm = (M + 255) / 256, cus = cu_count, tn = (I + 127) / 128;
  // stream-K (workspace given): the big tiles fill fractional rounds, for the price of the partial tiles' round trip (~35 us)
  const bool sk = sk_plan(tm * tn, K / 128, (int)cus, sk_workspace_fits(ws_bytes, (int)cus), lab.sk_max_rem) > 0;
  if (lab.gu_kernel == 2) {                       // (the launch cuts tiles wherever sk_plan says so)
    p.kind = sk ? TASU_GEMM_GU_PLAN_PP_STREAMK : TASU_GEMM_GU_PLAN_PP;
    p.streamk = sk;
    return *plan = p, TASU_OK;
  }
  auto rounds = [&](long tiles) { return (double)((tiles + cus - 1) / cus); };
  const double c128 = rounds(tm * ((I + 63) / 64)) * 0.5;
  const double c256_whole = rounds(tm * tn) / 1.26;
  const double c256_sk = sk ? ((double)(tm * tn) / cus) / 1.26 + 1.0e8 / K / 52012.0 : 1e30;
  const double c256 = c256_sk < c256_whole ? c256_sk : c256_whole;
  if (lab.pp_on && c256 < c128) {
    p.kind = TASU_GEMM_GU_PLAN_PP;
    if (c256_sk < c256_whole) {
      p.kind = TASU_GEMM_GU_PLAN_PP_STREAMK;
      p.streamk = true;
      return *plan = p, TASU_OK;
    }
    const long full = (tm * tn) / cus;                          // whole rounds of big tiles
    const long tn_main = full * cus / tm;                       // column tiles they cover
    if (lab.nsplit_on && full >= 1 && tn_main < tn && tn_main > 0) {
      const double c_split = (double)full / 1.26 + rounds(tm * (tn - tn_main) * 2) * 0.5 + 0.05;   // + the second launch's ramp
      if (c_split < c256) {
        p.kind = TASU_GEMM_GU_PLAN_PP_PLUS_PIPE;
        p.bn = 128;
        p.n_main = (int)tn_main * 128;
        p.n_tail = I - p.n_main;
      }
    }
  }
  return *plan = p, TASU_OK;
}

// Args of a plain problem: whole K in one work item, every column, no epilogue option.  Callers set only what differs
// (act, act_ld, relu, ksplit, split_stride, n0, n1, R).
inline Args make_args(const void* A, int lda, const void* B, int ldb, void* C, int ldc, const void* bias, const float* resid, int M,
                      int N, int K) {
  Args a;
  a.A = (const bf16*)A;
  a.B = (const bf16*)B;
  a.C = C;
  a.R = resid;
  a.bias = (const bf16*)bias;
  a.M = M;
  a.N = N;
  a.K = K;
  a.lda = lda;
  a.ldb = ldb;
  a.ldc = ldc;
  a.tiles_m = a.tiles_n = 0;
  a.act = nullptr;
  a.ksplit = 1;
  a.split_stride = 0;
  return a;
}

}  // namespace tasu_gemm

// ---- the launches behind a Plan, one per kernel family.  `a` comes from make_args; its n0 / n1 name the launch's columns, its
// relu (TASU_GEMM_OUT_BF16 only) and act / act_ld (gate|up) the epilogue options.  out_mode OUT_DSWIGLU (lab build): a.R is the
// saved gate|up matrix (bf16 [M, 2N]), C = dgu [M, 2N].
// gemm_pipe.hip: bn = 128 / 96 / 192 -> 256 x 128, 256 x 96 or 128 x 192 tiles
int tasu_gemm_pipe_dispatch(tasu_gemm::Args a, int out_mode, int bn, hipStream_t st);
// gemm_pp.hip, 256 x 256 tiles; ws (that of tasu_gemm_nt_bf16_ws) or nullptr: with it the launch cuts its trailing tiles along K
// wherever sk_plan(max_rem = sk_rem; -2 = the library default) says so
int tasu_gemm_pp_dispatch(tasu_gemm::Args a, int out_mode, hipStream_t st, void* ws, size_t ws_bytes, double sk_rem);
// ... gate|up + SwiGLU (a.N = I, a.C = gu [M, 2I], a.act / a.act_ld); I % 128 == 0, K % 128 == 0, K >= 256
int tasu_gemm_pp_gu_dispatch(tasu_gemm::Args a, hipStream_t st, void* ws, size_t ws_bytes);
namespace tasu_pp {
int cu_count();          // compute units of the current device rounded down to a multiple of 8 (256 without a device)
}
