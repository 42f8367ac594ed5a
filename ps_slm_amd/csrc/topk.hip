// Per-row log-softmax + top-k of the decode loop: tasu_logprob_topk / tasu_f32_logprob_topk and their forms under
// generate(repetition_penalty = p), tasu_logprob_topk_hist / tasu_f32_logprob_topk_hist.  Per row: lse over V columns, then the k
// best log-probs with their column ids in the order (value descending, column ascending); columns listed in `banned` (e.g. EOS
// while cur_len < min_length) never qualify; fewer than k selectable columns: the rest is (-inf, 0x7fffffff).  k <= 32.
//
// Two launches.  Stage 1, grid (M, 16): a column part's max, sum of exp and k best.  topk_part_kernel is one template for fp32
// logits and for both dtypes with history; bf16 logits without history keep topk_part_bf16_kernel<K>, the same threshold form with k
// at compile time and per-thread lists (topk_part_lists<K>) for massive ties and for parts longer than the register window, which is
// faster at k = 16 and 32.  Stage 2, one workgroup per row, merges the 16 parts; the three merge kernels are different algorithms
// (register lists, one candidate per thread, an LDS pool with the history tokens) that share the row's log-sum-exp and the ranking
// helpers below.  f32_logprob_topk_kernel serves fp32 rows without workspace / alignment or alone (M = 1).
//
// The HF RepetitionPenaltyLogitsProcessor rule  score' = score < 0 ? score * p : score / p  applies once to every distinct token of
// the row's history (kept next to the beam state by tasu_beam_hist_update, csrc/beam.hip):
//   mode 1 (greedy, num_beams = 1): HF hands the processor the RAW logits -- the part scan penalises the history columns before
//           max / sum-exp / selection; everything after it is the unpenalised form's.
//   mode 0 (beam search): HF hands it the log-softmax output and does not renormalise.  The order of a history column against the
//           others depends on the row's log-sum-exp, which a column part does not know: the part scan keeps history columns out of its
//           candidates (they count in max / sum-exp unmodified) and the merge launch adds the row's history tokens as candidates
//           with p * (x - lse).
// Membership of a column in the history is one bit of a per-workgroup LDS bitmask over the part's column range (set from the history
// with atomicOr, at most 2048 entries): thread t's chunk of VEC consecutive columns owns VEC consecutive bits, so a wave's 64 chunk
// reads touch 8 or 16 CONSECUTIVE 32-bit words (distinct banks; the lanes that share a word read the same address, which LDS
// broadcasts) -- one conflict-free LDS read per VEC columns.
#include "common.h"
#include "../../include/tasu_hip.h"

namespace {
constexpr int TOPK_MAX = 32;
constexpr int TOPK_PARTS = 16;        // column parts per row: 64 rows x 16 parts = 1024 blocks for the 152k-column vocabulary
constexpr int TOPK_MAXC_BF16 = 6, TOPK_MAXC_F32 = 10;   // 16-byte chunks a thread of the part scan holds in registers (bf16 x 8, fp32 x 4)
constexpr int TOPK_PCAND = 64;        // candidates a part ranks in one wave (k <= 16; k <= 32: twice as many, ranked through LDS)
constexpr int TOPK_HIST_MAX = 2048;   // history entries per row (the decode context limit)
constexpr int TOPK_NONE = 0x7fffffff;

__device__ __forceinline__ float rep_penalty(float s, float p) { return s < 0.f ? s * p : s / p; }

// ------------------------------------------------------------------------------------------------- shared pieces
// the selection order, everywhere: candidate (dv, di) comes before (v, id)
__device__ __forceinline__ bool before(float dv, int di, float v, int id) { return dv > v || (dv == v && di < id); }

// rank of (v, id) = the number of candidates before it; the candidates are lanes 0 .. n-1 of the wave, or n LDS entries
__device__ __forceinline__ int rank_in_wave(float v, int id, int n) {
  int rank = 0;
  for (int d = 0; d < n; ++d) {
    const float dv = __shfl(v, d, 64);
    const int di = __shfl(id, d, 64);
    rank += before(dv, di, v, id) ? 1 : 0;
  }
  return rank;
}
__device__ __forceinline__ int rank_in_lds(const float* cv, const int* ci, int n, float v, int id) {
  int rank = 0;
  for (int d = 0; d < n; ++d) rank += before(cv[d], ci[d], v, id) ? 1 : 0;
  return rank;
}
// the first of the wave's / the workgroup's (v, id) in the selection order, in every thread (block form: bv / bi hold NW entries)
__device__ __forceinline__ void wave_best(float& v, int& id) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(id, o, 64);
    if (before(ov, oi, v, id)) v = ov, id = oi;
  }
}
template <int NW>
__device__ __forceinline__ void block_best(float& v, int& id, float* bv, int* bi) {
  wave_best(v, id);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) bv[threadIdx.x >> 6] = v, bi[threadIdx.x >> 6] = id;
  __syncthreads();
  v = bv[0], id = bi[0];
#pragma unroll
  for (int w = 1; w < NW; ++w)
    if (before(bv[w], bi[w], v, id)) v = bv[w], id = bi[w];
}

// The row's log-sum-exp = mx + lg from the parts' (max, sum exp(x - max)), computed by one whole wave, and a column's log-prob:
// FAST (bf16 logits) __expf / __logf and x - lse; otherwise expf / logf and (x - max) - log(sum), torch.log_softmax's form.
template <bool FAST>
struct RowLse {
  float mx, lg;
  __device__ __forceinline__ float logprob(float v) const { return FAST ? v - (mx + lg) : (v - mx) - lg; }
};
template <bool FAST>
__device__ __forceinline__ RowLse<FAST> row_lse(const float* __restrict__ pm, const float* __restrict__ ps, int row, int lane) {
  const bool lp = lane < TOPK_PARTS;
  const float mp = lp ? pm[(size_t)row * TOPK_PARTS + lane] : -__builtin_inff();
  const float sp = lp ? ps[(size_t)row * TOPK_PARTS + lane] : 0.f;
  const float mx = wave_max(mp);
  const float sm = wave_sum(lp && mp > -__builtin_inff() ? sp * (FAST ? __expf(mp - mx) : expf(mp - mx)) : 0.f);
  return {mx, FAST ? __logf(sm) : logf(sm)};
}

template <typename T, int VEC>
struct TopkVec;
template <>
struct TopkVec<bf16, 8> {
  typedef bf16x8 type;
};
template <>
struct TopkVec<float, 4> {
  typedef f32x4 type;
};

// ------------------------------------------------------------------------------------------------- stage 1
// Grid (M, 16), 256 threads: the part's columns live in registers (one read, all loads in flight together).  pm / ps = max and sum
// exp(x - max) over its columns, pv / pi = its k best selectable columns (value descending, column ascending).
// Threshold form (per-thread insertion lists are instruction-bound: in a wave some lane inserts at almost every element):
//   tau = the largest, over the four waves, of the wave's k-th largest per-thread selectable maximum: at least k columns are >= tau,
//   so the part's k best all are; the sum-of-exp pass collects the columns >= tau (a handful) in LDS and they are ranked, by one
//   wave's shuffles or (PCAND > 64: the per-thread maxima alone can put 4 k - 3 columns at or above tau) by as many threads reading
//   LDS.  More than PCAND such columns (massive ties): k rounds of block argmax over the registers.
// HIST: the history of the row (mode 1: its columns penalised first; mode 0: its columns are not selectable here).  Without it the
// instantiation carries no bitmask, no history loads and no penalty code.
template <typename T, int VEC, int MAXC, bool FAST, int PCAND, bool HIST>
__global__ __launch_bounds__(256) void topk_part_kernel(const T* __restrict__ logits, int ld, int V, int k,
                                                        const int32_t* __restrict__ banned, int n_banned,
                                                        const int32_t* __restrict__ hist, int hist_ld,
                                                        const int32_t* __restrict__ hist_len, float p, int mode,
                                                        float* __restrict__ pm, float* __restrict__ ps, float* __restrict__ pv,
                                                        int32_t* __restrict__ pi) {
  typedef typename TopkVec<T, VEC>::type VT;
  __shared__ float red[4];
  __shared__ float wtau[4];
  __shared__ float bv[4];
  __shared__ int bi[4];
  __shared__ float cand_v[PCAND];
  __shared__ int cand_i[PCAND];
  __shared__ int cand_n;
  const int row = blockIdx.x, part = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const T* x = logits + (size_t)row * ld;
  const int nv = (V + VEC - 1) / VEC, per = (nv + TOPK_PARTS - 1) / TOPK_PARTS;    // (per <= 256 * MAXC: checked by the host entry)
  const int v0 = part * per, v1 = min(nv, v0 + per);
  if (t == 0) cand_n = 0;                                  // (published by the barriers of block_max)
  VT xs[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv = v0 + t + i * 256;
    if (cv < v1) xs[i] = *(const VT*)(x + (size_t)cv * VEC);
  }
  unsigned hm[MAXC];                                       // the history bits of this thread's chunks
#pragma unroll
  for (int i = 0; i < MAXC; ++i) hm[i] = 0u;
  if constexpr (HIST) {
    constexpr int NWORD = 256 * MAXC * VEC / 32;
    __shared__ unsigned hbits[NWORD];
    const int c0 = v0 * VEC, ncol = max(v1 - v0, 0) * VEC;
    for (int i = t; i < NWORD; i += 256) hbits[i] = 0u;
    __syncthreads();
    const int hl = min(max(hist_len[row], 0), min(hist_ld, TOPK_HIST_MAX));
    const int32_t* hr = hist + (size_t)row * hist_ld;
    for (int i = t; i < hl; i += 256) {
      const int c = hr[i], r = c - c0;
      if (r >= 0 && r < ncol && c < V) atomicOr(&hbits[r >> 5], 1u << (r & 31));
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int q = t + i * 256;
      hm[i] = (hbits[(q * VEC) >> 5] >> ((q * VEC) & 31)) & ((1u << VEC) - 1u);
    }
  }
  const int ban0 = n_banned > 0 ? banned[0] : -1, ban1 = n_banned > 1 ? banned[1] : -1;    // the usual case: EOS below min_length
  auto is_banned = [&](int c) {
    bool ban = c == ban0 || c == ban1;
    for (int b = 2; b < n_banned; ++b) ban |= (banned[b] == c);
    return ban;
  };
  // values (mode 1: penalised) and the selectable columns of this thread's chunks; columns outside the part or >= V hold -inf
  float f[MAXC][VEC];
  unsigned selm[MAXC];
  float m = -__builtin_inff(), msel = -__builtin_inff();
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv = v0 + t + i * 256;
    selm[i] = 0u;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int c = cv * VEC + j;
      float v = -__builtin_inff();
      if (cv < v1 && c < V) {
        v = (float)xs[i][j];
        const bool in_hist = HIST && ((hm[i] >> j) & 1u);
        if (HIST && mode == 1 && in_hist) v = rep_penalty(v, p);
        if (!(mode == 0 && in_hist) && !is_banned(c)) {
          selm[i] |= 1u << j;
          msel = fmaxf(msel, v);
        }
      }
      f[i][j] = v;
      m = fmaxf(m, v);
    }
  }
  m = block_max<4>(m, red);
  // the wave's k-th largest per-thread best: k rounds of (wave max, retire one lane that holds it)
  float mine = msel, kth = -__builtin_inff();
  for (int r = 0; r < k; ++r) {
    kth = wave_max(mine);
    const unsigned long long holders = __ballot(mine == kth);
    if (lane == __ffsll((long long)holders) - 1) mine = -__builtin_inff();
  }
  if (lane == 0) wtau[wave] = kth;
  __syncthreads();
  const float tau = fmaxf(fmaxf(wtau[0], wtau[1]), fmaxf(wtau[2], wtau[3]));
  float s = 0.f;                                           // (the order of this sum is part of the output: chunk i, element j)
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float v = f[i][j];
      if (v > -__builtin_inff()) {
        s += FAST ? __expf(v - m) : expf(v - m);
        if (v >= tau && ((selm[i] >> j) & 1u)) {
          const int slot = atomicAdd(&cand_n, 1);
          if (slot < PCAND) cand_v[slot] = v, cand_i[slot] = (v0 + t + i * 256) * VEC + j;
        }
      }
    }
  s = block_sum<4>(s, red);                                // (its barriers also publish the candidates)
  const size_t slot0 = (size_t)row * TOPK_PARTS + part;
  if (t == 0) pm[slot0] = m, ps[slot0] = s;
  const int n_cand = cand_n;
  if (n_cand <= PCAND) {                                   // block-uniform
    if constexpr (PCAND > 64) {
      if (t < n_cand) {
        const float v = cand_v[t];
        const int id = cand_i[t];
        const int rank = rank_in_lds(cand_v, cand_i, n_cand, v, id);
        if (rank < k) pv[slot0 * k + rank] = v, pi[slot0 * k + rank] = id;
      }
      if (t >= n_cand && t < k) pv[slot0 * k + t] = -__builtin_inff(), pi[slot0 * k + t] = TOPK_NONE;   // fewer than k selectable columns
    } else if (wave == 0) {
      const bool live = lane < n_cand;
      const float v = live ? cand_v[lane] : -__builtin_inff();
      const int id = live ? cand_i[lane] : TOPK_NONE;
      const int rank = rank_in_wave(v, id, n_cand);
      if (live && rank < k) pv[slot0 * k + rank] = v, pi[slot0 * k + rank] = id;
      if (lane >= n_cand && lane < k) pv[slot0 * k + lane] = -__builtin_inff(), pi[slot0 * k + lane] = TOPK_NONE;
    }
    return;
  }
  // massive ties: k rounds of "the best selectable column after the previous pick" over the registers
  float pvv = __builtin_inff();
  int pii = -1;
  for (int r = 0; r < k; ++r) {
    float best = -__builtin_inff();
    int bid = TOPK_NONE;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float v = f[i][j];
        const int c = (v0 + t + i * 256) * VEC + j;
        if (!(v > -__builtin_inff()) || !((selm[i] >> j) & 1u)) continue;
        const bool after = v < pvv || (v == pvv && c > pii);
        if (!after || v < best || (v == best && c > bid)) continue;
        best = v, bid = c;
      }
    block_best<4>(best, bid, bv, bi);
    if (t == 0) pv[slot0 * k + r] = bid == TOPK_NONE ? -__builtin_inff() : best, pi[slot0 * k + r] = bid;
    pvv = best, pii = bid;
    if (bid == TOPK_NONE) pvv = -__builtin_inff(), pii = TOPK_NONE;
  }
}

// The general form of stage 1 for bf16 rows: per-thread sorted lists of K merged per wave and per block (grid and outputs as
// topk_part_kernel).  Instruction-bound: every element pays the insertion.  topk_part_bf16_kernel calls it for the whole part, the
// statistics included, when the part is longer than its register window or more columns than its cap reach its threshold.
template <int K>
__device__ void topk_part_lists(const bf16* __restrict__ logits, int ld, int V,
                                                        const int32_t* __restrict__ banned, int n_banned,
                                                        float* __restrict__ pm, float* __restrict__ ps,
                                                        float* __restrict__ pv, int32_t* __restrict__ pi) {
  __shared__ float red[4];
  __shared__ float cv[4 * K];
  __shared__ int ci[4 * K];
  const int row = blockIdx.x, part = blockIdx.y;
  const bf16* lr = logits + (size_t)row * ld;
  float tv[K];
  int ti[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    tv[j] = -__builtin_inff();
    ti[j] = TOPK_NONE;
  }
  // this part's 8-column chunks [v0, v1) (ld % 8 == 0, checked by the host entry); columns >= V are skipped
  const int nv = (V + 7) / 8;
  const int per = (nv + TOPK_PARTS - 1) / TOPK_PARTS;
  const int v0 = part * per, v1 = min(nv, v0 + per);
  // a thread's chunks are loaded ONCE, all loads in flight together (two dependent passes over global memory, five
  // sequential loads each, were most of this kernel's time); parts longer than 256 * MAXC chunks take the loop below too
  constexpr int MAXC = TOPK_MAXC_BF16;
  bf16x8 xs[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv8 = v0 + threadIdx.x + i * 256;
    xs[i] = cv8 < v1 ? *(const bf16x8*)(lr + cv8 * 8) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const int vreg = min(v1, v0 + 256 * MAXC);      // chunks [v0, vreg) live in registers
  float m = -__builtin_inff();
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv8 = v0 + threadIdx.x + i * 256;
    if (cv8 < vreg) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (cv8 * 8 + j < V) m = fmaxf(m, (float)xs[i][j]);
    }
  }
  for (int cv8 = vreg + threadIdx.x; cv8 < v1; cv8 += 256) {
    const bf16x8 x = *(const bf16x8*)(lr + cv8 * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (cv8 * 8 + j < V) m = fmaxf(m, (float)x[j]);
  }
  m = block_max<4>(m, red);
  float s = 0.f;
  const int ban0 = n_banned > 0 ? banned[0] : -1, ban1 = n_banned > 1 ? banned[1] : -1;    // the usual case: EOS below min_length
  auto visit = [&](const bf16x8& x, int cv8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = cv8 * 8 + j;
      if (c >= V) continue;
      const float f = (float)x[j];
      s += __expf(f - m);
      // thread-local sorted list (descending; on ties the smaller column, seen first, stays ahead)
      if (f > tv[K - 1]) {
        bool ban = c == ban0 || c == ban1;             // (a global load per candidate here cost ~0.5 us each, ~20 per thread)
        for (int b = 2; b < n_banned; ++b) ban |= (banned[b] == c);
        if (ban) continue;
        tv[K - 1] = f;
        ti[K - 1] = c;
#pragma unroll
        for (int jj = K - 1; jj > 0; --jj) {
          if (tv[jj] > tv[jj - 1]) {
            const float a = tv[jj];
            tv[jj] = tv[jj - 1];
            tv[jj - 1] = a;
            const int b2 = ti[jj];
            ti[jj] = ti[jj - 1];
            ti[jj - 1] = b2;
          }
        }
      }
    }
  };
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv8 = v0 + threadIdx.x + i * 256;
    if (cv8 < vreg) visit(xs[i], cv8);
  }
  for (int cv8 = vreg + threadIdx.x; cv8 < v1; cv8 += 256) visit(*(const bf16x8*)(lr + cv8 * 8), cv8);
  s = block_sum<4>(s, red);
  const size_t slot0 = (size_t)row * TOPK_PARTS + part;
  if (threadIdx.x == 0) {
    pm[slot0] = m;
    ps[slot0] = s;
  }
  // Selection without block-wide rounds (K rounds of block argmax with two barriers each were 30 of this kernel's 38 us):
  //   each WAVE merges its 64 sorted lists by K rounds of wave argmax over the list heads (shuffles only; the winner shifts
  //   its register list up), leaving the wave's K best, sorted; the four waves' 4 K candidates then meet in LDS and wave 0
  //   ranks them (rank = number of candidates ahead in the (value desc, column asc) order).
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < K; ++r) {
    float v = tv[0];
    int id = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(id, o, 64);
      if (ov > v || (ov == v && oi < id)) {
        v = ov;
        id = oi;
      }
    }
    if (id == ti[0] && v == tv[0]) {                // this lane's head won (columns are unique; exhausted lists hold TOPK_NONE)
#pragma unroll
      for (int j = 0; j + 1 < K; ++j) {
        tv[j] = tv[j + 1];
        ti[j] = ti[j + 1];
      }
      tv[K - 1] = -__builtin_inff();
      ti[K - 1] = TOPK_NONE;
    }
    if (lane == 0) {
      cv[wave * K + r] = v;
      ci[wave * K + r] = id;
    }
  }
  __syncthreads();
  if constexpr (4 * K > 64) {                              // K > 16: the 4 K candidates are ranked by 4 K threads reading LDS
    if (threadIdx.x < 4 * K) {
      const float v = cv[threadIdx.x];
      const int id = ci[threadIdx.x];
      int rank = 0;
      for (int d = 0; d < 4 * K; ++d) {
        const float dv = cv[d];
        const int di = ci[d];
        rank += (dv > v || (dv == v && (di < id || (di == id && d < (int)threadIdx.x)))) ? 1 : 0;
      }
      if (rank < K) {
        pv[slot0 * K + rank] = v;
        pi[slot0 * K + rank] = id;
      }
    }
  } else if (wave == 0) {
    static_assert(4 * K <= 64, "the four waves' candidates fit one wave");
    const bool live = lane < 4 * K;
    const float v = live ? cv[lane] : -__builtin_inff();
    const int id = live ? ci[lane] : TOPK_NONE;
    int rank = 0;
#pragma unroll
    for (int d = 0; d < 4 * K; ++d) {
      const float dv = __shfl(v, d, 64);
      const int di = __shfl(id, d, 64);
      rank += (dv > v || (dv == v && (di < id || (di == id && d < lane)))) ? 1 : 0;
    }
    if (live && rank < K) {
      pv[slot0 * K + rank] = v;
      pi[slot0 * K + rank] = id;
    }
  }
}

// Stage 1 of tasu_logprob_topk (bf16, no history): topk_part_kernel's threshold form with k at compile time, the logits kept
// packed in registers and converted in each pass, and the lists above where that kernel takes its block-argmax rounds (and for a
// part longer than the register window, V > 196,608).  It holds the time of the 8 x 8 and 4 x 16 decode shapes, which the shared
// scan misses by 38 and 72 us per launch; same outputs, bit for bit.
template <int K>
__global__ __launch_bounds__(256) void topk_part_bf16_kernel(const bf16* __restrict__ logits, int ld, int V,
                                                        const int32_t* __restrict__ banned, int n_banned,
                                                        float* __restrict__ pm, float* __restrict__ ps,
                                                        float* __restrict__ pv, int32_t* __restrict__ pi) {
  __shared__ float red[4];
  __shared__ float wtau[4];
  constexpr int CAP = K <= 16 ? TOPK_PCAND : 2 * TOPK_PCAND; // (up to 4 K - 3 per-thread maxima alone can reach tau)
  __shared__ float cand_v[CAP];
  __shared__ int cand_i[CAP];
  __shared__ int cand_n;
  const int row = blockIdx.x, part = blockIdx.y;
  const bf16* lr = logits + (size_t)row * ld;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = (V + 7) / 8;
  const int per = (nv + TOPK_PARTS - 1) / TOPK_PARTS;
  const int v0 = part * per, v1 = min(nv, v0 + per);
  constexpr int MAXC = TOPK_MAXC_BF16;
  if (v1 - v0 > 256 * MAXC) {                              // a part longer than the register window: general form
    topk_part_lists<K>(logits, ld, V, banned, n_banned, pm, ps, pv, pi);
    return;
  }
  if (threadIdx.x == 0) cand_n = 0;
  bf16x8 xs[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv8 = v0 + threadIdx.x + i * 256;
    xs[i] = cv8 < v1 ? *(const bf16x8*)(lr + cv8 * 8) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const int ban0 = n_banned > 0 ? banned[0] : -1, ban1 = n_banned > 1 ? banned[1] : -1;
  auto is_banned = [&](int c) {
    bool ban = c == ban0 || c == ban1;
    for (int b = 2; b < n_banned; ++b) ban |= (banned[b] == c);
    return ban;
  };
  // pass 1: the part's maximum (softmax statistics: all columns) and this thread's best selectable column value
  float m = -__builtin_inff(), msel = -__builtin_inff();
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv8 = v0 + threadIdx.x + i * 256;
    if (cv8 < v1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cv8 * 8 + j;
        if (c < V) {
          const float f = (float)xs[i][j];
          m = fmaxf(m, f);
          if (f > msel && !is_banned(c)) msel = f;
        }
      }
    }
  }
  m = block_max<4>(m, red);
  // the wave's K-th largest per-thread best: K rounds of (wave max, retire one lane that holds it)
  float mine = msel, kth = -__builtin_inff();
#pragma unroll
  for (int r = 0; r < K; ++r) {
    kth = wave_max(mine);
    const unsigned long long holders = __ballot(mine == kth);
    if (lane == __ffsll((long long)holders) - 1) mine = -__builtin_inff();
  }
  if (lane == 0) wtau[wave] = kth;
  __syncthreads();
  const float tau = fmaxf(fmaxf(wtau[0], wtau[1]), fmaxf(wtau[2], wtau[3]));
  // pass 2: sum of exp, and the columns >= tau
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv8 = v0 + threadIdx.x + i * 256;
    if (cv8 < v1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = cv8 * 8 + j;
        if (c < V) {
          const float f = (float)xs[i][j];
          s += __expf(f - m);
          if (f >= tau && f > -__builtin_inff() && !is_banned(c)) {
            const int slot = atomicAdd(&cand_n, 1);
            if (slot < CAP) {
              cand_v[slot] = f;
              cand_i[slot] = c;
            }
          }
        }
      }
    }
  }
  s = block_sum<4>(s, red);                              // (its barriers also publish the candidates)
  const int n_cand = cand_n;
  if (n_cand > CAP) {                                      // block-uniform
    topk_part_lists<K>(logits, ld, V, banned, n_banned, pm, ps, pv, pi);
    return;
  }
  const size_t slot0 = (size_t)row * TOPK_PARTS + part;
  if (threadIdx.x == 0) {
    pm[slot0] = m;
    ps[slot0] = s;
  }
  if constexpr (CAP > 64) {                                // K > 16: up to 128 candidates, ranked by as many threads reading LDS
    const int t = threadIdx.x;
    if (t < n_cand) {
      const float v = cand_v[t];
      const int id = cand_i[t];
      int rank = 0;
      for (int d = 0; d < n_cand; ++d) rank += (cand_v[d] > v || (cand_v[d] == v && cand_i[d] < id)) ? 1 : 0;
      if (rank < K) {
        pv[slot0 * K + rank] = v;
        pi[slot0 * K + rank] = id;
      }
    }
    if (t >= n_cand && t < K) {                            // fewer than K selectable columns in this part
      pv[slot0 * K + t] = -__builtin_inff();
      pi[slot0 * K + t] = TOPK_NONE;
    }
  } else if (wave == 0) {
    const bool live = lane < n_cand;
    const float v = live ? cand_v[lane] : -__builtin_inff();
    const int id = live ? cand_i[lane] : TOPK_NONE;
    int rank = 0;
    for (int d = 0; d < n_cand; ++d) {
      const float dv = __shfl(v, d, 64);
      const int di = __shfl(id, d, 64);
      rank += (dv > v || (dv == v && di < id)) ? 1 : 0;
    }
    if (live && rank < K) {
      pv[slot0 * K + rank] = v;
      pi[slot0 * K + rank] = id;
    }
    if (lane >= n_cand && lane < K) {                     // fewer than K selectable columns in this part
      pv[slot0 * K + lane] = -__builtin_inff();
      pi[slot0 * K + lane] = TOPK_NONE;
    }
  }
}

// ------------------------------------------------------------------------------------------------- stage 2
// bf16, no history.  One wave per row: lane p < TOPK_PARTS owns part p's sorted list in registers (one round trip; a load per round
// made the K rounds K dependent round trips); K rounds of wave argmax over the list heads, the winner shifts its list up.
template <int K>
__global__ __launch_bounds__(64) void topk_merge_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                        const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                                        float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const bool live = lane < TOPK_PARTS;
  const size_t slot0 = (size_t)row * TOPK_PARTS + (live ? lane : 0);
  const RowLse<true> lse = row_lse<true>(pm, ps, row, lane);
  float lv[K];
  int li[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    lv[j] = live ? pv[slot0 * K + j] : -__builtin_inff();
    li[j] = live ? pi[slot0 * K + j] : TOPK_NONE;
  }
#pragma unroll
  for (int r = 0; r < K; ++r) {
    float v = lv[0];
    int id = li[0];
    wave_best(v, id);
    if (id == li[0] && v == lv[0]) {                // this part's head won (columns are unique; exhausted lists hold TOPK_NONE)
#pragma unroll
      for (int j = 0; j + 1 < K; ++j) {
        lv[j] = lv[j + 1];
        li[j] = li[j + 1];
      }
      lv[K - 1] = -__builtin_inff();
      li[K - 1] = TOPK_NONE;
    }
    if (lane == 0) {
      out_val[(size_t)row * K + r] = lse.logprob(v);
      out_idx[(size_t)row * K + r] = id;
    }
  }
}

// fp32, no history.  NT >= 16 k threads: one candidate per thread, each ranked against all through LDS.
template <int NT>
__global__ __launch_bounds__(NT) void f32_topk_merge_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                             const float* __restrict__ pv, const int32_t* __restrict__ pi, int k,
                                                             float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  __shared__ float cv[NT];
  __shared__ int ci[NT];
  __shared__ float stat[2];
  __shared__ int nvalid;
  const int row = blockIdx.x, t = threadIdx.x;
  const int n = TOPK_PARTS * k;                          // <= NT: one candidate per thread
  if (t == 0) nvalid = 0;
  float v = -__builtin_inff();
  int id = TOPK_NONE;
  if (t < n) v = pv[(size_t)row * n + t], id = pi[(size_t)row * n + t];
  cv[t] = v, ci[t] = id;
  if (t < 64) {
    const RowLse<false> w0 = row_lse<false>(pm, ps, row, t);
    if (t == 0) stat[0] = w0.mx, stat[1] = w0.lg;
  }
  __syncthreads();
  const RowLse<false> lse{stat[0], stat[1]};
  if (id != TOPK_NONE) {
    atomicAdd(&nvalid, 1);
    const int rank = rank_in_lds(cv, ci, n, v, id);
    if (rank < k) out_val[(size_t)row * k + rank] = lse.logprob(v), out_idx[(size_t)row * k + rank] = id;
  }
  __syncthreads();
  if (t >= nvalid && t < k) out_val[(size_t)row * k + t] = -__builtin_inff(), out_idx[(size_t)row * k + t] = TOPK_NONE;   // fewer than k selectable columns
}

// With history, bf16 and fp32.  One wave per row: a pool in LDS of the parts' 16 k candidates as log-probs and, in mode 0, the row's
// history tokens as rep_penalty(x - lse) (banned or out-of-range tokens: -inf, never picked); then k rounds of "the best pool entry
// after the previous pick".  The copies of a token that occurs more than once in the history are EQUAL pool entries, so "after the
// previous pick" passes over them: penalised once, listed at most once.
template <typename T, bool FAST>
__global__ __launch_bounds__(64) void topk_merge_hist_kernel(const T* __restrict__ logits, int ld, int V, int k,
                                                             const int32_t* __restrict__ banned, int n_banned,
                                                             const int32_t* __restrict__ hist, int hist_ld,
                                                             const int32_t* __restrict__ hist_len, float p, int mode, int cap,
                                                             const float* __restrict__ pm, const float* __restrict__ ps,
                                                             const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                                             float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  extern __shared__ float pool_v[];                      // [cap] values, then [cap] ids; cap >= 16 k + min(hist_ld, 2048)
  int* pool_i = (int*)(pool_v + cap);
  const int row = blockIdx.x, lane = threadIdx.x;
  const RowLse<FAST> lse = row_lse<FAST>(pm, ps, row, lane);
  const int n = TOPK_PARTS * k;
  for (int i = lane; i < n; i += 64) {
    const float v = pv[(size_t)row * n + i];
    const int id = pi[(size_t)row * n + i];
    pool_v[i] = (id != TOPK_NONE && v > -__builtin_inff()) ? lse.logprob(v) : -__builtin_inff();
    pool_i[i] = id;
  }
  const int hl = mode == 0 ? min(max(hist_len[row], 0), min(min(hist_ld, TOPK_HIST_MAX), cap - n)) : 0;
  const int32_t* hr = hist + (size_t)row * hist_ld;
  for (int i = lane; i < hl; i += 64) {
    const int c = hr[i];
    float v = -__builtin_inff();
    if (c >= 0 && c < V) {
      bool ban = false;
      for (int b = 0; b < n_banned; ++b) ban |= (banned[b] == c);
      if (!ban) v = rep_penalty(lse.logprob((float)logits[(size_t)row * ld + c]), p);
    }
    pool_v[n + i] = v;
    pool_i[n + i] = c;
  }
  __syncthreads();
  const int total = n + hl;
  float pvv = __builtin_inff();
  int pii = -1;
  for (int r = 0; r < k; ++r) {
    float best = -__builtin_inff();
    int bid = TOPK_NONE;
    for (int i = lane; i < total; i += 64) {
      const float v = pool_v[i];
      const int id = pool_i[i];
      if (!(v > -__builtin_inff())) continue;
      const bool after = v < pvv || (v == pvv && id > pii);
      if (!after || v < best || (v == best && id >= bid)) continue;
      best = v, bid = id;
    }
    wave_best(best, bid);
    if (lane == 0) {
      out_val[(size_t)row * k + r] = bid == TOPK_NONE ? -__builtin_inff() : best;
      out_idx[(size_t)row * k + r] = bid;
    }
    pvv = best, pii = bid;
    if (bid == TOPK_NONE) pvv = -__builtin_inff(), pii = TOPK_NONE;
  }
}

// ------------------------------------------------------------------------------------------------- one fp32 row per workgroup
// log_softmax + top-k of one fp32 logits row per 1024-thread block, for rows the 16-part split does not serve.  Threshold form
// (three passes over the row instead of 2 + k): tau = the k-th largest of the 1024 per-thread maxima over selectable columns -- at
// least k columns are >= tau, so the k best all are; the columns >= tau (a handful) are collected in LDS during the sum-of-exp pass
// and ranked.  More than CAND of them (massive ties): the round-by-round form below takes over.
constexpr int F32_TOPK_CAND = 512;
__global__ __launch_bounds__(1024) void f32_logprob_topk_kernel(const float* __restrict__ logits, int ld, int V, int k,
                                                                const int32_t* __restrict__ banned, int n_banned,
                                                                float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  __shared__ float red[16];
  __shared__ float bv[16];
  __shared__ int bi[16];
  __shared__ float cand_v[F32_TOPK_CAND];
  __shared__ int cand_i[F32_TOPK_CAND];
  __shared__ int cand_n;
  const float* x = logits + (size_t)blockIdx.x * ld;
  const int t = threadIdx.x;
  auto is_banned = [&](int c) {
    bool ban = false;
    for (int b = 0; b < n_banned; ++b) ban |= banned[b] == c;
    return ban;
  };
  if (t == 0) cand_n = 0;
  float m = -__builtin_inff(), msel = -__builtin_inff();
  for (int c = t; c < V; c += 1024) {
    const float v = x[c];
    m = fmaxf(m, v);
    if (v > msel && !is_banned(c)) msel = v;
  }
  m = block_max<16>(m, red);
  // tau: k rounds of (block maximum of the per-thread selectable maxima, retire one thread that holds it)
  float mine = msel, tau = -__builtin_inff();
  for (int r = 0; r < k; ++r) {
    float best = mine;
    int who = t;
    block_best<16>(best, who, bv, bi);
    tau = best;
    if (t == who) mine = -__builtin_inff();
  }
  float s = 0.f;
  for (int c = t; c < V; c += 1024) {
    const float v = x[c];
    s += expf(v - m);
    if (v >= tau && v > -__builtin_inff() && !is_banned(c)) {
      const int slot = atomicAdd(&cand_n, 1);
      if (slot < F32_TOPK_CAND) cand_v[slot] = v, cand_i[slot] = c;
    }
  }
  s = block_sum<16>(s, red);                         // (its barriers also publish the candidates)
  const RowLse<false> lse{m, logf(s)};
  const int n_cand = cand_n;
  if (n_cand <= F32_TOPK_CAND) {
    if (t < n_cand) {
      const float v = cand_v[t];
      const int id = cand_i[t];
      const int rank = rank_in_lds(cand_v, cand_i, n_cand, v, id);
      if (rank < k) {
        out_val[(size_t)blockIdx.x * k + rank] = lse.logprob(v);
        out_idx[(size_t)blockIdx.x * k + rank] = id;
      }
    }
    if (t >= n_cand && t < k) {                      // fewer than k selectable columns
      out_val[(size_t)blockIdx.x * k + t] = -__builtin_inff();
      out_idx[(size_t)blockIdx.x * k + t] = TOPK_NONE;
    }
    return;
  }
  // general form: k rounds of "the best column after the previous pick"
  float pv = __builtin_inff();
  int pi = -1;
  for (int r = 0; r < k; ++r) {
    float best = -__builtin_inff();
    int bid = TOPK_NONE;
    for (int c = t; c < V; c += 1024) {
      const float v = x[c];
      const bool after = v < pv || (v == pv && c > pi);
      if (!after || v < best || (v == best && c > bid)) continue;
      if (!is_banned(c)) best = v, bid = c;
    }
    block_best<16>(best, bid, bv, bi);
    pv = best, pi = bid;
    if (t == 0) {
      out_val[(size_t)blockIdx.x * k + r] = bid == TOPK_NONE ? -__builtin_inff() : lse.logprob(best);
      out_idx[(size_t)blockIdx.x * k + r] = bid;
    }
    if (bid == TOPK_NONE) pv = -__builtin_inff();      // fewer than k selectable columns: the remaining picks are empty too
  }
}

// ------------------------------------------------------------------------------------------------- host side
// the workspace of the two-launch forms: M * 16 * (2 + 2 k) floats = pm | ps | pv | pi
struct TopkWs {
  float *pm, *ps, *pv;
  int32_t* pi;
};
inline bool topk_ws_split(float* workspace, int64_t workspace_floats, int M, int k, TopkWs& w) {
  const size_t slots = (size_t)M * TOPK_PARTS;
  if (!workspace || (size_t)workspace_floats < slots * (2 + 2 * (size_t)k)) return false;
  w.pm = workspace;
  w.ps = w.pm + slots;
  w.pv = w.ps + slots;
  w.pi = (int32_t*)(w.pv + slots * k);
  return true;
}
// chunks of VEC columns per part; a part must fit the register window of topk_part_kernel (and its LDS bitmask)
template <int VEC>
inline int topk_part_chunks(int V) {
  return ((V + VEC - 1) / VEC + TOPK_PARTS - 1) / TOPK_PARTS;
}

template <typename T, int VEC, int MAXC, bool FAST, bool HIST>
int topk_part_launch(const T* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned, const int32_t* hist, int hist_ld,
                     const int32_t* hist_len, float penalty, int mode, const TopkWs& w, hipStream_t stream) {
  if (k <= 16) {
    TASU_LAUNCH((topk_part_kernel<T, VEC, MAXC, FAST, TOPK_PCAND, HIST>), dim3(M, TOPK_PARTS), dim3(256), 0, stream, logits, ld, V, k, banned,
                n_banned, hist, hist_ld, hist_len, penalty, mode, w.pm, w.ps, w.pv, w.pi);
  } else {
    TASU_LAUNCH((topk_part_kernel<T, VEC, MAXC, FAST, 2 * TOPK_PCAND, HIST>), dim3(M, TOPK_PARTS), dim3(256), 0, stream, logits, ld, V, k,
                banned, n_banned, hist, hist_ld, hist_len, penalty, mode, w.pm, w.ps, w.pv, w.pi);
  }
  return TASU_OK;
}

template <typename T, int VEC, int MAXC, bool FAST>
int topk_hist_launch(const T* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned, const int32_t* hist, int hist_ld,
                     const int32_t* hist_len, float penalty, int mode, float* out_val, int32_t* out_idx, float* workspace,
                     int64_t workspace_floats, hipStream_t stream) {
  if (!logits || !out_val || !out_idx || !workspace || !hist || !hist_len || M <= 0 || V <= 0 || ld < V || ld % VEC ||
      ((uintptr_t)logits & 15) || k <= 0 || k > TOPK_MAX || n_banned < 0 || (n_banned > 0 && !banned) || hist_ld <= 0 ||
      !(penalty > 0.f) || (mode != 0 && mode != 1))
    return TASU_ERR_ARG;
  TopkWs w;
  if (topk_part_chunks<VEC>(V) > 256 * MAXC || !topk_ws_split(workspace, workspace_floats, M, k, w)) return TASU_ERR_ARG;
  const int cap = TOPK_PARTS * k + (mode == 0 ? (hist_ld < TOPK_HIST_MAX ? hist_ld : TOPK_HIST_MAX) : 0);
  if (int rc = topk_part_launch<T, VEC, MAXC, FAST, true>(logits, ld, M, V, k, banned, n_banned, hist, hist_ld, hist_len, penalty, mode, w, stream))
    return rc;
  TASU_LAUNCH((topk_merge_hist_kernel<T, FAST>), dim3(M), dim3(64), (size_t)cap * 8, stream, logits, ld, V, k, banned, n_banned, hist, hist_ld,
              hist_len, penalty, mode, cap, w.pm, w.ps, w.pv, w.pi, out_val, out_idx);
  return TASU_OK;
}
}  // namespace

extern "C" int tasu_logprob_topk(const void* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned,
                                 float* out_val, int32_t* out_idx, float* workspace, int64_t workspace_floats, void* stream) {
  if (!logits || !out_val || !out_idx || !workspace || M <= 0 || V <= 0 || ld < V || ld % 8 || k <= 0 || k > TOPK_MAX ||
      n_banned < 0 || (n_banned > 0 && !banned))
    return TASU_ERR_ARG;
  TopkWs w;
  if (!topk_ws_split(workspace, workspace_floats, M, k, w)) return TASU_ERR_ARG;
  // (the register lists of the scan's fallback and of the merge need k at compile time)
#define TOPK_CASE(KK)                                                                                                         \
  case KK:                                                                                                                    \
    TASU_LAUNCH(topk_part_bf16_kernel<KK>, dim3(M, TOPK_PARTS), dim3(256), 0, (hipStream_t)stream, (const bf16*)logits, ld, V, \
                banned, n_banned, w.pm, w.ps, w.pv, w.pi);                                                                    \
    TASU_LAUNCH(topk_merge_kernel<KK>, dim3(M), dim3(64), 0, (hipStream_t)stream, w.pm, w.ps, w.pv, w.pi, out_val, out_idx);   \
    return TASU_OK;
  switch (k) {
    TOPK_CASE(1) TOPK_CASE(2) TOPK_CASE(4) TOPK_CASE(6) TOPK_CASE(8) TOPK_CASE(16)
    // the widths of 5, 6, 7 and 9..16 beams (k = 2 * num_beams)
    TOPK_CASE(10) TOPK_CASE(12) TOPK_CASE(14) TOPK_CASE(18) TOPK_CASE(20) TOPK_CASE(22) TOPK_CASE(24) TOPK_CASE(26) TOPK_CASE(28)
    TOPK_CASE(30) TOPK_CASE(32)
    default:
      return TASU_ERR_ARG;
  }
#undef TOPK_CASE
}

extern "C" int tasu_f32_logprob_topk(const float* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned, float* out_val,
                                     int32_t* out_idx, float* workspace, int64_t workspace_floats, void* stream) {
  if (!logits || !out_val || !out_idx || M <= 0 || V <= 0 || ld < V || k <= 0 || k > TOPK_MAX || n_banned < 0 || (n_banned > 0 && !banned))
    return TASU_ERR_ARG;
  // with a workspace of M * 16 * (2 + 2 k) floats, 16-byte aligned rows and a vocabulary the parts hold in registers: two launches,
  // the row split over 16 workgroups; otherwise one workgroup per row
  TopkWs w;
  if (topk_ws_split(workspace, workspace_floats, M, k, w) && ld % 4 == 0 && !((uintptr_t)logits & 15) &&
      topk_part_chunks<4>(V) <= 256 * TOPK_MAXC_F32 && M > 1) {
    if (int rc = topk_part_launch<float, 4, TOPK_MAXC_F32, false, false>(logits, ld, M, V, k, banned, n_banned, nullptr, 0, nullptr, 1.f, 0, w,
                                                              (hipStream_t)stream))
      return rc;
    if (k <= 16)
      TASU_LAUNCH(f32_topk_merge_kernel<256>, dim3(M), dim3(256), 0, (hipStream_t)stream, w.pm, w.ps, w.pv, w.pi, k, out_val, out_idx);
    else
      TASU_LAUNCH(f32_topk_merge_kernel<512>, dim3(M), dim3(512), 0, (hipStream_t)stream, w.pm, w.ps, w.pv, w.pi, k, out_val, out_idx);
    return TASU_OK;
  }
  TASU_LAUNCH(f32_logprob_topk_kernel, dim3(M), dim3(1024), 0, (hipStream_t)stream, logits, ld, V, k, banned, n_banned, out_val, out_idx);
  return TASU_OK;
}

extern "C" int tasu_logprob_topk_hist(const void* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned,
                                      const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, int mode,
                                      float* out_val, int32_t* out_idx, float* workspace, int64_t workspace_floats, void* stream) {
  return topk_hist_launch<bf16, 8, TOPK_MAXC_BF16, true>((const bf16*)logits, ld, M, V, k, banned, n_banned, hist, hist_ld, hist_len, penalty, mode, out_val,
                                            out_idx, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int tasu_f32_logprob_topk_hist(const float* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned,
                                          const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, int mode,
                                          float* out_val, int32_t* out_idx, float* workspace, int64_t workspace_floats, void* stream) {
  return topk_hist_launch<float, 4, TOPK_MAXC_F32, false>(logits, ld, M, V, k, banned, n_banned, hist, hist_ld, hist_len, penalty, mode, out_val, out_idx,
                                               workspace, workspace_floats, (hipStream_t)stream);
}
