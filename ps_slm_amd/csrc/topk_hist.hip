// HF RepetitionPenaltyLogitsProcessor on the device decode loop (generate(repetition_penalty = p), p != 1): the per-row
// hypothesis history next to the beam state, and the log-softmax + top-k of tasu_logprob_topk / tasu_f32_logprob_topk with the
// rule  score' = score < 0 ? score * p : score / p  applied once to every distinct token of the row's history.
//   mode 1 (greedy, num_beams = 1): HF hands the processor the RAW logits -- the part scan penalises the history columns before
//           max / sum-exp / selection; everything after it is the unpenalised form's.
//   mode 0 (beam search): HF hands it the log-softmax output and does not renormalise.  The order of a history column against the
//           others depends on the row's log-sum-exp, which a column part does not know: the part scan keeps history columns out of its
//           candidates (they count in max / sum-exp unmodified) and the merge launch adds the row's history tokens as candidates
//           with p * (x - lse).
// The 16-part split and the two launches of the unpenalised kernels stay: no further pass over V.  Membership of a column in the
// history is one bit of a per-workgroup LDS bitmask over the part's column range (set from the history with atomicOr, at most 2048
// entries): thread t's chunk of VEC consecutive columns owns VEC consecutive bits, so a wave's 64 chunk reads touch 8 or 16
// CONSECUTIVE 32-bit words (distinct banks; the lanes that share a word read the same address, which LDS broadcasts) -- one
// conflict-free LDS read per VEC columns.
#include "common.h"
#include "../../include/tasu_hip.h"

namespace {
constexpr int HT_PARTS = 16;          // column parts per row (the workspace layout of tasu_logprob_topk)
constexpr int HT_PCAND = 64;          // threshold form: candidates a part ranks in one wave (k <= 16; k <= 32: twice as many, ranked through LDS)
constexpr int HT_HIST_MAX = 2048;     // history entries per row (the decode context limit)
constexpr int HT_NONE = 0x7fffffff;

__device__ __forceinline__ float rep_penalty(float s, float p) { return s < 0.f ? s * p : s / p; }

template <typename T, int VEC>
struct HtVec;
template <>
struct HtVec<bf16, 8> {
  typedef bf16x8 type;
};
template <>
struct HtVec<float, 4> {
  typedef f32x4 type;
};

// Stage 1, grid (M, 16), 256 threads: the part's columns live in registers (one read).  pm / ps = max and sum exp(x - max) over
// its columns (mode 1: history columns penalised first), pv / pi = its k best selectable columns (value descending, column
// ascending; mode 0: history columns are not selectable here) by the threshold form, or on massive ties by k rounds of block argmax.
template <typename T, int VEC, int MAXC, bool FAST, int PCAND>
__global__ __launch_bounds__(256) void topk_part_hist_kernel(const T* __restrict__ logits, int ld, int V, int k,
                                                             const int32_t* __restrict__ banned, int n_banned,
                                                             const int32_t* __restrict__ hist, int hist_ld,
                                                             const int32_t* __restrict__ hist_len, float p, int mode,
                                                             float* __restrict__ pm, float* __restrict__ ps, float* __restrict__ pv,
                                                             int32_t* __restrict__ pi) {
  typedef typename HtVec<T, VEC>::type VT;
  constexpr int NWORD = 256 * MAXC * VEC / 32;
  __shared__ float red[4];
  __shared__ float wtau[4];
  __shared__ float bv[4];
  __shared__ int bi[4];
  __shared__ float cand_v[PCAND];
  __shared__ int cand_i[PCAND];
  __shared__ int cand_n;
  __shared__ unsigned hbits[NWORD];
  const int row = blockIdx.x, part = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const T* x = logits + (size_t)row * ld;
  const int nv = (V + VEC - 1) / VEC, per = (nv + HT_PARTS - 1) / HT_PARTS;      // (per <= 256 * MAXC: checked by the host entry)
  const int v0 = part * per, v1 = min(nv, v0 + per);
  const int c0 = v0 * VEC, ncol = max(v1 - v0, 0) * VEC;
  for (int i = t; i < NWORD; i += 256) hbits[i] = 0u;
  if (t == 0) cand_n = 0;
  VT xs[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int cv = v0 + t + i * 256;
    if (cv < v1) xs[i] = *(const VT*)(x + (size_t)cv * VEC);
  }
  __syncthreads();
  const int hl = min(max(hist_len[row], 0), min(hist_ld, HT_HIST_MAX));
  const int32_t* hr = hist + (size_t)row * hist_ld;
  for (int i = t; i < hl; i += 256) {
    const int c = hr[i], r = c - c0;
    if (r >= 0 && r < ncol && c < V) atomicOr(&hbits[r >> 5], 1u << (r & 31));
  }
  __syncthreads();
  const int ban0 = n_banned > 0 ? banned[0] : -1, ban1 = n_banned > 1 ? banned[1] : -1;
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
    const int q = t + i * 256, cv = v0 + q;
    const unsigned hm = (hbits[(q * VEC) >> 5] >> ((q * VEC) & 31)) & ((1u << VEC) - 1u);
    selm[i] = 0u;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int c = cv * VEC + j;
      float v = -__builtin_inff();
      if (cv < v1 && c < V) {
        v = (float)xs[i][j];
        const bool in_hist = (hm >> j) & 1u;
        if (mode == 1 && in_hist) v = rep_penalty(v, p);
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
  // tau = the largest, over the four waves, of the wave's k-th largest per-thread selectable maximum: >= k columns are >= tau
  float mine = msel, kth = -__builtin_inff();
  for (int r = 0; r < k; ++r) {
    kth = wave_max(mine);
    const unsigned long long holders = __ballot(mine == kth);
    if (lane == __ffsll((long long)holders) - 1) mine = -__builtin_inff();
  }
  if (lane == 0) wtau[wave] = kth;
  __syncthreads();
  const float tau = fmaxf(fmaxf(wtau[0], wtau[1]), fmaxf(wtau[2], wtau[3]));
  float s = 0.f;
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
  s = block_sum<4>(s, red);                              // (its barriers also publish the candidates)
  const size_t slot0 = (size_t)row * HT_PARTS + part;
  if (t == 0) pm[slot0] = m, ps[slot0] = s;
  const int n_cand = cand_n;
  if (n_cand <= PCAND) {
    if constexpr (PCAND > 64) {                            // as many threads as candidates rank them by reading LDS
      if (t < n_cand) {
        const float v = cand_v[t];
        const int id = cand_i[t];
        int rank = 0;
        for (int d = 0; d < n_cand; ++d) rank += (cand_v[d] > v || (cand_v[d] == v && cand_i[d] < id)) ? 1 : 0;
        if (rank < k) pv[slot0 * k + rank] = v, pi[slot0 * k + rank] = id;
      }
      if (t >= n_cand && t < k) pv[slot0 * k + t] = -__builtin_inff(), pi[slot0 * k + t] = HT_NONE;
    } else if (wave == 0) {
      const bool live = lane < n_cand;
      const float v = live ? cand_v[lane] : -__builtin_inff();
      const int id = live ? cand_i[lane] : HT_NONE;
      int rank = 0;
      for (int d = 0; d < n_cand; ++d) {
        const float dv = __shfl(v, d, 64);
        const int di = __shfl(id, d, 64);
        rank += (dv > v || (dv == v && di < id)) ? 1 : 0;
      }
      if (live && rank < k) pv[slot0 * k + rank] = v, pi[slot0 * k + rank] = id;
      if (lane >= n_cand && lane < k) pv[slot0 * k + lane] = -__builtin_inff(), pi[slot0 * k + lane] = HT_NONE;
    }
    return;
  }
  // massive ties: k rounds of "the best selectable column after the previous pick" over the registers
  float pvv = __builtin_inff();
  int pii = -1;
  for (int r = 0; r < k; ++r) {
    float best = -__builtin_inff();
    int bid = HT_NONE;
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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bid, o, 64);
      if (ov > best || (ov == best && oi < bid)) best = ov, bid = oi;
    }
    __syncthreads();
    if (lane == 0) bv[wave] = best, bi[wave] = bid;
    __syncthreads();
    best = bv[0], bid = bi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < bid)) best = bv[w], bid = bi[w];
    if (t == 0) pv[slot0 * k + r] = bid == HT_NONE ? -__builtin_inff() : best, pi[slot0 * k + r] = bid;
    pvv = best, pii = bid;
    if (bid == HT_NONE) pvv = -__builtin_inff(), pii = HT_NONE;
  }
}

// Stage 2, one wave per row: lse from the parts' (max, sum); a pool in LDS of the parts' 16 k candidates as log-probs and, in mode 0,
// the row's history tokens as rep_penalty(x - lse) (banned or out-of-range tokens: -inf, never picked); then k rounds of "the best
// pool entry after the previous pick" in the (value descending, id ascending) order.  The copies of a token that occurs more than
// once in the history are EQUAL pool entries, so "after the previous pick" passes over them: penalised once, listed at most once.
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
  const bool lp_ = lane < HT_PARTS;
  const float mp = lp_ ? pm[(size_t)row * HT_PARTS + lane] : -__builtin_inff();
  const float sp = lp_ ? ps[(size_t)row * HT_PARTS + lane] : 0.f;
  const float mx = wave_max(mp);
  const float sm = wave_sum(lp_ && mp > -__builtin_inff() ? sp * (FAST ? __expf(mp - mx) : expf(mp - mx)) : 0.f);
  const float lg = FAST ? __logf(sm) : logf(sm);
  auto logprob = [&](float v) { return FAST ? v - (mx + lg) : (v - mx) - lg; };   // (the two unpenalised kernels' own forms)
  const int n = HT_PARTS * k;
  for (int i = lane; i < n; i += 64) {
    const float v = pv[(size_t)row * n + i];
    const int id = pi[(size_t)row * n + i];
    pool_v[i] = (id != HT_NONE && v > -__builtin_inff()) ? logprob(v) : -__builtin_inff();
    pool_i[i] = id;
  }
  const int hl = mode == 0 ? min(max(hist_len[row], 0), min(min(hist_ld, HT_HIST_MAX), cap - n)) : 0;
  const int32_t* hr = hist + (size_t)row * hist_ld;
  for (int i = lane; i < hl; i += 64) {
    const int c = hr[i];
    float v = -__builtin_inff();
    if (c >= 0 && c < V) {
      bool ban = false;
      for (int b = 0; b < n_banned; ++b) ban |= (banned[b] == c);
      if (!ban) v = rep_penalty(logprob((float)logits[(size_t)row * ld + c]), p);
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
    int bid = HT_NONE;
    for (int i = lane; i < total; i += 64) {
      const float v = pool_v[i];
      const int id = pool_i[i];
      if (!(v > -__builtin_inff())) continue;
      const bool after = v < pvv || (v == pvv && id > pii);
      if (!after || v < best || (v == best && id >= bid)) continue;
      best = v, bid = id;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bid, o, 64);
      if (ov > best || (ov == best && oi < bid)) best = ov, bid = oi;
    }
    if (lane == 0) {
      out_val[(size_t)row * k + r] = bid == HT_NONE ? -__builtin_inff() : best;
      out_idx[(size_t)row * k + r] = bid;
    }
    pvv = best, pii = bid;
    if (bid == HT_NONE) pvv = -__builtin_inff(), pii = HT_NONE;
  }
}

// The hypothesis history of every beam row after tasu_beam_update: row m's history = its parent's (next_src[m]) + its new token
// (next_ids[m]), IN PLACE, one workgroup per utterance staging its n_beams rows through LDS (a beam's parent is a row of the same
// utterance; the pattern of the cache row index in tasu_decode_step_prologue), so the launch replays in a captured graph with fixed
// pointers.  n = ctl[0] = positions generated including the one just decided; ctl[1] (done): nothing is read after it, no-op.
__global__ __launch_bounds__(256) void beam_hist_update_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ hist_len,
                                                               const int32_t* __restrict__ ctl, const int32_t* __restrict__ next_src,
                                                               const int32_t* __restrict__ next_ids, int nb, int M, int max_new) {
  extern __shared__ int stage[];                          // [nb][max_new]
  const int n = ctl[0];
  if (ctl[1] || n < 1 || n > max_new) return;             // (block-uniform)
  const int m0 = blockIdx.x * nb, rows = min(nb, M - m0);
  for (int r = 0; r < rows; ++r) {
    int src = next_src[m0 + r];
    if (src < m0 || src >= m0 + rows) src = m0 + r;
    for (int i = threadIdx.x; i < n - 1; i += 256) stage[r * max_new + i] = hist[(size_t)src * max_new + i];
  }
  __syncthreads();
  for (int r = 0; r < rows; ++r) {
    int32_t* dst = hist + (size_t)(m0 + r) * max_new;
    for (int i = threadIdx.x; i < n - 1; i += 256) dst[i] = stage[r * max_new + i];
    if (threadIdx.x == 0) {
      dst[n - 1] = next_ids[m0 + r];
      hist_len[m0 + r] = n;
    }
  }
}

// More than 5 beams: n_beams * max_new ints no longer fit the LDS a launch gets by default, so the rows are staged HT_WIDE_COLS
// positions at a time (dst[r, i] = src[parent r, i] for the SAME i: a pass only reads and writes its own columns).
constexpr int HT_WIDE_NB = 16, HT_WIDE_COLS = 512;
__global__ __launch_bounds__(256) void beam_hist_update_wide_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ hist_len,
                                                                    const int32_t* __restrict__ ctl, const int32_t* __restrict__ next_src,
                                                                    const int32_t* __restrict__ next_ids, int nb, int M, int max_new) {
  __shared__ int stage[HT_WIDE_NB * HT_WIDE_COLS];
  const int n = ctl[0];
  if (ctl[1] || n < 1 || n > max_new) return;             // (block-uniform)
  const int m0 = blockIdx.x * nb, rows = min(nb, M - m0);
  for (int c0 = 0; c0 < n - 1; c0 += HT_WIDE_COLS) {
    const int w = min(HT_WIDE_COLS, n - 1 - c0);
    for (int r = 0; r < rows; ++r) {
      int src = next_src[m0 + r];
      if (src < m0 || src >= m0 + rows) src = m0 + r;
      for (int i = threadIdx.x; i < w; i += 256) stage[r * HT_WIDE_COLS + i] = hist[(size_t)src * max_new + c0 + i];
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      int32_t* dst = hist + (size_t)(m0 + r) * max_new + c0;
      for (int i = threadIdx.x; i < w; i += 256) dst[i] = stage[r * HT_WIDE_COLS + i];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < rows) {
    hist[(size_t)(m0 + threadIdx.x) * max_new + n - 1] = next_ids[m0 + threadIdx.x];
    hist_len[m0 + threadIdx.x] = n;
  }
}

template <typename T, int VEC, int MAXC, bool FAST>
int topk_hist_launch(const T* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned, const int32_t* hist, int hist_ld,
                     const int32_t* hist_len, float penalty, int mode, float* out_val, int32_t* out_idx, float* workspace,
                     int64_t workspace_floats, hipStream_t stream) {
  if (!logits || !out_val || !out_idx || !workspace || !hist || !hist_len || M <= 0 || V <= 0 || ld < V || ld % VEC ||
      ((uintptr_t)logits & 15) || k <= 0 || k > 32 || n_banned < 0 || (n_banned > 0 && !banned) || hist_ld <= 0 ||
      !(penalty > 0.f) || (mode != 0 && mode != 1))
    return TASU_ERR_ARG;
  const int nv = (V + VEC - 1) / VEC, per = (nv + HT_PARTS - 1) / HT_PARTS;
  if (per > 256 * MAXC) return TASU_ERR_ARG;               // a part must fit the register window (and its LDS bitmask)
  const size_t slots = (size_t)M * HT_PARTS;
  if ((size_t)workspace_floats < slots * (2 + 2 * (size_t)k)) return TASU_ERR_ARG;
  float* pm = workspace;
  float* ps = pm + slots;
  float* pv = ps + slots;
  int32_t* pi = (int32_t*)(pv + slots * k);
  const int cap = HT_PARTS * k + (mode == 0 ? (hist_ld < HT_HIST_MAX ? hist_ld : HT_HIST_MAX) : 0);
  if (k <= 16) {
    TASU_LAUNCH((topk_part_hist_kernel<T, VEC, MAXC, FAST, HT_PCAND>), dim3(M, HT_PARTS), dim3(256), 0, stream, logits, ld, V, k, banned,
                n_banned, hist, hist_ld, hist_len, penalty, mode, pm, ps, pv, pi);
  } else {
    TASU_LAUNCH((topk_part_hist_kernel<T, VEC, MAXC, FAST, 2 * HT_PCAND>), dim3(M, HT_PARTS), dim3(256), 0, stream, logits, ld, V, k, banned,
                n_banned, hist, hist_ld, hist_len, penalty, mode, pm, ps, pv, pi);
  }
  TASU_LAUNCH((topk_merge_hist_kernel<T, FAST>), dim3(M), dim3(64), (size_t)cap * 8, stream, logits, ld, V, k, banned, n_banned, hist, hist_ld,
              hist_len, penalty, mode, cap, pm, ps, pv, pi, out_val, out_idx);
  return TASU_OK;
}
}  // namespace

extern "C" int tasu_logprob_topk_hist(const void* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned,
                                      const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, int mode,
                                      float* out_val, int32_t* out_idx, float* workspace, int64_t workspace_floats, void* stream) {
  return topk_hist_launch<bf16, 8, 6, true>((const bf16*)logits, ld, M, V, k, banned, n_banned, hist, hist_ld, hist_len, penalty, mode, out_val,
                                            out_idx, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int tasu_f32_logprob_topk_hist(const float* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned,
                                          const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, int mode,
                                          float* out_val, int32_t* out_idx, float* workspace, int64_t workspace_floats, void* stream) {
  return topk_hist_launch<float, 4, 10, false>(logits, ld, M, V, k, banned, n_banned, hist, hist_ld, hist_len, penalty, mode, out_val, out_idx,
                                               workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int tasu_beam_hist_update(int32_t* hist, int32_t* hist_len, const int32_t* ctl, const int32_t* next_src,
                                     const int32_t* next_ids, int B, int n_beams, int max_new, void* stream) {
  if (!hist || !hist_len || !ctl || !next_src || !next_ids || B <= 0 || n_beams <= 0 || n_beams > HT_WIDE_NB || max_new <= 0 ||
      max_new > HT_HIST_MAX)
    return TASU_ERR_ARG;
  if (n_beams > 5) {
    TASU_LAUNCH(beam_hist_update_wide_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, hist, hist_len, ctl, next_src, next_ids, n_beams,
                B * n_beams, max_new);
    return TASU_OK;
  }
  TASU_LAUNCH(beam_hist_update_kernel, dim3(B), dim3(256), (size_t)n_beams * max_new * sizeof(int), (hipStream_t)stream, hist, hist_len, ctl,
              next_src, next_ids, n_beams, B * n_beams, max_new);
  return TASU_OK;
}
