// generate(do_sample = True, num_beams = 1) on the device decode loop: tasu_sample_uniform (the position's uniforms) and
// tasu_sample_rows / tasu_f32_sample_rows (one token per row of bf16 / fp32 logits).
//
// THE DISTRIBUTION is HF's, in HF's order (transformers generation/utils.py _get_logits_processor, then _sample), per row, on fp32
// values of the raw logits x:
//   1. repetition penalty on the row's history tokens, once per distinct token:  x' = x < 0 ? x * p : x / p   (mode 1 of csrc/topk.hip)
//   2. the EOS ban of min_length: banned columns score -inf
//   3. s = x' / T, a correctly rounded fp32 division (a reciprocal multiply moves ties); -0 counts as +0
//   4. top-k: keep s >= (the k-th largest s).  TIES AT THE THRESHOLD ARE KEPT (TopKLogitsWarper: scores < topk(scores, k)[-1] go)
//   5. top-p over the survivors: softmax, accumulated in ASCENDING order of s; entries whose cumulative mass is <= 1 - top_p go,
//      the largest always stays (TopPLogitsWarper, min_tokens_to_keep = 1).  top_p >= 1 turns the step off.
//   6. softmax of what is left.
// THE DRAW is ours: inverse CDF in ascending TOKEN-ID order over the survivors, w_j = exp(s_j - max s), Z = sum w,
//   token = the smallest survivor i with  sum_{j <= i} w_j > u * Z.
// The uniform of generated position t (0-based; the beam state's device counter ctl[0]) and row r (the utterance) is counter based,
// the splitmix64 finaliser of csrc/lora.hip's dropout masks (mix64) over
//   key = seed ^ (uint64(t) * 0x9E3779B97F4A7C15)            (seed: one int64 in device memory, uploaded per generate() call)
//   z   = mix64(key + uint64(r) * 0xD1B54A32D192ED03)
//   u   = float(z >> 40) * 2^-24                             (the top 24 bits: u in [0, 1 - 2^-24], exact in fp32)
// Seed and counter are read from device memory, never kernel arguments: a replayed hipGraph draws fresh numbers every position and
// every call.  The sampler reads u from a buffer, so tests feed it any u.
//
// tasu_sample_rows: one 1024-thread workgroup per row; two passes over the row (the first from HBM, the second from L2), or five:
//   a. every thread's largest selectable x' (s is monotone in x': its largest s is one division); tau0 = the k-th largest of those
//      1024 maxima (a radix select over one key per thread): at least k columns are >= tau0, so everything below it is out of the
//      top k.  Fewer than k threads with a selectable column (a short row): tau0 = -inf.  From here on a column is divided by T only
//      when its x' reaches xlo, a bound 2^-21 relative below tau0 * T (three fp32 roundings lie between x' and the comparison with
//      tau0): the scans are a load, the history bit, the ban and one comparison per column.
//   b. the columns >= tau0 (a small multiple of k) go to an LDS candidate list; radix select (11 + 11 + 10 bits of the
//      order-preserving integer image of s, an INTEGER LDS histogram per pass) of the k-th largest s among them: tau, the number of
//      columns above it and the number equal to it.  More candidates than the list holds (top_k near the pool size, many ties): the
//      three radix passes and the gather below read the row itself instead.
//   c. the survivors s >= tau go to an LDS pool of TASU_SAMPLE_POOL entries.  More survivors than the pool holds -- only possible
//      when more entries TIE at the threshold than the pool has room for -- are cut in token-id order (the columns above tau and the
//      first ties by id).  This departs from HF, which keeps every tie.
//   d. an exact rank sort of the pool by (s descending, id ascending); weights w = expf(s - max); top-p: suffix sums S_r (ascending s
//      = from the end of the sorted pool), the cut is the first rank r >= 1 with S_r <= (1 - top_p) * S_0.  Among equal s the larger
//      ids go first (HF's sort leaves that order open).
//   e. a rank sort of the kept entries by id, their inclusive prefix sums C in id order, Z = the last of them, and the pick: the
//      first entry with C > u * Z.  u <= 1 - 2^-24 makes fl(u * Z) < Z, so an entry always qualifies.
// Every sum is a fixed tree (6 shuffle levels per wave, then the waves' totals in order): no floating-point atomics, bit-identical
// run to run.  The pool order after the atomics of step c is arbitrary and does not matter: the sorts are total orders.
// Output in tasu_logprob_topk's format for k = 2: slot 0 = the token and its log-probability (s - max) - log Z under the final
// distribution, slot 1 = (-inf, 0x7fffffff).  With one beam, tasu_beam_update ranks slot 1 behind slot 0 whatever slot 0 holds
// (-inf + anything < a finite score, and EOS's -1e9 keeps slot 0 finite), so the filler never becomes the running token.
// A row without a selectable column (all -inf / NaN) yields token 0 with -inf: ids stay inside the embedding table.
//
// generate(do_sample = True, num_beams = nb > 1), HF's beam-search multinomial sampling (_beam_search with do_sample): tasu_beam_sample_rows
// / tasu_f32_beam_sample_rows, the same kernel with BEAM set; tasu_beam_update_drawn (csrc/beam.hip) consumes its output.
// THE DISTRIBUTION is HF's, per beam row, on fp32 values:
//   0. lp = log_softmax(x) over all V columns, in tasu_logprob_topk's form of the arithmetic mode: bf16 logits x - (max + __logf(sum
//      __expf(x - max))), fp32 logits (x - max) - logf(sum expf(x - max)); the sum is a fixed tree
//   1. repetition penalty ON THE LOG-PROBS of the row's history tokens (mode 0 of csrc/topk.hip), once per distinct token, no renormalisation
//   2. the EOS ban;   3. s = lp' / T, a true division
//   4. top-k at max(top_k, 2) and 5. top-p that never removes the two largest: with more than one beam HF builds the warpers with
//      min_tokens_to_keep = 2.  Ties, the pool's id cut and the ascending-mass form are those of one beam.  Nothing is renormalised.
//   6. HF draws 2 nb of an utterance's nb * V accumulated scores a = s + running score WITHOUT REPLACEMENT in proportion to softmax(a).
// THE DRAW is ours: the Plackett-Luce order of softmax(a) by Gumbel keys, which needs no serial walk per utterance and cannot run out
// of mass.  For output row m = b * nb + j, surviving column v, generated position t (ctl[0]) and the call's seed (both device words):
//   z   = mix64((seed ^ uint64(t) * 0x9E3779B97F4A7C15) + uint64(m * V + v) * 0xD1B54A32D192ED03)
//   u   = (float(z >> 41) + 0.5) * 2^-23                     (23 bits and a half: exact in fp32, 0 < u < 1)
//   key = fl(a + G),  G = -logf(-logf(u)),  a = fl(s + run_scores[m])
// The utterance's draw order is its 2 nb largest keys, descending, then (beam, column) ascending; a row hands over its own K = 2 nb
// largest as out_key / out_val (= a) / out_idx [M, K] in that order, the rest (-inf, -inf, 0x7fffffff).  A filtered column is never a
// candidate: where torch.multinomial would fill a draw of more entries than have probability from zero-probability categories in an
// unspecified order, the keys decide (at the first position beams >= 1, at -1e9, supply them).  `first`: output row m reads logits
// row m / nb (the prompt's last position, B rows of logits).
#include "common.h"
#include "../../include/tasu_hip.h"

namespace {
constexpr int SAMPLE_POOL = TASU_SAMPLE_POOL;
constexpr int SAMPLE_THREADS = 1024, SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_MAX_V = 196608, SAMPLE_MAX_M = 256;
constexpr int SAMPLE_HIST_MAX = 2048;    // history entries per row (the decode context limit)
constexpr int SAMPLE_BINS = 2048;        // 11-bit digits
constexpr int SAMPLE_NONE = 0x7fffffff;
static_assert(SAMPLE_POOL == SAMPLE_THREADS, "one pool entry per thread in the sorts and scans");

__device__ __forceinline__ uint64_t sample_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void sample_uniform_kernel(const int64_t* __restrict__ seed, const int32_t* __restrict__ counter, int M,
                                                             float* __restrict__ u) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= M) return;
  const uint64_t key = (uint64_t)seed[0] ^ ((uint64_t)(uint32_t)counter[0] * 0x9E3779B97F4A7C15ull);
  const uint64_t z = sample_mix64(key + (uint64_t)r * 0xD1B54A32D192ED03ull);
  u[r] = (float)(uint32_t)(z >> 40) * 0x1p-24f;
}

// the order-preserving integer image of a float: a > b  <=>  order_key(a) > order_key(b)  (no NaN, -0 canonicalised before)
__device__ __forceinline__ uint32_t order_key(float s) {
  const uint32_t b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Inclusive scan over the workgroup's 1024 threads in thread order (SUFFIX: from the last thread down): 6 shuffle levels inside the
// wave, then the other waves' totals added one by one in a fixed order.  wt: SAMPLE_WAVES entries of LDS.
template <typename S, bool SUFFIX>
__device__ __forceinline__ S block_scan(S v, S* wt) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const S x = SUFFIX ? __shfl_down(v, o, 64) : __shfl_up(v, o, 64);
    if (SUFFIX ? lane + o < 64 : lane >= o) v += x;
  }
  __syncthreads();
  if (lane == (SUFFIX ? 0 : 63)) wt[w] = v;
  __syncthreads();
  S off = 0;
  if (SUFFIX) {
    for (int i = SAMPLE_WAVES - 1; i > w; --i) off += wt[i];
  } else {
    for (int i = 0; i < w; ++i) off += wt[i];
  }
  return off + v;
}

struct RadixSel {
  uint32_t key;      // the k-th largest key (k clamped to the number of keys)
  int n_gt, n_eq;    // keys above it / equal to it
  int total;         // keys visited (0: nothing else is valid)
};
// The k-th largest of the keys `visit` enumerates (visit(f) calls f(key) for every key of this thread; every pass enumerates the same
// keys).  hist: SAMPLE_BINS ints, wt: SAMPLE_WAVES ints, res: 4 ints of LDS.  Block-uniform result.
template <typename Visit>
__device__ __forceinline__ RadixSel radix_select(int k, Visit visit, int* hist, int* wt, int* res) {
  const int t = threadIdx.x;
  uint32_t prefix = 0u, mask = 0u;
  RadixSel r{0u, 0, 0, 0};
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const int sh = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const uint32_t dm = pass == 2 ? 0x3ffu : 0x7ffu;
    hist[t] = 0;
    hist[t + SAMPLE_THREADS] = 0;
    __syncthreads();
    visit([&](uint32_t key) {
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> sh) & dm], 1);
    });
    __syncthreads();
    const int h0 = hist[2 * t], h1 = hist[2 * t + 1];
    const int sfx = block_scan<int, true>(h0 + h1, wt);           // keys in bins >= 2 t
    if (t == 0) res[3] = sfx;
    __syncthreads();
    if (pass == 0) {
      r.total = res[3];
      if (r.total == 0) return r;                                  // (block-uniform)
      k = min(k, r.total);
    }
    const int g1 = sfx - (h0 + h1), g0 = g1 + h1;                  // keys in bins above 2 t + 1 / above 2 t
    if (g1 < k && k <= g1 + h1) res[0] = 2 * t + 1, res[1] = g1, res[2] = h1;
    if (g0 < k && k <= g0 + h0) res[0] = 2 * t, res[1] = g0, res[2] = h0;
    __syncthreads();
    prefix |= (uint32_t)res[0] << sh;
    mask |= dm << sh;
    r.n_gt += res[1];
    k -= res[1];
    r.n_eq = res[2];
    __syncthreads();                                               // (res and hist are rewritten by the next pass)
  }
  r.key = prefix;
  return r;
}

template <typename T>
struct SampleVec;
template <>
struct SampleVec<bf16> {
  typedef bf16x8 type;
  static constexpr int VEC = 8;
};
template <>
struct SampleVec<float> {
  typedef f32x4 type;
  static constexpr int VEC = 4;
};

// what the BEAM form of sample_rows_kernel needs on top: the device words of the RNG, the rows' running scores, the output
struct BeamDraw {
  const int64_t* seed;
  const int32_t* ctl;
  const float* run_scores;    // [M]
  float* out_key;             // [M, K]
  int nb, first, K;
};

template <typename T, bool HIST, bool BEAM>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(const T* __restrict__ logits, int ld, int V,
                                                                     const float* __restrict__ u, const int32_t* __restrict__ banned,
                                                                     int n_banned, const int32_t* __restrict__ hist, int hist_ld,
                                                                     const int32_t* __restrict__ hist_len, float penalty, float temp,
                                                                     int top_k, float top_p, float* __restrict__ out_val,
                                                                     int32_t* __restrict__ out_idx, BeamDraw bd) {
  typedef typename SampleVec<T>::type VT;
  constexpr int VEC = SampleVec<T>::VEC;
  constexpr bool FAST = sizeof(T) == 2;                            // (BEAM) bf16 logits: tasu_logprob_topk's __expf / __logf form
  __shared__ int bins[SAMPLE_BINS];
  __shared__ int wt_i[SAMPLE_WAVES];
  __shared__ float wt_f[SAMPLE_WAVES];
  __shared__ int res[4];
  __shared__ float pool_v[SAMPLE_POOL], sort_v[SAMPLE_POOL], id_w[SAMPLE_POOL];
  __shared__ int pool_i[SAMPLE_POOL], sort_i[SAMPLE_POOL];
  __shared__ int s_count, s_surv, s_keep, s_pick;
  __shared__ float s_stat[2];
  __shared__ unsigned hbits[HIST ? SAMPLE_MAX_V / 32 : 1];
  const int row = blockIdx.x, t = threadIdx.x;
  const T* x = logits + (size_t)(BEAM && bd.first ? row / bd.nb : row) * ld;
  const int nchunk = (V + VEC - 1) / VEC;                          // (ld % VEC == 0 and ld >= V: the last chunk lies inside the row)
  if constexpr (HIST) {
    const int nword = (V + 31) / 32;
    for (int i = t; i < nword; i += SAMPLE_THREADS) hbits[i] = 0u;
    __syncthreads();
    const int hl = min(max(hist_len[row], 0), min(hist_ld, SAMPLE_HIST_MAX));
    const int32_t* hr = hist + (size_t)row * hist_ld;
    for (int i = t; i < hl; i += SAMPLE_THREADS) {
      const int c = hr[i];
      if (c >= 0 && c < V) atomicOr(&hbits[c >> 5], 1u << (c & 31));
    }
  }
  if (t == 0) s_count = 0, s_surv = 0;
  __syncthreads();
  // step 0 (BEAM): the row's max and log-sum-exp over all V columns
  float lse_mx = 0.f, lse_lg = 0.f;
  if constexpr (BEAM) {
    float m = -__builtin_inff();
    for (int c = t; c < nchunk; c += SAMPLE_THREADS) {
      const VT xs = *(const VT*)(x + (size_t)c * VEC);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (c * VEC + j < V) m = fmaxf(m, (float)xs[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((t & 63) == 0) wt_f[t >> 6] = m;
    __syncthreads();
    m = wt_f[0];
    for (int i = 1; i < SAMPLE_WAVES; ++i) m = fmaxf(m, wt_f[i]);
    float sum = 0.f;
    for (int c = t; c < nchunk; c += SAMPLE_THREADS) {
      const VT xs = *(const VT*)(x + (size_t)c * VEC);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float v = (float)xs[j];
        if (c * VEC + j < V && v > -__builtin_inff()) sum += FAST ? __expf(v - m) : expf(v - m);
      }
    }
    const float tot = block_scan<float, false>(sum, wt_f);         // (a fixed tree; the last thread holds the row's sum)
    if (t == SAMPLE_THREADS - 1) s_stat[0] = tot;
    __syncthreads();
    lse_mx = m;
    lse_lg = FAST ? __logf(s_stat[0]) : logf(s_stat[0]);
    __syncthreads();
  }
  const int ban0 = n_banned > 0 ? banned[0] : -1, ban1 = n_banned > 1 ? banned[1] : -1;    // the usual case: EOS below min_length
  // steps 1-2 of the distribution for column c holding xv: x'; -inf: not selectable
  auto penalised = [&](float xv, int c) -> float {
    bool ban = c == ban0 || c == ban1;
    for (int b = 2; b < n_banned; ++b) ban |= (banned[b] == c);
    if (ban) return -__builtin_inff();
    float v = xv;
    if constexpr (BEAM) v = FAST ? v - (lse_mx + lse_lg) : (v - lse_mx) - lse_lg;
    if constexpr (HIST) {
      if ((hbits[c >> 5] >> (c & 31)) & 1u) v = v < 0.f ? v * penalty : v / penalty;
    }
    return v > -__builtin_inff() ? v : -__builtin_inff();          // (NaN: not selectable)
  };
  // step 3: s = x' / T
  auto score = [&](float v) -> float {
    v = __fdiv_rn(v, temp);
    return v == 0.f ? 0.f : v;                                     // -0 -> +0: equal floats, equal keys
  };
  float xlo = -__builtin_inff();                                   // columns with x' below it are out of the top k (set after step a)
  // f(s, column) for every selectable column of chunk c whose x' reaches xlo
  auto chunk_scores = [&](int c, auto f) {
    const VT xs = *(const VT*)(x + (size_t)c * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int col = c * VEC + j;
      if (col < V) {
        const float v = penalised((float)xs[j], col);
        if (v > -__builtin_inff() && v >= xlo) {
          const float s = score(v);
          if (s > -__builtin_inff()) f(s, col);
        }
      }
    }
  };
  auto row_scores = [&](auto f) {
    for (int c = t; c < nchunk; c += SAMPLE_THREADS) chunk_scores(c, f);
  };

  // ---- a. tau0 from the per-thread maxima
  float mine = -__builtin_inff();
  for (int c = t; c < nchunk; c += SAMPLE_THREADS) {
    const VT xs = *(const VT*)(x + (size_t)c * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (c * VEC + j < V) mine = fmaxf(mine, penalised((float)xs[j], c * VEC + j));
  }
  if (mine > -__builtin_inff()) mine = score(mine);                // (the division is monotone: the thread's largest s)
  const RadixSel s0 = radix_select(top_k, [&](auto f) { if (mine > -__builtin_inff()) f(order_key(mine)); }, bins, wt_i, res);
  const uint32_t tau0 = s0.total >= top_k ? s0.key : 0u;
  if (tau0 != 0u) {
    const float ts = __uint_as_float((tau0 & 0x80000000u) ? tau0 ^ 0x80000000u : ~tau0);
    const float tt = ts * temp;
    if (fabsf(tt) < __builtin_inff()) xlo = tt - fabsf(tt) * 0x1p-21f - 1e-30f;
  }
  // ---- b. the k-th largest s: over the candidate list in LDS (it aliases the sort buffers), or over the row when it overflows
  float* cand_v = sort_v;
  int* cand_i = sort_i;
  row_scores([&](float s, int col) {
    if (order_key(s) >= tau0) {
      const int slot = atomicAdd(&s_count, 1);
      if (slot < SAMPLE_POOL) cand_v[slot] = s, cand_i[slot] = col;
    }
  });
  __syncthreads();
  const int n_cand = s_count;
  const bool listed = n_cand <= SAMPLE_POOL;                       // (block-uniform)
  const RadixSel sel = listed ? radix_select(top_k, [&](auto f) {
    for (int i = t; i < n_cand; i += SAMPLE_THREADS) f(order_key(cand_v[i]));
  }, bins, wt_i, res) : radix_select(top_k, [&](auto f) {
    row_scores([&](float s, int) {
      const uint32_t key = order_key(s);
      if (key >= tau0) f(key);
    });
  }, bins, wt_i, res);
  if (sel.total == 0) {                                            // nothing selectable (block-uniform)
    if constexpr (BEAM) {
      if (t < bd.K) {
        bd.out_key[(size_t)row * bd.K + t] = -__builtin_inff(), out_val[(size_t)row * bd.K + t] = -__builtin_inff();
        out_idx[(size_t)row * bd.K + t] = SAMPLE_NONE;
      }
      return;
    }
    if (t == 0) {
      out_val[(size_t)row * 2] = -__builtin_inff(), out_idx[(size_t)row * 2] = 0;
      out_val[(size_t)row * 2 + 1] = -__builtin_inff(), out_idx[(size_t)row * 2 + 1] = SAMPLE_NONE;
    }
    return;
  }
  // ---- c. the survivors
  const uint32_t tau = sel.key;
  const bool fits = sel.n_gt + sel.n_eq <= SAMPLE_POOL;
  const int n = fits ? sel.n_gt + sel.n_eq : SAMPLE_POOL;
  if (listed) {                                                    // (then the survivors fit: they are candidates)
    for (int i = t; i < n_cand; i += SAMPLE_THREADS)
      if (order_key(cand_v[i]) >= tau) {
        const int slot = atomicAdd(&s_surv, 1);
        if (slot < SAMPLE_POOL) pool_v[slot] = cand_v[i], pool_i[slot] = cand_i[i];
      }
  } else {
    row_scores([&](float s, int col) {
      const uint32_t key = order_key(s);
      if (key > tau || (fits && key == tau)) {
        const int slot = atomicAdd(&s_surv, 1);
        if (slot < SAMPLE_POOL) pool_v[slot] = s, pool_i[slot] = col;
      }
    });
  }
  if (!listed && !fits) {                                                     // the first ties in token-id order fill the pool (block-uniform)
    int base = sel.n_gt;                                           // (n_gt < top_k <= SAMPLE_POOL)
    for (int c0 = 0; c0 < nchunk && base < SAMPLE_POOL; c0 += SAMPLE_THREADS) {
      const int c = c0 + t;
      unsigned ties = 0u;
      float tv = 0.f;
      if (c < nchunk) chunk_scores(c, [&](float s, int col) {
        if (order_key(s) == tau) ties |= 1u << (col - c * VEC), tv = s;
      });
      const int cnt = __popc(ties);
      const int incl = block_scan<int, false>(cnt, wt_i);
      int pos = base + incl - cnt;
      for (int j = 0; j < VEC; ++j)
        if ((ties >> j) & 1u) {
          if (pos < SAMPLE_POOL) pool_v[pos] = tv, pool_i[pos] = c * VEC + j;
          ++pos;
        }
      if (t == SAMPLE_THREADS - 1) res[0] = incl;
      __syncthreads();
      base += res[0];
      __syncthreads();
    }
  }
  __syncthreads();
  // ---- d. rank sort by (s descending, id ascending), weights, top-p
  if (t < n) {
    const float v = pool_v[t];
    const int id = pool_i[t];
    int rank = 0;
    for (int d = 0; d < n; ++d) {
      const float dv = pool_v[d];
      const int di = pool_i[d];
      rank += (dv > v || (dv == v && di < id)) ? 1 : 0;
    }
    sort_v[rank] = v, sort_i[rank] = id;
  }
  if (t == 0) s_keep = n;
  __syncthreads();
  const float smax = sort_v[0];
  const float w = t < n ? expf(sort_v[t] - smax) : 0.f;
  if (top_p < 1.f) {
    const float sfx = block_scan<float, true>(w, wt_f);            // the mass of ranks >= t: HF's ascending cumulative sum
    if (t == 0) s_stat[0] = sfx;
    __syncthreads();
    const float cut = (1.f - top_p) * s_stat[0];
    if (t >= (BEAM ? 2 : 1) && t < n && sfx <= cut) atomicMin(&s_keep, t);     // (BEAM: min_tokens_to_keep = 2)
    __syncthreads();
  }
  const int n_keep = s_keep;
  if constexpr (BEAM) {
    // ---- e'. the kept entries' accumulated scores and Gumbel keys; the row's K best by (key descending, id ascending)
    float a = -__builtin_inff(), key = -__builtin_inff();
    int id = SAMPLE_NONE;
    if (t < n_keep) {
      id = sort_i[t];
      a = sort_v[t] + bd.run_scores[row];
      const uint64_t kk = (uint64_t)bd.seed[0] ^ ((uint64_t)(uint32_t)bd.ctl[0] * 0x9E3779B97F4A7C15ull);
      const uint64_t z = sample_mix64(kk + ((uint64_t)row * (uint64_t)V + (uint64_t)id) * 0xD1B54A32D192ED03ull);
      const float uu = ((float)(uint32_t)(z >> 41) + 0.5f) * 0x1p-23f;
      key = a + -logf(-logf(uu));
      id_w[t] = key;
    }
    __syncthreads();
    if (t < n_keep) {
      int rank = 0;
      for (int d = 0; d < n_keep; ++d) {
        const float dk = id_w[d];
        rank += (dk > key || (dk == key && sort_i[d] < id)) ? 1 : 0;
      }
      if (rank < bd.K) {
        bd.out_key[(size_t)row * bd.K + rank] = key, out_val[(size_t)row * bd.K + rank] = a;
        out_idx[(size_t)row * bd.K + rank] = min(max(id, 0), V - 1);
      }
    } else if (t < bd.K) {                                         // (ranks n_keep .. K - 1: fewer survivors than K)
      bd.out_key[(size_t)row * bd.K + t] = -__builtin_inff(), out_val[(size_t)row * bd.K + t] = -__builtin_inff();
      out_idx[(size_t)row * bd.K + t] = SAMPLE_NONE;
    }
    return;
  }
  // ---- e. the kept entries in id order, their prefix sums, the pick
  if (t < n_keep) {
    const int id = sort_i[t];
    int rank = 0;
    for (int d = 0; d < n_keep; ++d) rank += sort_i[d] < id ? 1 : 0;
    pool_v[rank] = sort_v[t], pool_i[rank] = id, id_w[rank] = w;
  }
  if (t == 0) s_pick = n_keep - 1;
  __syncthreads();
  const float cum = block_scan<float, false>(t < n_keep ? id_w[t] : 0.f, wt_f);
  if (t == n_keep - 1) s_stat[1] = cum;
  __syncthreads();
  const float Z = s_stat[1];
  const float target = u[row] * Z;
  if (t < n_keep && cum > target) atomicMin(&s_pick, t);
  __syncthreads();
  if (t == 0) {
    const int pick = s_pick;
    out_val[(size_t)row * 2] = (pool_v[pick] - smax) - logf(Z);
    out_idx[(size_t)row * 2] = min(max(pool_i[pick], 0), V - 1);   // (a column id already; the next step indexes the embedding table with it)
    out_val[(size_t)row * 2 + 1] = -__builtin_inff();
    out_idx[(size_t)row * 2 + 1] = SAMPLE_NONE;
  }
}

template <typename T>
int sample_rows_launch(const T* logits, int ld, int M, int V, const float* u, const int32_t* banned, int n_banned, const int32_t* hist,
                       int hist_ld, const int32_t* hist_len, float penalty, float temperature, int top_k, float top_p, float* out_val,
                       int32_t* out_idx, hipStream_t stream) {
  constexpr int VEC = SampleVec<T>::VEC;
  if (!logits || !u || !out_val || !out_idx || M <= 0 || M > SAMPLE_MAX_M || V <= 0 || V > SAMPLE_MAX_V || ld < V || ld % VEC ||
      ((uintptr_t)logits & 15) || n_banned < 0 || (n_banned > 0 && !banned) || top_k < 1 || top_k > SAMPLE_POOL ||
      !(temperature > 0.f) || !(temperature < __builtin_inff()) || !(top_p >= 0.f))
    return TASU_ERR_ARG;
  if (hist) {
    if (!hist_len || hist_ld <= 0 || !(penalty > 0.f)) return TASU_ERR_ARG;
    TASU_LAUNCH((sample_rows_kernel<T, true, false>), dim3(M), dim3(SAMPLE_THREADS), 0, stream, logits, ld, V, u, banned, n_banned, hist, hist_ld,
                hist_len, penalty, temperature, top_k, top_p, out_val, out_idx, BeamDraw{});
    return TASU_OK;
  }
  if (penalty != 1.f) return TASU_ERR_ARG;                         // a penalty needs the history
  TASU_LAUNCH((sample_rows_kernel<T, false, false>), dim3(M), dim3(SAMPLE_THREADS), 0, stream, logits, ld, V, u, banned, n_banned, hist, hist_ld,
              hist_len, penalty, temperature, top_k, top_p, out_val, out_idx, BeamDraw{});
  return TASU_OK;
}

template <typename T>
int beam_sample_rows_launch(const T* logits, int ld, int M, int V, int K, int n_beams, int first, const int64_t* seed, const int32_t* ctl,
                            const float* run_scores, const int32_t* banned, int n_banned, const int32_t* hist, int hist_ld,
                            const int32_t* hist_len, float penalty, float temperature, int top_k, float top_p, float* out_key,
                            float* out_val, int32_t* out_idx, hipStream_t stream) {
  constexpr int VEC = SampleVec<T>::VEC;
  if (!logits || !seed || !ctl || !run_scores || !out_key || !out_val || !out_idx || M <= 0 || M > SAMPLE_MAX_M || V <= 0 ||
      V > SAMPLE_MAX_V || ld < V || ld % VEC || ((uintptr_t)logits & 15) || n_banned < 0 || (n_banned > 0 && !banned) || top_k < 1 ||
      top_k > SAMPLE_POOL || !(temperature > 0.f) || !(temperature < __builtin_inff()) || !(top_p >= 0.f) || K < 1 || K > 32 ||
      n_beams < 1 || M % n_beams || (first != 0 && first != 1))
    return TASU_ERR_ARG;
  if (top_k < 2) top_k = 2;                                        // HF: min_tokens_to_keep = 2 with more than one beam
  const BeamDraw bd{seed, ctl, run_scores, out_key, n_beams, first, K};
  if (hist) {
    if (!hist_len || hist_ld <= 0 || !(penalty > 0.f)) return TASU_ERR_ARG;
    TASU_LAUNCH((sample_rows_kernel<T, true, true>), dim3(M), dim3(SAMPLE_THREADS), 0, stream, logits, ld, V, (const float*)nullptr, banned, n_banned,
                hist, hist_ld, hist_len, penalty, temperature, top_k, top_p, out_val, out_idx, bd);
    return TASU_OK;
  }
  if (penalty != 1.f) return TASU_ERR_ARG;                         // a penalty needs the history
  TASU_LAUNCH((sample_rows_kernel<T, false, true>), dim3(M), dim3(SAMPLE_THREADS), 0, stream, logits, ld, V, (const float*)nullptr, banned, n_banned,
              hist, hist_ld, hist_len, penalty, temperature, top_k, top_p, out_val, out_idx, bd);
  return TASU_OK;
}
}  // namespace

extern "C" int tasu_sample_uniform(const int64_t* seed, const int32_t* counter, int M, float* u, void* stream) {
  if (!seed || !counter || !u || M <= 0 || M > SAMPLE_MAX_M) return TASU_ERR_ARG;
  TASU_LAUNCH(sample_uniform_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, counter, M, u);
  return TASU_OK;
}

extern "C" int tasu_sample_rows(const void* logits, int ld, int M, int V, const float* u, const int32_t* banned, int n_banned,
                                const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, float temperature, int top_k,
                                float top_p, float* out_val, int32_t* out_idx, void* stream) {
  return sample_rows_launch<bf16>((const bf16*)logits, ld, M, V, u, banned, n_banned, hist, hist_ld, hist_len, penalty, temperature, top_k,
                                  top_p, out_val, out_idx, (hipStream_t)stream);
}

extern "C" int tasu_f32_sample_rows(const float* logits, int ld, int M, int V, const float* u, const int32_t* banned, int n_banned,
                                    const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, float temperature, int top_k,
                                    float top_p, float* out_val, int32_t* out_idx, void* stream) {
  return sample_rows_launch<float>(logits, ld, M, V, u, banned, n_banned, hist, hist_ld, hist_len, penalty, temperature, top_k, top_p,
                                   out_val, out_idx, (hipStream_t)stream);
}

extern "C" int tasu_beam_sample_rows(const void* logits, int ld, int M, int V, int K, int n_beams, int first, const int64_t* seed,
                                     const int32_t* ctl, const float* run_scores, const int32_t* banned, int n_banned,
                                     const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, float temperature,
                                     int top_k, float top_p, float* out_key, float* out_val, int32_t* out_idx, void* stream) {
  return beam_sample_rows_launch<bf16>((const bf16*)logits, ld, M, V, K, n_beams, first, seed, ctl, run_scores, banned, n_banned, hist,
                                       hist_ld, hist_len, penalty, temperature, top_k, top_p, out_key, out_val, out_idx,
                                       (hipStream_t)stream);
}

extern "C" int tasu_f32_beam_sample_rows(const float* logits, int ld, int M, int V, int K, int n_beams, int first, const int64_t* seed,
                                         const int32_t* ctl, const float* run_scores, const int32_t* banned, int n_banned,
                                         const int32_t* hist, int hist_ld, const int32_t* hist_len, float penalty, float temperature,
                                         int top_k, float top_p, float* out_key, float* out_val, int32_t* out_idx, void* stream) {
  return beam_sample_rows_launch<float>(logits, ld, M, V, K, n_beams, first, seed, ctl, run_scores, banned, n_banned, hist, hist_ld,
                                        hist_len, penalty, temperature, top_k, top_p, out_key, out_val, out_idx, (hipStream_t)stream);
}
