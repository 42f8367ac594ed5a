// Beam bookkeeping of the device decode loop: tasu_beam_update (one generated position of the beam search) and
// tasu_beam_hist_update (every beam row's token history, for generate(repetition_penalty)).
//
// One generated position of HF ``generate(num_beams = nb, do_sample = False, early_stopping = False)`` (transformers
// generation/utils.py ``_beam_search``; restated in oracle/tasu_oracle.py::beam_search_generate and, vectorised, in
// ps_slm_amd/decode.py::BeamState, which these kernels reproduce decision for decision):
//   candidates  = per-row top-K log-probs (K = 2 nb) + the running score of their beam;
//   top K       by (score desc, beam asc, token asc) -- the order of a flattened [nb * V] top-k;
//   running     = the first nb candidates that neither are EOS nor reach max_new (their score otherwise + NEG);
//   finished    = candidates among the first nb that stop compete with the kept ones on score / len^penalty;
//   done        = no utterance can still improve (HF's heuristic on the best running score) or every candidate stopped.
// Sequences are not copied: every step records (token, parent slot) of the running beams in bp_tok / bp_par
// [step][b][slot], a finished hypothesis keeps (last step, parent slot, last token), and the host walks the back-pointers
// once at the end.  The update also writes the NEXT step's device inputs (token ids, cache source rows for the beam
// reorder, position ids, cache slots, lengths, the EOS ban while cur < min_length), so the whole decode step replays as one
// hipGraph with no host round trip; ctl[0] = positions generated so far, ctl[1] = done (then the kernels are no-ops).
//
// tasu_beam_update_drawn is the same position under generate(do_sample = True, num_beams > 1), HF's beam-search multinomial sampling:
// the rows' K candidates come from tasu_beam_sample_rows (csrc/sample.hip, whose header states the distribution and the draw) with a
// Gumbel key each, the utterance's K are the K LARGEST KEYS in the order (key desc, beam asc, token asc) -- the draw order of sampling
// without replacement in proportion to softmax(accumulated score) -- and everything after that runs on (accumulated score, beam,
// token) in that order, as HF does with the unsorted output of torch.multinomial: the running beams are the best nb non-stopped BY
// SCORE (ties: the earlier slot), and only the first nb slots of the draw may enter the finished heap.
//
// Up to BEAM_MAX_NB beams an utterance's nb * K candidates fit one wave (beam_update_kernel, one launch); up to BEAM_WIDE_MAX_NB
// they take a workgroup (beam_update_wide_kernel + beam_finish_kernel).  The two differ in how the K best are found; what follows
// -- the running set, the finished-hypothesis merge and the unsat test -- is beam_select, one wave's work in both.
#include "common.h"
#include "../../include/tasu_hip.h"

namespace {
constexpr float BEAM_NEG = -1.0e9f;
constexpr int BEAM_MAX_NB = 5;          // nb * 2 nb candidates fit the 64 lanes of a wave
constexpr int BEAM_WIDE_MAX_NB = 16;
constexpr int BEAM_WIDE_THREADS = 2 * BEAM_WIDE_MAX_NB * BEAM_WIDE_MAX_NB;
struct BeamArgs {
  const float* vals;          // [B * nb, K] (first call: [B, K], beams >= 1 absent)
  const int32_t* idx;
  float* run_scores;          // [B, nb]
  float* fin_scores;          // [B, nb]
  int32_t* fin_len;           // [B, nb]
  int32_t* fin_par;           // [B, nb]   parent slot (running set of the previous step) of a kept finished hypothesis
  int32_t* fin_tok;           // [B, nb]   its last token
  int32_t* is_fin;            // [B, nb]
  int32_t* unsat;             // [B]
  int32_t* bp_tok;            // [max_new, B, nb]
  int32_t* bp_par;            // [max_new, B, nb]
  const float* len_pow;       // [max_new + 2]: float32(t ** length_penalty)
  int32_t* ctl;               // [0] cur, [1] done
  int32_t* done_host;         // optional pinned host word mirroring ctl[1]
  const int32_t* valid;       // [B] real (unpadded) prompt length
  int32_t* next_ids;          // [B * nb]
  int32_t* next_src;
  int32_t* next_pos;
  int32_t* next_slot;
  int32_t* next_lens;
  int32_t* banned;            // [1]: eos while the next position is still below min_length, else -1
  int B, nb, max_new, eos, min_length, S, first;
  const float* keys;          // DRAWN: [B * nb, K] the candidates' Gumbel keys (vals then hold ACCUMULATED scores, B * nb rows always)
};

// candidate c = (beam c / K, k-th best of that beam): its score and token
// DRAWN (beam-sample, tasu_beam_update_drawn): the candidate's accumulated score and token as tasu_beam_sample_rows wrote them, and
// its key ck, by which the K best are chosen; a filler (0x7fffffff) becomes token 0 at -inf, inside the embedding table.  Otherwise ck
// is the score itself.
template <bool DRAWN>
__device__ __forceinline__ void beam_candidate(const BeamArgs& p, int b, int c, int K, float& cs, int& ct, float& ck) {
  const int j = c / K, k = c - j * K;
  if constexpr (DRAWN) {
    const size_t o = ((size_t)b * p.nb + j) * K + k;
    ct = p.idx[o];
    const bool real = ct >= 0 && ct != 0x7fffffff;
    cs = real ? p.vals[o] : -__builtin_inff();
    ck = real ? p.keys[o] : -__builtin_inff();
    if (!real) ct = 0;
    return;
  }
  float v = BEAM_NEG;
  ct = 0;
  if (!p.first || j == 0) {
    const size_t row = p.first ? (size_t)b : (size_t)b * p.nb + j;
    v = p.vals[row * K + k];
    ct = p.idx[row * K + k];
  }
  cs = v + p.run_scores[b * p.nb + j];
  ck = cs;
}
// candidate (sd, td) at index d of beam jd precedes candidate (cs, ct) at index c of beam j
__device__ __forceinline__ bool beam_before(float sd, int jd, int td, int d, float cs, int j, int ct, int c) {
  return sd > cs || (sd == cs && (jd < j || (jd == j && (td < ct || (td == ct && d < c)))));
}

// One WAVE, utterance b, once its K best candidates lie in order in top_lp / top_tok / top_beam (LDS, visible to the wave): the
// running beams of the next step with their back-pointers and device inputs, the finished-hypothesis merge, and the test whether a
// running beam can still beat the worst kept hypothesis.  Every selection is a rank computed with wave shuffles -- rank = number of
// entries that precede this one -- so there are no per-thread arrays and no serial scans.  still: the utterance can still improve;
// all_stop: every one of its K best stops.
__device__ __forceinline__ void beam_select(const BeamArgs& p, int b, int lane, int cur, float lp_now, const float* top_lp_s,
                                            const int* top_tok_s, const int* top_beam_s, bool& still, bool& all_stop) {
  const int nb = p.nb, K = 2 * nb;
  // ---- lanes i < K: the K best in order
  const bool is_top = lane < K;
  const float top_lp = is_top ? top_lp_s[lane] : 0.f;
  const int tok = is_top ? top_tok_s[lane] : 0, beam = is_top ? top_beam_s[lane] : 0;
  const bool stop = is_top && (tok == p.eos || cur + 1 >= p.max_new);
  const float run_lp = is_top ? top_lp + (stop ? BEAM_NEG : 0.f) : -__builtin_inff();
  all_stop = __all(!is_top || stop);
  // running beams of the next step: stable top nb of run_lp
  int r_run = 0;
  for (int d = 0; d < K; ++d) {
    const float sd = __shfl(run_lp, d, 64);
    r_run += (sd > run_lp || (sd == run_lp && d < lane)) ? 1 : 0;
  }
  const bool runs = is_top && r_run < nb;
  if (runs) {
    const size_t o = ((size_t)cur * p.B + b) * nb + r_run;
    p.bp_tok[o] = tok;
    p.bp_par[o] = beam;
    const int m = b * nb + r_run;
    p.next_ids[m] = tok;
    p.next_src[m] = b * nb + beam;
    p.next_pos[m] = p.valid[b] + cur;
    p.next_slot[m] = p.S + cur;
    p.next_lens[m] = p.S + cur + 1;
  }
  const float best_run_lp = __shfl(run_lp, __ffsll((long long)__ballot(runs && r_run == 0)) - 1, 64);   // new running score of slot 0
  // ---- finished hypotheses: stable top nb of [kept (lanes 0..nb-1) | new (lanes nb..nb+K-1)]
  const bool unsat = p.unsat[b] != 0;
  const bool is_old = lane < nb, is_new = lane >= nb && lane < nb + K;
  const int src = lane - nb;                             // index into the K best for the new entries
  float m_sc = -__builtin_inff();
  int m_len = 0, m_par = 0, m_tok = 0, m_fin = 0;
  {
    // new entries read the top list through shuffles (lane src holds entry src)
    const float t_lp = __shfl(top_lp, src < 0 ? 0 : src, 64);
    const int t_tok = __shfl(tok, src < 0 ? 0 : src, 64), t_beam = __shfl(beam, src < 0 ? 0 : src, 64);
    const int t_stop = __shfl((int)stop, src < 0 ? 0 : src, 64);
    if (is_old) {
      m_sc = p.fin_scores[b * nb + lane];
      m_len = p.fin_len[b * nb + lane];
      m_par = p.fin_par[b * nb + lane];
      m_tok = p.fin_tok[b * nb + lane];
      m_fin = p.is_fin[b * nb + lane];
    } else if (is_new) {
      const bool just = t_stop && src < nb;
      float sc = t_lp / lp_now;
      sc = sc + (unsat ? 0.f : BEAM_NEG);
      sc = sc + (just ? 0.f : BEAM_NEG);
      m_sc = sc;
      m_len = cur + 1;
      m_par = t_beam;
      m_tok = t_tok;
      m_fin = just ? 1 : 0;
    }
  }
  int r_fin = 0;
  for (int d = 0; d < nb + K; ++d) {
    const float sd = __shfl(m_sc, d, 64);
    r_fin += (sd > m_sc || (sd == m_sc && d < lane)) ? 1 : 0;
  }
  const bool kept = (is_old || is_new) && r_fin < nb;
  // every lane has read its old entry: the wave is converged here, so the writes below cannot overtake those reads
  if (kept) {
    p.fin_scores[b * nb + r_fin] = m_sc;
    p.fin_len[b * nb + r_fin] = m_len;
    p.fin_par[b * nb + r_fin] = m_par;
    p.fin_tok[b * nb + r_fin] = m_tok;
    p.is_fin[b * nb + r_fin] = m_fin;
  }
  if (runs) p.run_scores[b * nb + r_run] = run_lp;
  // ---- can a running beam still beat the worst kept hypothesis?
  float min_fin = kept ? m_sc : __builtin_inff();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) min_fin = fminf(min_fin, __shfl_xor(min_fin, o, 64));
  const float best_run = best_run_lp / lp_now;           // the new cur is cur + 1: the same power
  const bool improve = __any(kept && best_run > (m_fin ? min_fin : BEAM_NEG));
  still = unsat && improve;
}

// The end of a position, one thread: done = no utterance can still improve or every candidate of every utterance stopped.
__device__ __forceinline__ void beam_close_position(const BeamArgs& p, int cur, int unsat_any, int stop_all) {
  const int done = !(unsat_any && !stop_all);
  p.ctl[0] = cur + 1;
  p.ctl[1] = done;
  p.banned[0] = (cur + 1 < p.min_length) ? p.eos : -1;
  if (p.done_host) __hip_atomic_store(p.done_host, done ? cur + 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// nb <= BEAM_MAX_NB.  One WAVE per utterance (16 utterances per pass of a 1024-thread block): lane c < nb * K holds candidate c and
// ranks it against the others with wave shuffles (the first, thread-per-utterance form of this kernel spent 88 us per position in
// scratch-memory loops).
template <bool DRAWN>
__global__ __launch_bounds__(1024) void beam_update_kernel(BeamArgs p) {
  __shared__ int s_unsat_any, s_stop_all;
  __shared__ float s_top_lp[16][2 * BEAM_MAX_NB];
  __shared__ int s_top_tok[16][2 * BEAM_MAX_NB], s_top_beam[16][2 * BEAM_MAX_NB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = p.nb, K = 2 * nb, NC = nb * K;
  const int cur = p.ctl[0];
  if (p.ctl[1]) return;                                   // finished earlier: leave every output as it is
  if (threadIdx.x == 0) {
    s_unsat_any = 0;
    s_stop_all = 1;
  }
  __syncthreads();
  const float lp_now = p.len_pow[cur + 1];
  for (int b = wave; b < p.B; b += 16) {                  // wave-uniform loop
    const int j = lane / K;
    float cs = -__builtin_inff(), ck = -__builtin_inff();
    int ct = 0;
    if (lane < NC) beam_candidate<DRAWN>(p, b, lane, K, cs, ct, ck);
    // ---- top K by (score desc, beam asc, token asc, candidate index asc); DRAWN: by key, the draw order
    int rank = 0;
    for (int d = 0; d < NC; ++d) {
      const float sd = __shfl(ck, d, 64);
      const int td = __shfl(ct, d, 64);
      rank += beam_before(sd, d / K, td, d, ck, j, ct, lane) ? 1 : 0;
    }
    if (lane < NC && rank < K) {
      s_top_lp[wave][rank] = cs;
      s_top_tok[wave][rank] = ct;
      s_top_beam[wave][rank] = j;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bool still, all_stop;
    beam_select(p, b, lane, cur, lp_now, s_top_lp[wave], s_top_tok[wave], s_top_beam[wave], still, all_stop);
    if (lane == 0) {
      p.unsat[b] = still ? 1 : 0;
      if (still) atomicOr(&s_unsat_any, 1);
      if (!all_stop) atomicAnd(&s_stop_all, 0);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) beam_close_position(p, cur, s_unsat_any, s_stop_all);
}

// BEAM_MAX_NB < nb <= BEAM_WIDE_MAX_NB (up to 16 * 32 = 512 candidates): one WORKGROUP per utterance.  Thread c < nb * K holds
// candidate c; the candidates meet in LDS and every thread counts the candidates that precede its own by reading them back (all
// threads read the same address: an LDS broadcast).  The K best then fit one wave (K <= 32, nb + K <= 48), and wave 0 runs
// beam_select on them.  The batch-wide `done` needs every utterance's verdict: a workgroup leaves two bits in its own unsat[b] --
// bit 0 = the utterance can still improve, bit 1 = one of its K best does not stop -- and beam_finish_kernel (one block, the next
// launch on the stream) reduces them, puts unsat[b] back to 0 / 1 and closes the position: no workgroup waits for another, the value
// cannot depend on the order in which they finish, and the state is the call's own (two decodes on two streams do not meet).
template <bool DRAWN>
__global__ __launch_bounds__(BEAM_WIDE_THREADS) void beam_update_wide_kernel(BeamArgs p) {
  __shared__ float s_cs[BEAM_WIDE_THREADS];
  __shared__ int s_ct[BEAM_WIDE_THREADS];
  __shared__ float s_top_lp[2 * BEAM_WIDE_MAX_NB];
  __shared__ int s_top_tok[2 * BEAM_WIDE_MAX_NB], s_top_beam[2 * BEAM_WIDE_MAX_NB];
  const int t = threadIdx.x, b = blockIdx.x;
  const int nb = p.nb, K = 2 * nb, NC = nb * K;
  const int cur = p.ctl[0];
  if (p.ctl[1]) return;                                   // finished earlier: leave every output as it is (block-uniform)
  const float lp_now = p.len_pow[cur + 1];
  const int j = t / K;
  float cs = -__builtin_inff(), ck = -__builtin_inff();
  int ct = 0;
  if (t < NC) beam_candidate<DRAWN>(p, b, t, K, cs, ct, ck);
  s_cs[t] = ck;                                           // (what the candidates are ranked by; DRAWN: the key)
  s_ct[t] = ct;
  __syncthreads();
  // ---- top K by (score desc, beam asc, token asc, candidate index asc)
  if (t < NC) {
    int rank = 0;
    for (int d0 = 0; d0 < NC; d0 += K) {                  // beam jd = d0 / K
      const int jd = d0 / K;
      for (int d = d0; d < d0 + K; ++d) rank += beam_before(s_cs[d], jd, s_ct[d], d, ck, j, ct, t) ? 1 : 0;
    }
    if (rank < K) {
      s_top_lp[rank] = cs;
      s_top_tok[rank] = ct;
      s_top_beam[rank] = j;
    }
  }
  __syncthreads();
  if (t >= 64) return;
  bool still, all_stop;
  beam_select(p, b, t, cur, lp_now, s_top_lp, s_top_tok, s_top_beam, still, all_stop);
  if (t == 0) p.unsat[b] = (still ? 1 : 0) | (all_stop ? 0 : 2);     // (bit 1: for beam_finish_kernel, which takes it out again)
}
__global__ __launch_bounds__(256) void beam_finish_kernel(BeamArgs p) {
  __shared__ int s_unsat_any, s_stop_all;
  const int cur = p.ctl[0];
  if (p.ctl[1]) return;
  if (threadIdx.x == 0) {
    s_unsat_any = 0;
    s_stop_all = 1;
  }
  __syncthreads();
  if ((int)threadIdx.x < p.B) {
    const int f = p.unsat[threadIdx.x];
    p.unsat[threadIdx.x] = f & 1;
    if (f & 1) atomicOr(&s_unsat_any, 1);
    if (f & 2) atomicAnd(&s_stop_all, 0);
  }
  __syncthreads();
  if (threadIdx.x == 0) beam_close_position(p, cur, s_unsat_any, s_stop_all);
}

// The hypothesis history of every beam row after tasu_beam_update: row m's history = its parent's (next_src[m]) + its new token
// (next_ids[m]), IN PLACE, one workgroup per utterance staging its n_beams rows through LDS (a beam's parent is a row of the same
// utterance; the pattern of the cache row index in tasu_decode_step_prologue), so the launch replays in a captured graph with fixed
// pointers.  The rows are staged HIST_COLS positions at a time (16 rows x 2048 ints do not fit the LDS a launch gets by default;
// dst[r, i] = src[parent r, i] for the SAME i: a pass only reads and writes its own columns).  n = ctl[0] = positions generated
// including the one just decided; ctl[1] (done): nothing is read after it, no-op.
constexpr int HIST_MAX = 2048;          // history entries per row (the decode context limit)
constexpr int HIST_COLS = 512;
__global__ __launch_bounds__(256) void beam_hist_update_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ hist_len,
                                                               const int32_t* __restrict__ ctl, const int32_t* __restrict__ next_src,
                                                               const int32_t* __restrict__ next_ids, int nb, int M, int max_new) {
  __shared__ int stage[BEAM_WIDE_MAX_NB * HIST_COLS];
  const int n = ctl[0];
  if (ctl[1] || n < 1 || n > max_new) return;             // (block-uniform)
  const int m0 = blockIdx.x * nb, rows = min(nb, M - m0);
  for (int c0 = 0; c0 < n - 1; c0 += HIST_COLS) {
    const int w = min(HIST_COLS, n - 1 - c0);
    for (int r = 0; r < rows; ++r) {
      int src = next_src[m0 + r];
      if (src < m0 || src >= m0 + rows) src = m0 + r;
      for (int i = threadIdx.x; i < w; i += 256) stage[r * HIST_COLS + i] = hist[(size_t)src * max_new + c0 + i];
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      int32_t* dst = hist + (size_t)(m0 + r) * max_new + c0;
      for (int i = threadIdx.x; i < w; i += 256) dst[i] = stage[r * HIST_COLS + i];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < rows) {
    hist[(size_t)(m0 + threadIdx.x) * max_new + n - 1] = next_ids[m0 + threadIdx.x];
    hist_len[m0 + threadIdx.x] = n;
  }
}
}  // namespace

extern "C" int tasu_beam_update(const float* vals, const int32_t* idx, float* run_scores, float* fin_scores, int32_t* fin_len,
                                int32_t* fin_par, int32_t* fin_tok, int32_t* is_fin, int32_t* unsat, int32_t* bp_tok,
                                int32_t* bp_par, const float* len_pow, int32_t* ctl, int32_t* done_host, const int32_t* valid,
                                int32_t* next_ids, int32_t* next_src, int32_t* next_pos, int32_t* next_slot, int32_t* next_lens,
                                int32_t* banned, int B, int n_beams, int max_new, int eos, int min_length, int S, int first,
                                void* stream) {
  if (!vals || !idx || !run_scores || !fin_scores || !fin_len || !fin_par || !fin_tok || !is_fin || !unsat || !bp_tok || !bp_par ||
      !len_pow || !ctl || !valid || !next_ids || !next_src || !next_pos || !next_slot || !next_lens || !banned)
    return TASU_ERR_ARG;
  if (B <= 0 || B > 256 || n_beams <= 0 || n_beams > BEAM_WIDE_MAX_NB || max_new <= 0 || S <= 0) return TASU_ERR_ARG;
  BeamArgs a{vals, idx, run_scores, fin_scores, fin_len, fin_par, fin_tok, is_fin, unsat, bp_tok, bp_par, len_pow, ctl,
             done_host, valid, next_ids, next_src, next_pos, next_slot, next_lens, banned, B, n_beams, max_new, eos,
             min_length, S, first};
  if (n_beams > BEAM_MAX_NB) {                            // a workgroup per utterance, then the batch-wide done flag
    TASU_LAUNCH(beam_update_wide_kernel<false>, dim3(B), dim3(BEAM_WIDE_THREADS), 0, (hipStream_t)stream, a);
    TASU_LAUNCH(beam_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    return TASU_OK;
  }
  TASU_LAUNCH(beam_update_kernel<false>, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  return TASU_OK;
}

extern "C" int tasu_beam_update_drawn(const float* keys, const float* vals, const int32_t* idx, float* run_scores, float* fin_scores,
                                      int32_t* fin_len, int32_t* fin_par, int32_t* fin_tok, int32_t* is_fin, int32_t* unsat,
                                      int32_t* bp_tok, int32_t* bp_par, const float* len_pow, int32_t* ctl, int32_t* done_host,
                                      const int32_t* valid, int32_t* next_ids, int32_t* next_src, int32_t* next_pos, int32_t* next_slot,
                                      int32_t* next_lens, int32_t* banned, int B, int n_beams, int max_new, int eos, int min_length, int S,
                                      void* stream) {
  if (!keys || !vals || !idx || !run_scores || !fin_scores || !fin_len || !fin_par || !fin_tok || !is_fin || !unsat || !bp_tok ||
      !bp_par || !len_pow || !ctl || !valid || !next_ids || !next_src || !next_pos || !next_slot || !next_lens || !banned)
    return TASU_ERR_ARG;
  if (B <= 0 || B > 256 || n_beams <= 0 || n_beams > BEAM_WIDE_MAX_NB || max_new <= 0 || S <= 0) return TASU_ERR_ARG;
  BeamArgs a{vals, idx, run_scores, fin_scores, fin_len, fin_par, fin_tok, is_fin, unsat, bp_tok, bp_par, len_pow, ctl,
             done_host, valid, next_ids, next_src, next_pos, next_slot, next_lens, banned, B, n_beams, max_new, eos,
             min_length, S, 0, keys};
  if (n_beams > BEAM_MAX_NB) {
    TASU_LAUNCH(beam_update_wide_kernel<true>, dim3(B), dim3(BEAM_WIDE_THREADS), 0, (hipStream_t)stream, a);
    TASU_LAUNCH(beam_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    return TASU_OK;
  }
  TASU_LAUNCH(beam_update_kernel<true>, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  return TASU_OK;
}

extern "C" int tasu_beam_hist_update(int32_t* hist, int32_t* hist_len, const int32_t* ctl, const int32_t* next_src,
                                     const int32_t* next_ids, int B, int n_beams, int max_new, void* stream) {
  if (!hist || !hist_len || !ctl || !next_src || !next_ids || B <= 0 || n_beams <= 0 || n_beams > BEAM_WIDE_MAX_NB || max_new <= 0 ||
      max_new > HIST_MAX)
    return TASU_ERR_ARG;
  TASU_LAUNCH(beam_hist_update_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, hist, hist_len, ctl, next_src, next_ids, n_beams,
              B * n_beams, max_new);
  return TASU_OK;
}
