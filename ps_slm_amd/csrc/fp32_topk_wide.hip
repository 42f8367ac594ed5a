// The column-part stage of tasu_f32_logprob_topk for 16 < k <= 32 (generate(num_beams = 9 .. 16) in fp32 arithmetic): fp32.hip's
// f32_topk_part_kernel with a cap of 128 candidates.  It lives in a file of its own because a kernel added to fp32.hip changes the
// register allocation and scheduling of that file's existing kernels, and the 1..8-beam launches are to stay what they were.
#include "common.h"
#include "../../include/tasu_hip.h"

namespace {
constexpr int F32_TOPK_PARTS = 16, F32_TOPK_MAXC = 10;     // fp32.hip's: the workspace layout of tasu_f32_logprob_topk
// fp32.hip's f32_topk_part_kernel for 16 < k <= 32: the per-thread maxima alone can put 4 k - 3 columns at or above tau, so the cap is 128
// candidates, ranked by as many threads reading LDS instead of by one wave's shuffles; everything else is that kernel, which
// stays as it was for k <= 16 (a fix to one of the two belongs in the other).
constexpr int F32_TOPK_PCAND_WIDE = 128;
__global__ __launch_bounds__(256) void f32_topk_part_wide_kernel(const float* __restrict__ logits, int ld, int V, int k,
                                                                 const int32_t* __restrict__ banned, int n_banned, float* __restrict__ pm,
                                                                 float* __restrict__ ps, float* __restrict__ pv, int32_t* __restrict__ pi) {
  constexpr int PCAND = F32_TOPK_PCAND_WIDE;
  __shared__ float red[4];
  __shared__ float wtau[4];
  __shared__ float bv[4];
  __shared__ int bi[4];
  __shared__ float cand_v[PCAND];
  __shared__ int cand_i[PCAND];
  __shared__ int cand_n;
  const int row = blockIdx.x, part = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* x = logits + (size_t)row * ld;
  const int nv4 = (V + 3) >> 2, per4 = (nv4 + F32_TOPK_PARTS - 1) / F32_TOPK_PARTS;
  const int v0 = part * per4, v1 = min(nv4, v0 + per4);
  auto is_banned = [&](int c) {
    bool ban = false;
    for (int b = 0; b < n_banned; ++b) ban |= banned[b] == c;
    return ban;
  };
  if (t == 0) cand_n = 0;
  f32x4 xs[F32_TOPK_MAXC];
#pragma unroll
  for (int i = 0; i < F32_TOPK_MAXC; ++i) {
    const int c4 = v0 + t + i * 256;
    xs[i] = c4 < v1 ? *(const f32x4*)(x + (size_t)c4 * 4) : f32x4{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c4 * 4 + j >= V) xs[i][j] = -__builtin_inff();         // (columns past V: padding of the leading dimension)
  }
  float m = -__builtin_inff(), msel = -__builtin_inff();
#pragma unroll
  for (int i = 0; i < F32_TOPK_MAXC; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = xs[i][j];
      m = fmaxf(m, v);
      if (v > msel && !is_banned((v0 + t + i * 256) * 4 + j)) msel = v;
    }
  m = block_max<4>(m, red);
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
  for (int i = 0; i < F32_TOPK_MAXC; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = xs[i][j];
      const int c = (v0 + t + i * 256) * 4 + j;
      if (v > -__builtin_inff()) {
        s += expf(v - m);
        if (v >= tau && !is_banned(c)) {
          const int slot = atomicAdd(&cand_n, 1);
          if (slot < PCAND) cand_v[slot] = v, cand_i[slot] = c;
        }
      }
    }
  s = block_sum<4>(s, red);                              // (its barriers also publish the candidates)
  const size_t slot0 = (size_t)row * F32_TOPK_PARTS + part;
  if (t == 0) pm[slot0] = m, ps[slot0] = s;
  const int n_cand = cand_n;
  if (n_cand <= PCAND) {
    if (t < n_cand) {                                      // as many threads as candidates rank them by reading LDS
      const float v = cand_v[t];
      const int id = cand_i[t];
      int rank = 0;
      for (int d = 0; d < n_cand; ++d) rank += (cand_v[d] > v || (cand_v[d] == v && cand_i[d] < id)) ? 1 : 0;
      if (rank < k) pv[slot0 * k + rank] = v, pi[slot0 * k + rank] = id;
    }
    if (t >= n_cand && t < k) pv[slot0 * k + t] = -__builtin_inff(), pi[slot0 * k + t] = 0x7fffffff;
    return;
  }
  // massive ties: k rounds of "the best column after the previous pick" over the registers
  float pvv = __builtin_inff();
  int pii = -1;
  for (int r = 0; r < k; ++r) {
    float best = -__builtin_inff();
    int bid = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < F32_TOPK_MAXC; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = xs[i][j];
        const int c = (v0 + t + i * 256) * 4 + j;
        if (!(v > -__builtin_inff())) continue;
        const bool after = v < pvv || (v == pvv && c > pii);
        if (!after || v < best || (v == best && c > bid)) continue;
        if (!is_banned(c)) best = v, bid = c;
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
    if (t == 0) pv[slot0 * k + r] = bid == 0x7fffffff ? -__builtin_inff() : best, pi[slot0 * k + r] = bid;
    pvv = best, pii = bid;
    if (bid == 0x7fffffff) pvv = -__builtin_inff(), pii = 0x7fffffff;
  }
}
}  // namespace

int tasu_f32_topk_part_wide(const float* logits, int ld, int M, int V, int k, const int32_t* banned, int n_banned, float* pm, float* ps,
                            float* pv, int32_t* pi, hipStream_t stream) {
  TASU_LAUNCH(f32_topk_part_wide_kernel, dim3(M, F32_TOPK_PARTS), dim3(256), 0, stream, logits, ld, V, k, banned, n_banned, pm, ps, pv, pi);
  return TASU_OK;
}
