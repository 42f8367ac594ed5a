// fp32 cross-attention projector (EncoderProjectorCTCCA, Multitask/model/projector.py:104-126) for the fp32 arithmetic mode:
//   out[r, h*dh:(h+1)*dh] = softmax_v(q[r, h] . E[v, h] / denom) . E[:, h]
// over ALL V rows of the LLM's input embedding table E [V, D] (keys and values at once; head h = columns h*dh .. h*dh + dh - 1).
// One fused pass, no [R, V] score matrix: a workgroup (8 waves) owns a tile of 16 RT rows of one head and one contiguous range of
// key tiles (its V-split).  Every key tile of KT rows x dh is staged once in LDS and feeds both products on
// v_mfma_f32_16x16x4_f32: the scores S = Q K^T (then divided by denom), an online softmax (running max / sum, expf), and
// O = alpha O + P K.  Each split writes its partial (m, l, O) to the workspace; f32_ca_merge_kernel combines the splits in
// ascending split order, so a call's bits are fixed by (R, V, D, H) and repeat exactly.  The next key tile's loads are in
// flight (registers) under the current tile's MFMAs.
#include <math.h>
#include <algorithm>
#include "common.h"
#include "../../include/tasu_hip.h"

namespace tasu_f32_ca {

constexpr int NW = 8, NT = 64 * NW;
constexpr int MAX_DH = 512;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Row tile of 16 RT rows, key tile of KT keys, by the head width (LDS: Q, one key tile and the score tile, ~85-108 KiB: one
// 8-wave workgroup per CU = 2 waves per SIMD; the register-staged next tile is the second buffer).
template <int RT, int KT>
struct Cfg {
  static constexpr int ROWS = 16 * RT;
  static constexpr int PAIRS = RT * (KT / 16);                 // 16 x 16 score tiles per key tile
  static constexpr int PPW = PAIRS >= NW ? PAIRS / NW : 1;     // score tiles per wave
  static constexpr int PARTS = PAIRS >= NW ? 1 : NW / PAIRS;   // waves sharing one score tile (a range of the dh contraction each)
  static constexpr int SLD = KT + 4;                           // score tile pitch (conflict-free column reads of 16 rows)
  static constexpr int OPW = 4;                                // O tiles per wave: RT * dh / 16 <= 32 for every served dh
  static constexpr int DH_MAX = MAX_DH / RT;                  // widest head of this configuration
  static constexpr int LPW = KT * DH_MAX / 4 / NT;             // 16-byte pieces of a key tile per thread
  static size_t lds_bytes(int dh) {
    return sizeof(float) * ((size_t)ROWS * (dh + 4) + (size_t)KT * (dh + 4) + (size_t)PARTS * ROWS * SLD + 3 * ROWS);
  }
  // backward: Q and dO tiles, one key tile, the score tile and the dP tile, lse and delta per row (136-151 KiB of the CU's 160)
  static size_t bwd_lds_bytes(int dh) {
    return sizeof(float) * (2 * (size_t)ROWS * (dh + 4) + (size_t)KT * (dh + 4) + 2 * (size_t)PARTS * ROWS * SLD + 2 * ROWS);
  }
};

inline int cfg_of(int dh) { return dh <= 128 ? 0 : (dh <= 256 ? 1 : 2); }
inline int rows_of(int dh) { return dh <= 128 ? 64 : (dh <= 256 ? 32 : 16); }
inline int kt_of(int dh) { return dh <= 256 ? 64 : 32; }

// Splits of the key range: enough workgroups to cover the chip twice, at most 64, every split at least 4 key tiles (never
// empty).  Returns the number of splits; *per = key tiles per split.
inline int plan_splits(int R, int V, int D, int H, int* per) {
  const int dh = D / H, rt = (R + rows_of(dh) - 1) / rows_of(dh), n_tiles = (V + kt_of(dh) - 1) / kt_of(dh);
  const int want = (512 + rt * H - 1) / (rt * H);
  const int s = std::max(1, std::min(std::min(want, 64), n_tiles / 4));
  *per = (n_tiles + s - 1) / s;
  return (n_tiles + *per - 1) / *per;
}

// grid (row tiles, H, splits); ws: O partials [splits][R][D], then (m, l) [splits][R][H][2]
template <int RT, int KT>
__global__ __launch_bounds__(NT) void f32_ca_attn_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ E, int V, int D,
                                                        int dh, float denom, float* __restrict__ ws, int R, int tiles_per_split,
                                                        int n_tiles) {
  using C = Cfg<RT, KT>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ldk = dh + 4;
  float* sQ = lds;                                    // [ROWS][dh + 4]
  float* sK = sQ + C::ROWS * ldk;                     // [KT][dh + 4]
  float* sS = sK + KT * ldk;                          // [PARTS][ROWS][SLD]: scores, then P (part 0)
  float* sM = sS + C::PARTS * C::ROWS * C::SLD;       // running max, running sum, rescale of the current tile
  float* sL = sM + C::ROWS;
  float* sA = sL + C::ROWS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, l16 = lane & 15;
  const int r0 = blockIdx.x * C::ROWS, h = blockIdx.y, z = blockIdx.z, c0 = h * dh;
  const int tile_lo = z * tiles_per_split, tile_hi = min(n_tiles, tile_lo + tiles_per_split);
  const int dq = dh / 4, nh = dh / 16;
  // ---- Q tile (rows >= R zero) and the running statistics
  for (int i = t; i < C::ROWS * dq; i += NT) {
    const int r = i / dq, c = (i - r * dq) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < R) v = *(const f32x4*)(q + (size_t)(r0 + r) * ldq + c0 + c);
    *(f32x4*)&sQ[r * ldk + c] = v;
  }
  if (t < C::ROWS) sM[t] = -INFINITY, sL[t] = 0.f;
  // ---- key tile loader: KT * dh / 4 16-byte pieces, at most LPW per thread; keys >= V are zeros
  f32x4 kr[C::LPW];
  auto load_tile = [&](int tile) {
    const int k0 = tile * KT;
#pragma unroll
    for (int j = 0; j < C::LPW; ++j) {
      const int i = t + j * NT;
      kr[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < KT * dq) {
        const int k = i / dq, c = (i - k * dq) * 4;
        if (k0 + k < V) kr[j] = *(const f32x4*)(E + (size_t)(k0 + k) * D + c0 + c);
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < C::LPW; ++j) {
      const int i = t + j * NT;
      if (i < KT * dq) {
        const int k = i / dq, c = (i - k * dq) * 4;
        *(f32x4*)&sK[k * ldk + c] = kr[j];
      }
    }
  };
  f32x4 o[C::OPW];
#pragma unroll
  for (int j = 0; j < C::OPW; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int n_otiles = RT * nh;
  // score-tile ownership: pair p = (row tile p / (KT / 16), key tile p % (KT / 16)), contraction range of part `part`
  const int part = wave % C::PARTS, pw = wave / C::PARTS;
  const int h_lo = part * nh / C::PARTS, h_hi = (part + 1) * nh / C::PARTS;
  // softmax ownership: ROWS rows over NT threads, TPR threads per row (a power of two inside a wave)
  constexpr int TPR = NT / C::ROWS, KPT = KT / TPR;
  const int srow = t / TPR, sidx = t % TPR;

  if (tile_lo < tile_hi) load_tile(tile_lo);
  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    store_tile();
    __syncthreads();                                                   // (A) key tile and Q in LDS
    if (tile + 1 < tile_hi) load_tile(tile + 1);                       // next tile in flight under this one's MFMAs
    // ---- scores: S[m][key] = sum_d Q[m][d] K[key][d], two accumulators per tile (even / odd 16-column steps)
#pragma unroll
    for (int pp = 0; pp < C::PPW; ++pp) {
      const int p = pw * C::PPW + pp, rt = p / (KT / 16), kt = p % (KT / 16);
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
      const float* kp = sK + (kt * 16 + l16) * ldk + 4 * g;
      const float* qp = sQ + (rt * 16 + l16) * ldk + 4 * g;
      int hh = h_lo;
      for (; hh + 1 < h_hi; hh += 2) {
        const f32x4 fk0 = *(const f32x4*)(kp + hh * 16), fq0 = *(const f32x4*)(qp + hh * 16);
        const f32x4 fk1 = *(const f32x4*)(kp + hh * 16 + 16), fq1 = *(const f32x4*)(qp + hh * 16 + 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) a0 = mfma4(fk0[e], fq0[e], a0), a1 = mfma4(fk1[e], fq1[e], a1);
      }
      if (hh < h_hi) {
        const f32x4 fk0 = *(const f32x4*)(kp + hh * 16), fq0 = *(const f32x4*)(qp + hh * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) a0 = mfma4(fk0[e], fq0[e], a0);
      }
      // lane: row rt*16 + l16, keys kt*16 + 4g .. + 3
      *(f32x4*)&sS[(part * C::ROWS + rt * 16 + l16) * C::SLD + kt * 16 + 4 * g] = a0 + a1;
    }
    __syncthreads();                                                   // (B) scores in LDS
    // ---- online softmax over this tile's keys (the parts' partial sums added in part order)
    {
      const int kbase = tile * KT;
      float s[KPT], mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int k = sidx * KPT + j;
        float v = sS[srow * C::SLD + k];
#pragma unroll
        for (int pt = 1; pt < C::PARTS; ++pt) v += sS[(pt * C::ROWS + srow) * C::SLD + k];
        v = v / denom;                                                 // `/ d ** 0.5` (projector.py:120): a division
        s[j] = kbase + k < V ? v : -INFINITY;
        mx = fmaxf(mx, s[j]);
      }
#pragma unroll
      for (int off = TPR / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      const float m_old = sM[srow], m_new = fmaxf(m_old, mx);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const float p = expf(s[j] - m_new);                           // masked keys: exp(-inf) = 0
        sS[srow * C::SLD + sidx * KPT + j] = p;
        sum += p;
      }
#pragma unroll
      for (int off = 1; off < TPR; off <<= 1) sum += __shfl_xor(sum, off, 64);
      __syncthreads();                                                 // every thread has read m_old
      if (sidx == 0) {
        const float alpha = expf(m_old - m_new);                      // first tile: exp(-inf) = 0
        sA[srow] = alpha;
        sM[srow] = m_new;
        sL[srow] = sL[srow] * alpha + sum;
      }
    }
    __syncthreads();                                                   // (C) P and the rescale factors in LDS
    // ---- O = alpha O + P K: tile j of this wave = (row tile ot / nh, column tile ot % nh)
#pragma unroll
    for (int j = 0; j < C::OPW; ++j) {
      const int ot = wave + j * NW;
      if (ot < n_otiles) {
        const int rt = ot / nh, ct = ot - rt * nh;
        // the tile's contribution summed on its own, then added once: the running O is rounded once per key tile, not once
        // per 4 keys (V = 151,936 keys make thousands of additions into it)
        const float* pp = sS + (rt * 16 + l16) * C::SLD + 4 * g;
        const float* vp = sK + (4 * g) * ldk + ct * 16 + l16;
        f32x4 tp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < KT / 16; ++kh) {
          const f32x4 fp = *(const f32x4*)(pp + kh * 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) tp = mfma4(vp[(kh * 16 + e) * ldk], fp[e], tp);
        }
        o[j] = o[j] * sA[rt * 16 + l16] + tp;
      }
    }
    __syncthreads();                                                   // (D) LDS free for the next tile
  }
  // ---- partials: lane of O tile (rt, ct) holds row rt*16 + l16, columns ct*16 + 4g .. + 3
  float* wo = ws + (size_t)z * R * D;
#pragma unroll
  for (int j = 0; j < C::OPW; ++j) {
    const int ot = wave + j * NW;
    if (ot < n_otiles) {
      const int rt = ot / nh, ct = ot - rt * nh, r = r0 + rt * 16 + l16;
      if (r < R) *(f32x4*)(wo + (size_t)r * D + c0 + ct * 16 + 4 * g) = o[j];
    }
  }
  if (t < C::ROWS && r0 + t < R) {
    float* ml = ws + (size_t)gridDim.z * R * D + (((size_t)z * R + r0 + t) * gridDim.y + h) * 2;
    ml[0] = sM[t];
    ml[1] = sL[t];
  }
}

// out[r, c] = sum_z exp(m_z - M) O_z[r, c] / sum_z exp(m_z - M) l_z, splits in ascending order
// lse (optional): [R, H] = M + log(L), what the backward's P = exp(S - lse) reads; `out` does not depend on it
__global__ __launch_bounds__(256) void f32_ca_merge_kernel(const float* __restrict__ ws, int splits, float* __restrict__ out, int ldo,
                                                          int R, int D, int H, int dh, float* __restrict__ lse) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)R * D) return;
  const int r = (int)(i / D), c = (int)(i - (size_t)r * D), h = c / dh;
  const float* ml = ws + (size_t)splits * R * D;
  float M = -INFINITY;
  for (int z = 0; z < splits; ++z) M = fmaxf(M, ml[(((size_t)z * R + r) * H + h) * 2]);
  float L = 0.f, acc = 0.f;
  for (int z = 0; z < splits; ++z) {
    const float* e = ml + (((size_t)z * R + r) * H + h) * 2;
    const float w = expf(e[0] - M);
    L += e[1] * w;
    acc += ws[((size_t)z * R + r) * D + c] * w;
  }
  out[(size_t)r * ldo + c] = acc / L;
  if (lse && c == h * dh) lse[(size_t)r * H + h] = M + logf(L);
}

// ------------------------------------------------------------------------------------------------------------------ backward
// dq of the same attention (keys = values = the frozen table: the only gradient is the query's).  Same tiling, same V-splits and
// the same key-tile staging as the forward; per key tile, with lse from the forward and delta[r] = sum_c dO[r, c] O[r, c] of the head:
//   S = Q K^T / denom (recomputed),  P = exp(S - lse),  dP = dO K^T,  dS = P (dP - delta) / denom,  dq += dS K
// S and dP come out of one sweep over the key tile in LDS (two accumulator pairs per 16 x 16 tile); dS overwrites S and feeds the
// third product exactly as P feeds O in the forward.  Each split writes its partial dq to the workspace [splits][R][D];
// f32_ca_bwd_merge_kernel adds the splits in ascending order.
template <int RT, int KT>
__global__ __launch_bounds__(NT) void f32_ca_attn_bwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ E, int V, int D,
                                                            int dh, float denom, const float* __restrict__ out, int ldo,
                                                            const float* __restrict__ dout, int lddo, const float* __restrict__ lse,
                                                            float* __restrict__ ws, int R, int tiles_per_split, int n_tiles) {
  using C = Cfg<RT, KT>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int ldk = dh + 4;
  float* sQ = lds;                                    // [ROWS][dh + 4]
  float* sG = sQ + C::ROWS * ldk;                     // [ROWS][dh + 4]: dO
  float* sK = sG + C::ROWS * ldk;                     // [KT][dh + 4]
  float* sS = sK + KT * ldk;                          // [PARTS][ROWS][SLD]: scores, then dS (part 0)
  float* sP = sS + C::PARTS * C::ROWS * C::SLD;       // [PARTS][ROWS][SLD]: dP
  float* sL = sP + C::PARTS * C::ROWS * C::SLD;       // lse, delta per row
  float* sD = sL + C::ROWS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, l16 = lane & 15;
  const int r0 = blockIdx.x * C::ROWS, h = blockIdx.y, z = blockIdx.z, c0 = h * dh;
  const int tile_lo = z * tiles_per_split, tile_hi = min(n_tiles, tile_lo + tiles_per_split);
  const int dq = dh / 4, nh = dh / 16;
  constexpr int TPR = NT / C::ROWS, KPT = KT / TPR;
  const int srow = t / TPR, sidx = t % TPR;
  // ---- Q and dO tiles (rows >= R zero), lse, delta
  for (int i = t; i < C::ROWS * dq; i += NT) {
    const int r = i / dq, c = (i - r * dq) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < R) {
      v = *(const f32x4*)(q + (size_t)(r0 + r) * ldq + c0 + c);
      w = *(const f32x4*)(dout + (size_t)(r0 + r) * lddo + c0 + c);
    }
    *(f32x4*)&sQ[r * ldk + c] = v;
    *(f32x4*)&sG[r * ldk + c] = w;
  }
  {
    float dl = 0.f;
    if (r0 + srow < R)
      for (int c = sidx; c < dh; c += TPR) dl += dout[(size_t)(r0 + srow) * lddo + c0 + c] * out[(size_t)(r0 + srow) * ldo + c0 + c];
#pragma unroll
    for (int off = 1; off < TPR; off <<= 1) dl += __shfl_xor(dl, off, 64);
    if (sidx == 0) {
      sD[srow] = dl;
      sL[srow] = r0 + srow < R ? lse[(size_t)(r0 + srow) * gridDim.y + h] : 0.f;
    }
  }
  f32x4 kr[C::LPW];
  auto load_tile = [&](int tile) {
    const int k0 = tile * KT;
#pragma unroll
    for (int j = 0; j < C::LPW; ++j) {
      const int i = t + j * NT;
      kr[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < KT * dq) {
        const int k = i / dq, c = (i - k * dq) * 4;
        if (k0 + k < V) kr[j] = *(const f32x4*)(E + (size_t)(k0 + k) * D + c0 + c);
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < C::LPW; ++j) {
      const int i = t + j * NT;
      if (i < KT * dq) {
        const int k = i / dq, c = (i - k * dq) * 4;
        *(f32x4*)&sK[k * ldk + c] = kr[j];
      }
    }
  };
  f32x4 o[C::OPW];
#pragma unroll
  for (int j = 0; j < C::OPW; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int n_otiles = RT * nh;
  const int part = wave % C::PARTS, pw = wave / C::PARTS;
  const int h_lo = part * nh / C::PARTS, h_hi = (part + 1) * nh / C::PARTS;

  if (tile_lo < tile_hi) load_tile(tile_lo);
  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    store_tile();
    __syncthreads();                                                   // (A) key tile, Q, dO and the row statistics in LDS
    if (tile + 1 < tile_hi) load_tile(tile + 1);
    // ---- S = Q K^T and dP = dO K^T over the same key fragments
#pragma unroll
    for (int pp = 0; pp < C::PPW; ++pp) {
      const int p = pw * C::PPW + pp, rt = p / (KT / 16), kt = p % (KT / 16);
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
      const float* kp = sK + (kt * 16 + l16) * ldk + 4 * g;
      const float* qp = sQ + (rt * 16 + l16) * ldk + 4 * g;
      const float* gp = sG + (rt * 16 + l16) * ldk + 4 * g;
      int hh = h_lo;
      for (; hh + 1 < h_hi; hh += 2) {
        const f32x4 fk0 = *(const f32x4*)(kp + hh * 16), fq0 = *(const f32x4*)(qp + hh * 16), fg0 = *(const f32x4*)(gp + hh * 16);
        const f32x4 fk1 = *(const f32x4*)(kp + hh * 16 + 16), fq1 = *(const f32x4*)(qp + hh * 16 + 16), fg1 = *(const f32x4*)(gp + hh * 16 + 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a0 = mfma4(fk0[e], fq0[e], a0), a1 = mfma4(fk1[e], fq1[e], a1);
          b0 = mfma4(fk0[e], fg0[e], b0), b1 = mfma4(fk1[e], fg1[e], b1);
        }
      }
      if (hh < h_hi) {
        const f32x4 fk0 = *(const f32x4*)(kp + hh * 16), fq0 = *(const f32x4*)(qp + hh * 16), fg0 = *(const f32x4*)(gp + hh * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) a0 = mfma4(fk0[e], fq0[e], a0), b0 = mfma4(fk0[e], fg0[e], b0);
      }
      const int at = (part * C::ROWS + rt * 16 + l16) * C::SLD + kt * 16 + 4 * g;
      *(f32x4*)&sS[at] = a0 + a1;
      *(f32x4*)&sP[at] = b0 + b1;
    }
    __syncthreads();                                                   // (B) S and dP in LDS
    // ---- dS = P (dP - delta) / denom over this tile's keys (the parts' partial sums added in part order); keys >= V: 0
    {
      const int kbase = tile * KT;
      const float l = sL[srow], dl = sD[srow];
#pragma unroll
      for (int j = 0; j < KPT; ++j) {
        const int k = sidx * KPT + j;
        float v = sS[srow * C::SLD + k], dp = sP[srow * C::SLD + k];
#pragma unroll
        for (int pt = 1; pt < C::PARTS; ++pt) v += sS[(pt * C::ROWS + srow) * C::SLD + k], dp += sP[(pt * C::ROWS + srow) * C::SLD + k];
        v = v / denom;
        sS[srow * C::SLD + k] = kbase + k < V ? expf(v - l) * (dp - dl) / denom : 0.f;
      }
    }
    __syncthreads();                                                   // (C) dS in LDS
    // ---- dq += dS K, the tile's contribution summed on its own and added once (as the forward's O)
#pragma unroll
    for (int j = 0; j < C::OPW; ++j) {
      const int ot = wave + j * NW;
      if (ot < n_otiles) {
        const int rt = ot / nh, ct = ot - rt * nh;
        const float* pp = sS + (rt * 16 + l16) * C::SLD + 4 * g;
        const float* vp = sK + (4 * g) * ldk + ct * 16 + l16;
        f32x4 tp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < KT / 16; ++kh) {
          const f32x4 fp = *(const f32x4*)(pp + kh * 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) tp = mfma4(vp[(kh * 16 + e) * ldk], fp[e], tp);
        }
        o[j] = o[j] + tp;
      }
    }
    __syncthreads();                                                   // (D) LDS free for the next tile
  }
  float* wo = ws + (size_t)z * R * D;
#pragma unroll
  for (int j = 0; j < C::OPW; ++j) {
    const int ot = wave + j * NW;
    if (ot < n_otiles) {
      const int rt = ot / nh, ct = ot - rt * nh, r = r0 + rt * 16 + l16;
      if (r < R) *(f32x4*)(wo + (size_t)r * D + c0 + ct * 16 + 4 * g) = o[j];
    }
  }
}

// dq[r, c] = sum_z ws[z][r][c], splits in ascending order
__global__ __launch_bounds__(256) void f32_ca_bwd_merge_kernel(const float* __restrict__ ws, int splits, float* __restrict__ dq, int lddq,
                                                              int R, int D) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)R * D) return;
  const int r = (int)(i / D), c = (int)(i - (size_t)r * D);
  float acc = 0.f;
  for (int z = 0; z < splits; ++z) acc += ws[((size_t)z * R + r) * D + c];
  dq[(size_t)r * lddq + c] = acc;
}

template <int RT, int KT>
static int launch(const float* q, int ldq, const float* E, int V, int D, int H, float denom, float* ws, int R, int splits, int per,
                  hipStream_t st) {
  using C = Cfg<RT, KT>;
  const int dh = D / H, n_tiles = (V + KT - 1) / KT;
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute((const void*)f32_ca_attn_kernel<RT, KT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)C::lds_bytes(C::DH_MAX)) != hipSuccess)
      return TASU_ERR_LAUNCH;
    attr = true;
  }
  dim3 grid((R + C::ROWS - 1) / C::ROWS, H, splits);
  TASU_LAUNCH((f32_ca_attn_kernel<RT, KT>), grid, dim3(NT), C::lds_bytes(dh), st, q, ldq, E, V, D, dh, denom, ws, R, per, n_tiles);
  return TASU_OK;
}

template <int RT, int KT>
static int launch_bwd(const float* q, int ldq, const float* E, int V, int D, int H, float denom, const float* out, int ldo,
                      const float* dout, int lddo, const float* lse, float* ws, int R, int splits, int per, hipStream_t st) {
  using C = Cfg<RT, KT>;
  const int dh = D / H, n_tiles = (V + KT - 1) / KT;
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute((const void*)f32_ca_attn_bwd_kernel<RT, KT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)C::bwd_lds_bytes(C::DH_MAX)) != hipSuccess)
      return TASU_ERR_LAUNCH;
    attr = true;
  }
  dim3 grid((R + C::ROWS - 1) / C::ROWS, H, splits);
  TASU_LAUNCH((f32_ca_attn_bwd_kernel<RT, KT>), grid, dim3(NT), C::bwd_lds_bytes(dh), st, q, ldq, E, V, D, dh, denom, out, ldo, dout, lddo,
              lse, ws, R, per, n_tiles);
  return TASU_OK;
}

}  // namespace tasu_f32_ca

using namespace tasu_f32_ca;

extern "C" int64_t tasu_f32_ca_workspace_floats(int R, int V, int D, int H) {
  if (R < 1 || V < 1 || H < 1 || D < H || D % H) return -1;
  int per;
  return (int64_t)plan_splits(R, V, D, H, &per) * R * ((int64_t)D + 2 * H);
}

static int ca_forward(const float* q, int ldq, const float* table, int V, int D, int H, float denom, float* out, int ldo, float* lse, int R,
                      float* workspace, int64_t workspace_floats, void* stream) {
  if (!q || !table || !out || !workspace || V < 1 || R < 1 || H < 1 || D < H || D % H) return TASU_ERR_ARG;
  const int dh = D / H;
  if (dh % 16 || dh > MAX_DH || ldq < D || ldo < D || ldq % 4 || !(denom > 0.f) || !isfinite(denom)) return TASU_ERR_ARG;
  if (((uintptr_t)q | (uintptr_t)table | (uintptr_t)workspace) & 15) return TASU_ERR_ARG;
  if ((int64_t)R * D > INT32_MAX || (int64_t)V * D > ((int64_t)1 << 40)) return TASU_ERR_ARG;
  int per;
  const int splits = plan_splits(R, V, D, H, &per);
  if (workspace_floats < tasu_f32_ca_workspace_floats(R, V, D, H)) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (cfg_of(dh)) {
    case 0: rc = launch<4, 64>(q, ldq, table, V, D, H, denom, workspace, R, splits, per, st); break;
    case 1: rc = launch<2, 64>(q, ldq, table, V, D, H, denom, workspace, R, splits, per, st); break;
    default: rc = launch<1, 32>(q, ldq, table, V, D, H, denom, workspace, R, splits, per, st); break;
  }
  if (rc) return rc;
  const size_t n = (size_t)R * D;
  TASU_LAUNCH(f32_ca_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, workspace, splits, out, ldo, R, D, H, dh, lse);
  return TASU_OK;
}

extern "C" int tasu_f32_ca_attn(const float* q, int ldq, const float* table, int V, int D, int H, float denom, float* out, int ldo, int R,
                                float* workspace, int64_t workspace_floats, void* stream) {
  return ca_forward(q, ldq, table, V, D, H, denom, out, ldo, nullptr, R, workspace, workspace_floats, stream);
}

extern "C" int tasu_f32_ca_attn_lse(const float* q, int ldq, const float* table, int V, int D, int H, float denom, float* out, int ldo,
                                    float* lse, int R, float* workspace, int64_t workspace_floats, void* stream) {
  if (!lse) return TASU_ERR_ARG;
  return ca_forward(q, ldq, table, V, D, H, denom, out, ldo, lse, R, workspace, workspace_floats, stream);
}

extern "C" int tasu_f32_ca_attn_bwd(const float* q, int ldq, const float* table, int V, int D, int H, float denom, const float* out, int ldo,
                                    const float* dout, int lddo, const float* lse, float* dq, int lddq, int R, float* workspace,
                                    int64_t workspace_floats, void* stream) {
  if (!q || !table || !out || !dout || !lse || !dq || !workspace || V < 1 || R < 1 || H < 1 || D < H || D % H) return TASU_ERR_ARG;
  const int dh = D / H;
  if (dh % 16 || dh > MAX_DH || ldq < D || ldo < D || lddo < D || lddq < D || ldq % 4 || lddo % 4 || !(denom > 0.f) || !isfinite(denom))
    return TASU_ERR_ARG;
  if (((uintptr_t)q | (uintptr_t)table | (uintptr_t)dout | (uintptr_t)workspace) & 15) return TASU_ERR_ARG;
  if ((int64_t)R * D > INT32_MAX || (int64_t)V * D > ((int64_t)1 << 40)) return TASU_ERR_ARG;
  int per;
  const int splits = plan_splits(R, V, D, H, &per);                   // the forward's splits: [splits][R][D] fits its workspace
  if (workspace_floats < tasu_f32_ca_workspace_floats(R, V, D, H)) return TASU_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (cfg_of(dh)) {
    case 0: rc = launch_bwd<4, 64>(q, ldq, table, V, D, H, denom, out, ldo, dout, lddo, lse, workspace, R, splits, per, st); break;
    case 1: rc = launch_bwd<2, 64>(q, ldq, table, V, D, H, denom, out, ldo, dout, lddo, lse, workspace, R, splits, per, st); break;
    default: rc = launch_bwd<1, 32>(q, ldq, table, V, D, H, denom, out, ldo, dout, lddo, lse, workspace, R, splits, per, st); break;
  }
  if (rc) return rc;
  const size_t n = (size_t)R * D;
  TASU_LAUNCH(f32_ca_bwd_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, workspace, splits, dq, lddq, R, D);
  return TASU_OK;
}
