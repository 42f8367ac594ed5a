"""TEST HELPER (not a test, never shipped): plain float64 restatements of the bf16 NT GEMM of the training step and the prefill --
csrc/gemm.hip (128 x 128 / 128 x 96 tiles, 256 x 192 with the last-arriver split-K), csrc/gemm_pipe.hip (loader-wave tiles,
gate|up + SwiGLU, q|k|v + bias + RoPE, tasu_gemm_nt_bf16_splitk), csrc/gemm_pp.hip (256 x 256, stream-K, K-range slabs, the column
split over two kernels) and the store paths of csrc/gemm_epilogue.h -- on the exact bf16 input values, each with a bound E for
every element it returns.  Nothing is shared with the kernels or with tests/fake_ops.py.  u = 2^-8 (U), RMS_RATIO = 1.5 and the
exact-profile idea are those of tests/decode_ref64.py; `check_within` / `assert_within` are those of tests/attn_ref64.py.

OPERATORS, as csrc/gemm_epilogue.h (store_tile, store_gu_swiglu, store_qkv_rope), csrc/gemm.hip (the tile kernels' epilogue,
tasu_gemm_bias_relu_bf16, tasu_gemm_dswiglu) and csrc/elementwise.hip / common.h compute them; sum = sum_k a_k w_k in fp32:

    mode 0        C = bf16(sum + bias)
    mode 1        C = sum + bias                               (fp32)
    mode 2        C = R + bf16(sum + bias)                     (fp32; the bias is inside the rounding, R outside)
    bias + ReLU   C = bf16(max(sum + bias, 0))                 (fused: max before the one rounding; unfused: tasu_relu_fwd in place
                                                               on bf16(sum + bias) -- the same bits)
    gate|up       gu = bf16(sum);  act = bf16(bf16(silu(g)) t),  g | t = the gate | up halves of gu,  silu(g) = g / (1 + exp(-g))
    q|k|v         x = bf16(sum + bias);  q and k heads: y = bf16(x1 c - x2 s | x2 c + x1 s), (x1, x2) = dims (d, d + 64), c / s the
                  fp32 table;  v heads: x
    dswiglu       d = dact = bf16(sum);  sg = 1 / (1 + exp(-g));  dgu = bf16(d t sg (1 + g (1 - sg))) | bf16(d g sg)   (swiglu_bwd_f:
                  all of it in fp32, ONE rounding per output; g | t the saved gate|up)
    slabs         slab_s = the fp32 sum over the s-th K range;  C = bf16(sum_s slab_s)  (tasu_sum_slabs_bf16: one rounding)

EXACT PROFILE (decode_ref64 (b)): A = integers in [-4, 4], W = integers in [-4, 4] x 2^-s, bias = integers in [-8, 8] x 2^-s, R =
integers in [-64, 64] x 2^-s, s = ceil(log2(6.67 sqrt(K))); max|a| . max|w_int| . K < 2^24 is asserted.  Every fp32 partial sum is
then exact in ANY order -- across waves, K-tile pairs, stream-K ranges, split-K arrivals, slabs and the two-kernel column split --
so the linear epilogues (modes 0 / 1 / 2, bias + ReLU, gu, dact, the v heads, every slab and the slab sum) have ONE right bit
pattern, which float64 gives: the check is torch.equal.  An fp32 partial that went through bf16 on its way (sk_partial, the
256 x 192 last arriver, tasu_sum_slabs_bf16) cannot keep those bits: 46 % of the sums need more than 8 bits at K = 8960, over half from K = 16384.
The non-linear epilogues get exact accumulations as input; their E bounds their own rounding points only:

    SwiGLU       E = (2u + u^2 + 2^-20) |silu(g) t|            -- decode_ref64's bound: store_gu_swiglu has the decode kernels'
                 rounding points (bf16(sum) twice, bf16(silu), bf16(product), silu_f of common.h).  2^-20 covers silu_f's
                 (2|g| + 6) 2^-24 (below) and the fp32 product for |g| <= 5, which `reference` asserts.
    bias + RoPE  E = u |y| + 2^-22 (|x1 c| + |x2 s|)           -- decode_ref64's bound: the OUT_QKV_ROPE epilogue rounds x to bf16
                 before the rotation and runs rope_pair_f of common.h (one rounded product, one FMA), as rope.hip does.
    dswiglu      with a1 = (2|g| + 6) 2^-24 the relative error of sg (__expf(-g) = exp2(-g log2 e): the scaled argument carries
                 2 |g| 2^-24 relative in the result, the instruction 2 ulp; the addition 1 ulp; the division 2.5 ulp), f = 1 + g (1 - sg):
                     E_f  = |g| (sg a1 + 2^-24) + 2^-23 (1 + |g| (1 - sg))      (1 - sg, the product, the addition)
                     E_dg = u |dg| + |d t| sg (a1 |f| + E_f) + 2^-22 |dg|       (three products, second order)
                     E_du = (u + a1 + 2^-22) |du|
                 E_f is an ABSOLUTE bound because f cancels near g = -1.28, where u |dg| alone would demand more than fp32 gives.
GEMM_LIMIT = 1.0: every fp32 allowance is inside E, nothing is left to a factor.

N(0, 1) PROFILE (K <= 512): A ~ N(0, 1), W ~ N(0, 1 / K), bias ~ N(0, 1), R ~ N(0, 1), the inputs of tests/test_gpu_ops.py.  With
F = (K + 2) 2^-24 (sum_k |a_k w_k| + |bias|) the rigorous first-order bound of the fp32 accumulation in any order (K products exact
in fp32, K - 1 additions, the bias, the store), z = sum + bias:

    mode 0, ReLU, gu, dact, v, slab sum    E = u (|z| + F) + F         (ReLU: max is 1-Lipschitz)
    mode 1, a slab                         E = F
    mode 2                                 E = u (|z| + F) + F + 2^-24 (|R| + |z| + F)     (the fp32 addition of R)

F stays below 2 % of u |z| at |z| ~ 1, K = 512.  Second check: rms(err / (u |c|)) over |c| >= 2^-6 at most RMS_RATIO x the torch
double's on the same inputs (nearest 0.29 ulp, truncation 0.58 ulp).  The non-linear outputs (act, q | k, dgu) are held to the
second check only on this profile -- their per-element teeth are in the exact profile.  fp32 mode is held to F only.

GUARDS.  A, W, the saved gate|up and the rotary tables are allocated with 256 rows (the tallest tile) beyond M / N (and, on some
cases, lda = ldb = K + 8), bias with 256 elements beyond N, R like C: all NaN outside the operand.  C (and gu, act, dgu, the
slabs) has two guard rows, guard columns up to ldc, `coff` elements in front and 8 behind, and holds a sentinel bit pattern
everywhere before the launch: `OutBuf.check` requires the sentinel bit for bit outside [M, N] and no NaN inside.

The module also holds the case lists the CPU and the GPU file share (CASES), an independent restatement of the gate|up policy
(gu_route, which tests/test_gemm_ref64_cpu.py holds to tasu_gemm_gate_up_plan) and the facts of a stream-K schedule (streamk_facts)."""
import collections
import ctypes
import math

import numpy as np
import torch

from attn_ref64 import Check, assert_within, check_within  # noqa: F401
from decode_ref64 import RMS_RATIO, U, assert_bits, assert_gemm_within, check_gemm, exact_shift, rms_ulp  # noqa: F401

HD = 128
GEMM_LIMIT = 1.0
F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
NAN = float("nan")
CUS = 256                                                        # MI355X; tasu_gemm_plan's default without a device
PP, PP_P128, PP_P192, SK, P128, P192, P96, SPLITK, TILES = range(1, 10)      # TASU_GEMM_PLAN_* of include/tasu_hip.h
PLAN_NAMES = {PP: "PP256", PP_P128: "PP256_PLUS_PIPE128", PP_P192: "PP256_PLUS_PIPE192", SK: "PP256_STREAMK", P128: "PIPE128",
              P192: "PIPE192", P96: "PIPE96", SPLITK: "TILE192_SPLITK", TILES: "TILES"}

# op:   plain | relu | swiglu | qkv | dswiglu | splitk | slabs        (N: output columns; swiglu / dswiglu: I; qkv: (H + 2G) 128)
# via:  plain: policy | pp256 | pipe128 | pipe192 | pipe96 | streamk;  swiglu: the route gu_route names;  others: policy
# pad:  ldc = N + pad;  coff / roff: C / R start that many elements into their buffer;  ldx: lda = ldb = K + ldx
# n01:  the case also runs the N(0, 1) profile;  plan: the TASU_GEMM_PLAN_* value the dispatcher must give (None: not dispatched)
Case = collections.namedtuple("Case", "op via M N K mode bias H G ks pad coff roff ldx n01 plan why")


def _c(op, via, M, N, K, mode=0, bias=False, H=0, G=0, ks=0, pad=0, coff=0, roff=0, ldx=0, n01=None, plan=None, why=""):
    if n01 is None:
        n01 = K <= 512 and M * N <= 1 << 21
    assert not n01 or K <= 512
    return Case(op, via, M, N, K, mode, bias, H, G, ks, pad, coff, roff, ldx, n01, plan, why)


def _modes(via, M, N, K, plan=None, why="", **kw):
    """one case per public mode; the bias alternates"""
    return [_c("plain", via, M, N, K, mode=m, bias=(m != 1) if kw.get("flip") is None else (m == 1), plan=plan, why=why,
               **{k: v for k, v in kw.items() if k != "flip"}) for m in (0, 1, 2)]


# ---- every plan of the dispatcher (ops.gemm with the workspace), the smallest shapes that reach it on 256 CUs.  plan_nt
# (csrc/gemm_dispatch.h): M <= 64 -> the 128-row tiles, pick_bn: 96 wide where ceil(N / 96) / 1.08 > ceil(N / 128), else 128 wide.  Above, the
# cost per tile round is 32768 (256 x 128), 28577 (128 x 192), 30720 (256 x 96), 52012 (256 x 256): one-round grids take 128 x 192;
# 256 x 128 needs ceil(M / 128) ceil(N / 192) > 256 >= ceil(M / 256) ceil(N / 128); 256 x 96 wins only on a tall single column
# (ceil(M / 256) <= 256 < ceil(M / 128)); whole 256 x 256 tiles need one round of them (52012) under two of the others; the column
# split needs three rounds of 256 x 256 (513 .. 640 tiles) against five and six of the small tiles, the tail's tile then picks the
# second kernel (tail <= 1536 columns: 128 x 192, above: 256 x 128); stream-K: fewer tiles than CUs with tiles . K / 128 >= 8 . 256;
# the 256 x 192 split-K: M > 128, fewer than 128 tiles of 256 x 96, K >= 16384, no stream-K plan.  plan_ksplit is 8 on every shape
# under a few hundred MB (2 needs 86+ tiles of 256 x 192 and fewer than 128 of 256 x 96: N <= 96, M >= 22016 at K = 16384).
PLAN_CASES = [
    _c("plain", "policy", 1, 40, 64, mode=1, bias=True, plan=TILES, why="M = 1, N < a tile, no multiple of 16; pick_bn 128"),
    _c("plain", "policy", 64, 203, 192, mode=0, bias=True, plan=TILES, why="pick_bn 96; ldc = N odd"),
    _c("plain", "policy", 17, 90, 128, mode=2, plan=TILES, why="pick_bn 128"),
    _c("plain", "policy", 50, 520, 256, mode=0, pad=8, coff=4, plan=TILES, why="pick_bn 96, C 8-byte aligned"),
    _c("plain", "policy", 32900, 40, 128, mode=0, bias=True, plan=P96, why="129 tiles of 256 x 96 against 258 of 128 x 192"),
    _c("plain", "policy", 2000, 3190, 256, mode=2, plan=P128, why="200 tiles of 256 x 128 against 272 of 128 x 192"),
    _c("plain", "policy", 300, 203, 128, mode=1, bias=True, pad=5, plan=P192, why="one round"),
    _c("plain", "policy", 2040, 4200, 256, mode=0, bias=True, plan=PP, why="136 tiles of 256 x 256 against two rounds of the others"),
    _c("plain", "policy", 3841, 9900, 256, mode=0, plan=PP_P128, why="624 tiles: 2 rounds + 1708 columns"),
    _c("plain", "policy", 3841, 8200, 256, mode=0, bias=True, plan=PP_P192, why="528 tiles: 2 rounds + 8 columns"),
    _c("plain", "policy", 1000, 1000, 16384, mode=0, bias=True, plan=SK, why="16 tiles x 128 pairs: 16 ranges of 8 pairs per tile"),
    _c("plain", "policy", 1000, 1000, 16384, mode=1, plan=SK, why="fp32 output through sk_partial"),
    _c("plain", "policy", 300, 200, 16384, mode=0, bias=True, plan=SPLITK, why="4 tiles of 256 x 192, 8 arrivals each"),
    _c("plain", "policy", 300, 200, 16384, mode=1, pad=3, plan=SPLITK, why="fp32 output through the last arriver"),
    _c("plain", "policy", 300, 200, 17920, mode=2, bias=True, plan=SPLITK, why="35 K-steps per arrival"),
]

# ---- every named kernel (ops.gemm_on) x every public mode x every store path of store_tile, at 2 x 3 / 2 x 5 / 3 x 3 / 2 x 6
# tiles with edges in both directions: the interior fast path and the edge path (pad 56: ldc = 576 keeps 16-byte rows); ldc no
# multiple of 8 / 4 (pad 3); C 8 bytes into its buffer (4 bf16 / 2 fp32 elements); R 2 elements (8 bytes) into its buffer; N no
# multiple of 4.
KERNEL_CASES = []
for _k in ("pp256", "pipe128", "pipe192", "pipe96"):
    KERNEL_CASES += _modes(_k, 300, 520, 256, pad=56, why="interior + edge tiles, 16-byte rows")
    KERNEL_CASES += _modes(_k, 300, 520, 256, pad=3, flip=True, why="ldc = 523")
    KERNEL_CASES += [c._replace(coff=4 if c.mode == 0 else 2)                                     # 8 bytes in either element size
                     for c in _modes(_k, 300, 520, 256, pad=8, why="C 8- but not 16-byte aligned")]
    KERNEL_CASES += _modes(_k, 300, 519, 256, pad=9, flip=True, why="N no multiple of 4 (mode 2: off WIDE_RESID)")
    KERNEL_CASES.append(_c("plain", _k, 300, 520, 256, mode=2, bias=True, pad=56, roff=2, why="R not 16-byte aligned"))
    KERNEL_CASES.append(_c("plain", _k, 265, 136, 256, mode=0, bias=True, ldx=8, why="lda = ldb = K + 8; 9 rows / 8 columns in the edge tiles"))
KERNEL_CASES += [
    _c("plain", "pipe128", 300, 203, 64, mode=0, bias=True, why="one K-tile"),
    _c("plain", "pipe192", 130, 203, 192, mode=2, ldx=8, why="three K-tiles: an odd count"),
    _c("plain", "pipe96", 257, 100, 128, mode=1, bias=True, why="one row in the second tile"),
    _c("plain", "pp256", 1290, 10760, 384, mode=0, bias=True, n01=False, why="258 tiles: two workgroups' streams cross a tile boundary, 6 K-tiles"),
    _c("plain", "pp256", 300, 520, 8960, mode=1, bias=True, why="140 K-tiles, fp32 output"),
]

# ---- stream-K (ops.gemm_streamk: tasu_gemm_nt_bf16_streamk, sk_plan with max_rem = 1), shapes chosen from tasu_streamk_schedule
# (tests/test_gemm_ref64_cpu.py asserts what each comment names)
STREAMK_CASES = (
    _modes("streamk", 1000, 1000, 16384, why="16 tiles x 128 pairs: every tile cut into 16 ranges, owner + 15 producers") +
    _modes("streamk", 1270, 700, 17920, why="15 tiles x 140 pairs on 256 workgroups: 8.2 pairs per range, ends snapped") +
    _modes("streamk", 2000, 2040, 4096, why="64 tiles x 32 pairs: 4 ranges per tile") +
    [_c("plain", "streamk", 4090, 4600, 1024, mode=0, bias=True, why="288 tiles x 8 pairs: rem + G tiles cut, whole, owner and producer items"),
     _c("plain", "streamk", 4090, 4600, 1024, mode=1, why="... fp32 output"),
     _c("plain", "streamk", 3841, 8200, 1024, mode=0, why="528 tiles x 8 pairs: 272 tiles cut, then 256 whole tiles dealt round-robin: a "
                                                           "workgroup's stream-K items are followed by a whole tile")])

# ---- K-range slabs: tasu_gemm_nt_bf16_splitk (128 x 192 tiles, ksplit <= 16) and tasu_gemm_nt_bf16_slabs (256 x 256 tiles,
# K / ksplit >= 256), two tile rows and columns with edges; each slab, then tasu_sum_slabs_bf16
SLAB_CASES = [_c("splitk", "policy", 200, 300, 128, ks=1), _c("splitk", "policy", 200, 300, 384, ks=3), _c("splitk", "policy", 200, 300, 1024, ks=16),
              _c("splitk", "policy", 200, 300, 9216, ks=16, ldx=8, why="9 K-tiles per slab"),
              _c("slabs", "policy", 300, 520, 256, ks=1), _c("slabs", "policy", 300, 520, 768, ks=3), _c("slabs", "policy", 300, 520, 4096, ks=16),
              _c("slabs", "policy", 300, 520, 8960, ks=5, why="the decoder's 5 x 1792")]


def gu_route(M, I, K, have_ws=True, cus=CUS):
    """tasu_gemm_gate_up_swiglu_ws's tile policy (plan_gate_up, csrc/gemm_dispatch.h), restated: 'pipe' (256 x 128 loader-wave tiles), 'pp' (whole
    256 x 256 tiles), 'pp+pipe' (whole rounds of 256 x 256 + the remaining columns on 256 x 128 in a second launch) or 'pp-sk' (256 x 256
    tiles cut along K).  In units of a 256 x 256 round: c128 = rounds(tm ceil(I / 64)) / 2, c256_whole = rounds(tm tn) / 1.26,
    c256_sk = tm tn / cus / 1.26 + 1e8 / K / 52012 where sk_plan(tm tn, K / 128, cus, max_rem = 0) > 0."""
    if I % 128 or K < 256 or K % 128:
        return "pipe"
    tm, tn = -(-M // 256), -(-I // 128)
    rounds = lambda t: float(-(-t // cus))
    c128 = rounds(tm * -(-I // 64)) * 0.5
    T, P = tm * tn, K // 128
    sk = have_ws and T % cus != 0 and T < cus and T * P // cus >= 8 and (4 * T <= cus or (4 * T <= 3 * cus and (16 * T) % cus == 0))
    whole = rounds(T) / 1.26
    c_sk = (T / cus) / 1.26 + 1.0e8 / K / 52012.0 if sk else 1e30
    if min(c_sk, whole) >= c128:
        return "pipe"
    if c_sk < whole:
        return "pp-sk"
    full = T // cus
    tn_main = full * cus // tm
    if full >= 1 and 0 < tn_main < tn and full / 1.26 + rounds(tm * (tn - tn_main) * 2) * 0.5 + 0.05 < whole:
        return "pp+pipe"
    return "pp"


GU_PLAN = {"pipe": 1, "pp": 2, "pp+pipe": 3, "pp-sk": 4}       # TASU_GEMM_GU_PLAN_* (include/tasu_hip.h): tasu_gemm_gate_up_plan


# ---- gate|up + SwiGLU.  pp: rounds(tm tn) / 1.26 < rounds(tm ceil(I / 64)) / 2 first holds at one round against two: two tile rows,
# I = 65 x 128.  pp+pipe: three rounds of 256 x 256 (513 .. 640 tiles) against five of 256 x 128, a tail of at most 128 tiles: two tile
# rows, I = 257 x 128.  pp-sk: fewer tiles than CUs, tiles . K / 128 >= 8 . 256 and 4 tiles <= CUs: 16 tiles behind K = 16384.
SWIGLU_CASES = [
    _c("swiglu", "pipe", 300, 200, 128, why="I % 8 == 0, not of 128: paired 16-byte stores, interior + edge"),
    _c("swiglu", "pipe", 265, 196, 256, why="I % 8 == 4: the 8-byte store path"),
    _c("swiglu", "pipe", 300, 200, 128, coff=4, why="gu and act 8- but not 16-byte aligned"),
    _c("swiglu", "pipe", 300, 256, 256, pad=64, why="the _ld form: act inside a wider buffer"),
    _c("swiglu", "pp", 300, 8320, 256, n01=False, why="130 tiles of 256 x 256 against 260 of 256 x 128"),
    _c("swiglu", "pp", 300, 8320, 256, n01=False, pad=8, coff=4, why="... _ld form, 8-byte aligned"),
    _c("swiglu", "pp+pipe", 300, 32896, 256, n01=False, why="514 tiles: 2 rounds + 128 tiles of 256 x 128"),
    _c("swiglu", "pp-sk", 500, 1024, 16384, why="16 tiles x 128 pairs cut along K"),
]

# ---- q|k|v + bias + RoPE (tasu_gemm_qkv_rope: 256 x 128 tiles, one head per tile column); M = 265: 9 rows in the last tile
QKV_CASES = [_c("qkv", "policy", 265, 4 * HD, 128, bias=True, H=2, G=1), _c("qkv", "policy", 265, 4 * HD, 256, bias=False, H=2, G=1),
             _c("qkv", "policy", 265, 16 * HD, 128, bias=True, H=12, G=2), _c("qkv", "policy", 100, 16 * HD, 64, bias=False, H=12, G=2),
             _c("qkv", "policy", 265, 36 * HD, 128, bias=True, H=28, G=4), _c("qkv", "policy", 521, 36 * HD, 64, bias=False, H=28, G=4, n01=False)]

# ---- dswiglu (the dispatcher's GEMM into dact + tasu_swiglu_bwd) and bias + ReLU (fused into the dispatcher's kernels above 64
# rows; at most 64 rows: the tile kernels + tasu_relu_fwd in place, ldc == N)
DSWIGLU_CASES = [_c("dswiglu", "policy", 300, 200, 128, plan=P192, why="loader waves"),
                 _c("dswiglu", "policy", 2040, 4200, 256, plan=PP, n01=False, why="256 x 256"),
                 _c("dswiglu", "policy", 50, 200, 128, plan=TILES, why="M <= 128: the tile kernels")]
RELU_CASES = [_c("relu", "policy", 300, 203, 128, bias=True, pad=5, plan=P192, why="loader waves, fused, edge path"),
              _c("relu", "policy", 300, 520, 256, bias=True, pad=56, plan=P192, why="loader waves, fused, paired stores"),
              _c("relu", "policy", 2040, 4200, 256, bias=True, plan=PP, n01=False, why="256 x 256, fused"),
              _c("relu", "policy", 50, 203, 128, bias=True, plan=TILES, why="unfused: tasu_relu_fwd in place, M N % 8 = 6")]

CASES = PLAN_CASES + KERNEL_CASES + STREAMK_CASES + SLAB_CASES + SWIGLU_CASES + QKV_CASES + DSWIGLU_CASES + RELU_CASES
FAMILY = {"plain": "gemm", "relu": "bias+relu", "swiglu": "gate|up+swiglu", "qkv": "qkv+rope", "dswiglu": "dswiglu", "splitk": "splitk",
          "slabs": "slabs"}


def case_id(c):
    s = f"{c.op}-{c.via}-{c.M}x{c.N}x{c.K}-m{c.mode}{'b' if c.bias else ''}"
    for name, v in (("ks", c.ks), ("pad", c.pad), ("coff", c.coff), ("roff", c.roff), ("ldx", c.ldx)):
        if v:
            s += f"-{name}{v}"
    if c.op == "qkv":
        s += f"-H{c.H}G{c.G}"
    return s


def needs_workspace(c):
    """the case goes through the stream-K flags / the split-K counters: run twice, equal bits, workspace words zero afterwards"""
    return c.via in ("streamk", "pp-sk") or c.plan in (SK, SPLITK) or c.op in ("splitk", "slabs")


# ================================================================================================ stream-K schedule facts
def streamk_facts(lib, tiles, pairs, grid=CUS):
    """tasu_streamk_schedule (host code of the kernel's own PpSchedule) for `tiles` tiles of `pairs` K-tile pairs:
    dict(cut = tiles cut along K, roles = {0 whole, 1 producer, 2 owner} met, max_ranges = most ranges one tile is cut into,
    snapped = a range end differs from floor(w units / grid), i.e. PpSchedule::ub moved it to a tile boundary,
    whole_after_cut = a workgroup's stream-K items are followed by a round-robin whole tile)."""
    max_items = 16
    items = np.full((grid, max_items, 4), -1, dtype=np.int32)
    counts = np.zeros(grid, dtype=np.int32)
    cut = lib.tasu_streamk_schedule(tiles, pairs, grid, items.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p), max_items)
    roles, ranges = set(), collections.Counter()
    starts = set()
    whole_after_cut = False
    for w in range(grid):
        for i in range(counts[w]):
            tile, k0, nk, kind = (int(v) for v in items[w, i])
            roles.add(kind)
            whole_after_cut |= i > 0 and tile < tiles - cut and int(items[w, 0, 0]) >= tiles - cut
            if tile >= tiles - cut:
                ranges[tile] += 1
                if i == 0:
                    starts.add((w, (tile - (tiles - cut)) * pairs + k0 // 2))
    units = cut * pairs
    snapped = any(u != w * units // grid for w, u in starts)
    return dict(cut=cut, roles=roles, max_ranges=max(ranges.values()) if ranges else 0, snapped=snapped, whole_after_cut=whole_after_cut)


# ================================================================================================ buffers
def sentinel(n, dtype):
    """n elements of a recognisable finite bit pattern (neighbours differ)"""
    i = torch.arange(n, dtype=torch.int64)
    if dtype == BF:
        return (0x4000 | ((i * 73 + 5) & 0x0FFF)).to(torch.int16).view(BF)
    return (0x40000000 | ((i * 2654435761 + 12345) & 0x0FFFFFFF)).to(torch.int32).view(F32)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


class OutBuf:
    """An output matrix [M, N] with leading dimension ld inside a flat buffer: `off` elements in front, 2 guard rows, guard columns
    up to ld, 8 elements behind; all sentinel.  `view(flat)`: the [M + 2, ld] matrix inside `flat` (the CPU buffer or a device copy
    of it); `check(flat)`: the [M, N] result, after asserting that everything else kept the sentinel's bits and no result is NaN."""

    def __init__(self, M, N, ld, dtype, off=0):
        assert ld >= N
        self.M, self.N, self.ld, self.off, self.dtype = M, N, ld, off, dtype
        self.flat = sentinel(off + (M + 2) * ld + 8, dtype)

    def view(self, flat=None):
        flat = self.flat if flat is None else flat
        return flat[self.off:self.off + (self.M + 2) * self.ld].view(self.M + 2, self.ld)

    def check(self, flat, what):
        flat = flat.cpu()
        inside = torch.zeros(flat.numel(), dtype=torch.bool)
        self.view(inside)[:self.M, :self.N] = True
        changed = (_bits(flat) != _bits(self.flat)) & ~inside
        if bool(changed.any()):
            i = int(torch.nonzero(changed)[0]) - self.off
            where = f"row {i // self.ld}, column {i % self.ld}" if i >= 0 else f"{-i} elements in front of C"
            raise AssertionError(f"{what}: {int(changed.sum())} elements outside [M = {self.M}, N = {self.N}] (ld {self.ld}) were written, "
                                 f"the first at {where}")
        got = self.view(flat)[:self.M, :self.N]
        assert not bool(torch.isnan(got).any()), f"{what}: NaN inside [M, N]: an operand guard was read"
        return got


GUARD = 256                                                      # NaN rows behind every operand: the tallest tile


def guarded(t, ldx=0):
    """operand [rows, cols] -> [rows + GUARD, cols + ldx] with NaN in the guard rows and the lda gap"""
    out = torch.full((t.shape[0] + GUARD, t.shape[1] + ldx), NAN, dtype=t.dtype)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def guarded_vec(t):
    return torch.cat([t, torch.full((GUARD,), NAN, dtype=t.dtype)])


def rope_table(M):
    """the fp32 rotary table of positions 0 .. M - 1 (theta 1e6, 64 frequencies)"""
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=F32) / HD))
    ang = torch.arange(M, dtype=F32)[:, None] * inv[None]
    return ang.cos(), ang.sin()


def make_inputs(c, profile):
    """Seeded inputs of a case, profile "exact" or "n01".  dict: a [M + GUARD, K + ldx], w [rows + GUARD, K + ldx] (rows = N; swiglu:
    2 N, gate rows first), bias [N + GUARD] / None, resid: the flat fp32 buffer of R (its matrix: resid_buf.view(resid)) / None, gu
    (dswiglu: the saved gate|up [M + GUARD, 2 N] bf16, N(0, 1)), cos / sin [M + GUARD, 64]; the guards are NaN."""
    M, N, K = c.M, c.N, c.K
    rows = 2 * N if c.op == "swiglu" else N
    gen = torch.Generator().manual_seed(11 * N + 3 * K + M + 1000 * c.mode)
    ri = lambda lo, hi, *sh: torch.randint(lo, hi + 1, sh, generator=gen).to(F32)
    d = dict(profile=profile, bias=None, resid=None, resid_buf=None)
    ld = N + c.pad
    if profile == "exact":
        s = 2.0 ** -exact_shift(K)
        a, w = ri(-4, 4, M, K), ri(-4, 4, rows, K)
        assert float(a.abs().max()) * float(w.abs().max()) * K < 2 ** 24
        a, w = a.to(BF), (w * s).to(BF)
        bias = (ri(-8, 8, N) * s).to(BF) if c.bias else None
        r = ri(-64, 64, M, N) * s if c.mode == 2 else None
    else:
        a = torch.randn(M, K, generator=gen).to(BF)
        w = (torch.randn(rows, K, generator=gen) / math.sqrt(K)).to(BF)
        bias = torch.randn(N, generator=gen).to(BF) if c.bias else None
        r = torch.randn(M, N, generator=gen) if c.mode == 2 else None
    d["a"], d["w"] = guarded(a, c.ldx), guarded(w, c.ldx)
    if bias is not None:
        d["bias"] = guarded_vec(bias)
    if r is not None:
        buf = OutBuf(M, N, ld, F32, c.roff)
        buf.flat = torch.full_like(buf.flat, NAN)
        buf.view()[:M, :N] = r
        d["resid_buf"], d["resid"] = buf, buf.flat
    if c.op == "dswiglu":
        d["gu"] = guarded(torch.randn(M, 2 * N, generator=gen).to(BF))
    if c.op == "qkv":
        cs, sn = rope_table(M)
        d["cos"], d["sin"] = guarded(cs), guarded(sn)
    return d


# ================================================================================================ the float64 restatement
def _bf64(x):
    """float64 -> the nearest bf16 (ties to even), as float64; callers pass values exact in fp32 (the exact profile)"""
    return x.to(F32).to(BF).to(F64)


Ref = collections.namedtuple("Ref", "exact tol frac_rounded scale")


def _core(c, d):
    a, w = d["a"][:c.M, :c.K].to(F64), d["w"][:-GUARD, :c.K].to(F64)
    bias = 0.0 if d["bias"] is None else d["bias"][:c.N].to(F64)
    R = None if d["resid"] is None else d["resid_buf"].view(d["resid"])[:c.M, :c.N].to(F64)
    return a, w, bias, R


def reference(c, d):
    """The float64 results of a case: exact: name -> tensor whose BITS are the right answer (exact profile); tol: name -> (ref, E),
    held within GEMM_LIMIT x E (E None: the rms statistic only); frac_rounded: the share of accumulations a bf16 rounding changes;
    scale: name -> the magnitude the N(0, 1) statistic divides by where it is not |ref|.
    Names: c | gu, act | qk, v | dact, dgu | slab0 .., c."""
    M, N, K = c.M, c.N, c.K
    a, w, bias, R = _core(c, d)
    ex = d["profile"] == "exact"
    acc = a @ w.t()
    absacc = None if ex else a.abs() @ w.abs().t()
    if ex:
        assert torch.equal(acc, acc.to(F32).to(F64)), "the exact profile's sums are not exact in fp32"
    frac = float((_bf64(acc) != acc).double().mean())
    rnd = _bf64 if ex else (lambda t: t)
    Fa = None if ex else (K + 2) * 2.0 ** -24 * (absacc + (bias.abs() if torch.is_tensor(bias) else 0.0))
    Ebf = lambda z, F: U * (z.abs() + F) + F                    # one bf16 rounding of an fp32 accumulation
    exact, tol, scale = {}, {}, {}

    def linear(name, z, F, dtype=BF):
        if ex:
            exact[name] = z.to(F32).to(dtype)
        else:
            tol[name] = (z, Ebf(z, F) if dtype == BF else F)

    if c.op in ("plain", "relu"):
        z = acc + bias
        if c.op == "relu" and ex:
            exact["c"] = z.clamp_min(0.0).to(F32).to(BF)
        elif c.op == "relu":
            tol["c"] = (z.clamp_min(0.0), Ebf(z, Fa))
        elif c.mode == 0:
            linear("c", z, Fa)
        elif c.mode == 1:
            linear("c", z, Fa, F32)
        elif ex:
            exact["c"] = (R + rnd(z)).to(F32)
        else:
            tol["c"] = (R + z, Ebf(z, Fa) + 2.0 ** -24 * (R.abs() + z.abs() + Fa))
    elif c.op == "swiglu":
        linear("gu", acc, Fa)
        g, t = rnd(acc[:, :N]), rnd(acc[:, N:])
        act = g / (1.0 + torch.exp(-g)) * t
        if ex:
            assert float(g.abs().max()) <= 5.0, "2^-20 covers silu_f for |g| <= 5 only"
        tol["act"] = (act, (2 * U + U * U + 2.0 ** -20) * act.abs() if ex else None)
    elif c.op == "qkv":
        H, G = c.H, c.G
        z = acc + bias
        x = rnd(z).view(M, H + 2 * G, HD)
        cs, sn = d["cos"][:M].to(F64)[:, None, :], d["sin"][:M].to(F64)[:, None, :]
        x1, x2 = x[:, :H + G, :64], x[:, :H + G, 64:]
        rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
        slop = torch.cat([(x1 * cs).abs() + (x2 * sn).abs(), (x2 * cs).abs() + (x1 * sn).abs()], -1)
        tol["qk"] = (rot.reshape(M, -1), (U * rot.abs() + 2.0 ** -22 * slop).reshape(M, -1) if ex else None)
        scale["qk"] = slop.reshape(M, -1)
        linear("v", z[:, (H + G) * HD:], None if ex else Fa[:, (H + G) * HD:])
    elif c.op == "dswiglu":
        linear("dact", acc, Fa)
        dd = rnd(acc)
        g, t = d["gu"][:M, :N].to(F64), d["gu"][:M, N:].to(F64)
        sg = 1.0 / (1.0 + torch.exp(-g))
        f = 1.0 + g * (1.0 - sg)
        dg, du = dd * t * sg * f, dd * g * sg
        a1 = (2 * g.abs() + 6) * 2.0 ** -24
        Ef = g.abs() * (sg * a1 + 2.0 ** -24) + 2.0 ** -23 * (1.0 + g.abs() * (1.0 - sg))
        Edg = U * dg.abs() + (dd * t).abs() * sg * (a1 * f.abs() + Ef) + 2.0 ** -22 * dg.abs()
        Edu = (U + a1 + 2.0 ** -22) * du.abs()
        tol["dgu"] = (torch.cat([dg, du], 1), torch.cat([Edg, Edu], 1) if ex else None)
    else:                                                        # splitk / slabs: each slab is the sum over its own K range
        per = K // c.ks
        total = torch.zeros(M, N, dtype=F64)
        Ft = None if ex else torch.zeros(M, N, dtype=F64)
        for s in range(c.ks):
            sl = slice(s * per, (s + 1) * per)
            z = a[:, sl] @ w[:, sl].t()
            Fs = None if ex else (per + 2) * 2.0 ** -24 * (a[:, sl].abs() @ w[:, sl].abs().t())
            linear(f"slab{s}", z, Fs, F32)
            total += z
            if not ex:
                Ft += Fs
        if not ex:
            Ft += c.ks * 2.0 ** -24 * absacc                     # the ks - 1 additions of tasu_sum_slabs_bf16
        linear("c", total, Ft)
    return Ref(exact, tol, frac, scale)


# ================================================================================================ the torch double
def run_double(fake, c, d):
    """The torch double (tests/fake_ops.py) on a case: name -> result [M, N] (the names of `reference`), run on guarded buffers
    of the same layout as the kernels' and checked by OutBuf.check."""
    M, N, K = c.M, c.N, c.K
    a, w = d["a"], d["w"]
    bias = None if d["bias"] is None else d["bias"]
    what = f"double {case_id(c)}"
    if c.op in ("plain", "relu"):
        out = OutBuf(M, N, N + c.pad, BF if c.mode == 0 else F32, c.coff)
        R = None if d["resid"] is None else d["resid_buf"].view(d["resid"])
        if c.op == "relu":
            tmp = torch.zeros(M, N, dtype=BF)
            fake.gemm_bias_relu(a, w[:-GUARD], tmp, M, N, K, bias)
            out.view()[:M, :N] = tmp
        else:
            fake.gemm(a, w[:-GUARD], out.view(), M, N, K, bias=bias, resid=R, mode=c.mode)
        return {"c": out.check(out.flat, what)}
    if c.op == "swiglu":
        gu, act = torch.zeros(M, 2 * N, dtype=BF), torch.zeros(M, N, dtype=BF)
        fake.gemm_gate_up_swiglu(a, w[:-GUARD], gu, act, M, N, K)
        return {"gu": gu, "act": act}
    if c.op == "qkv":
        qkv = torch.zeros(M, N, dtype=BF)
        fake.gemm_qkv_rope(a, w[:-GUARD], bias, qkv, d["cos"][:M].contiguous(), d["sin"][:M].contiguous(), M, c.H, c.G, K)
        return {"qk": qkv[:, :(c.H + c.G) * HD], "v": qkv[:, (c.H + c.G) * HD:]}
    if c.op == "dswiglu":
        dact, dgu = torch.zeros(M, N, dtype=BF), torch.zeros(M, 2 * N, dtype=BF)
        fake.gemm_dswiglu(a, w[:-GUARD], d["gu"][:M], dgu, dact, M, N, K)
        return {"dact": dact, "dgu": dgu}
    per = K // c.ks
    res = {}
    for s in range(c.ks):
        slab = torch.zeros(M, N)
        fake.gemm(a[:, s * per:(s + 1) * per], w[:-GUARD, s * per:(s + 1) * per], slab, M, N, per, mode=1)
        res[f"slab{s}"] = slab
    cc = torch.zeros(M, N, dtype=BF)
    fake.gemm_splitk(a, w[:-GUARD], cc, M, N, K, c.ks, None)
    res["c"] = cc
    return res


# ================================================================================================ checks
def check_case(c, d, ref, out, what):
    """one run's results against the reference: the bits where float64 names them, GEMM_LIMIT x E elsewhere; returns the largest
    |err| / E"""
    worst = 0.0
    for name, want in ref.exact.items():
        assert_bits(out[name], want, f"{what} {name}", c.K)
    for name, (want, E) in ref.tol.items():
        if E is not None:
            worst = max(worst, assert_gemm_within(out[name], want, E, GEMM_LIMIT, f"{what} {name}", c.K).worst)
    return worst


def rms_pairs(c, d, ref, out):
    """(name, got, want, scale) float64 of the results the N(0, 1) statistic is taken on: the bf16-rounded ones -- an fp32
    `R + bf16(sum)` less its R, the fp32 outputs not at all"""
    for name, (want, _) in ref.tol.items():
        if (c.op == "plain" and c.mode == 1) or name.startswith("slab"):
            continue
        got = out[name].to(F64)
        if c.op == "plain" and c.mode == 2:
            R = d["resid_buf"].view(d["resid"])[:c.M, :c.N].to(F64)
            got, want = got - R, want - R
        yield name, got, want, ref.scale.get(name)
