"""TEST HELPER (not a test, never shipped): plain float64 restatements of the fp32 decode family (csrc/fp32.hip, `tasu_f32_*`) on
the exact fp32 input values, each with a first-order bound E for every element it returns, the case lists, the seeded inputs and
the runs (`run_*`) that tests/test_f32_ref64_cpu.py (through F32Torch, a plain-torch fp32 restatement with HipOps' f32_* method
names) and tests/test_gpu_f32_f64.py (through HipOps) share.  Nothing is shared with the kernels.

RULES (those of tests/row_ref64.py).  e = 2^-24, LIMIT = 1.0: every element is held to |got - ref| <= E, and has the reference's
value exactly where E = 0 (copies, zero rows, max, integer outputs, the exact profiles).  An fp32 +, *, / : e relative; rsqrtf
4 e; expf 2 e and e |d| for its argument d; logf of S >= 1: 4 e |log S| + 2 e.  A fixed-order sum of terms t_i carries
depth . e . sum |t_i|, depth the longest chain of fp32 additions a term passes in THAT kernel:

    GEMMs          exact profile: integers in [-4, 4], dyadic bias / residual, max|a| max|w| K < 2^24: every partial sum is exact
                   in any order, the product is compared with torch.equal.  N(0, 1) profile (K <= 512):
                   F = (K + 2) e (sum |a w| + |bias|) [+ e (|r| + |c|) with a residual]: the tile kernel's chain is K / ksplit MFMA
                   steps + ksplit slabs, the streaming kernel's 16 KS + 8 waves + ksplit slabs, both below K + 2.
                   ReLU is 1-Lipschitz: F.  SiLU x / (1 + t), t = expf(-x): 1.1 F + e |silu| (5 + |x| t / (1 + t))  (|silu'| <= 1.1;
                   expf's 2 e, the addition, the division; expf's argument allowance e |x| weighs t / (1 + t) in the quotient),
                   and |x| 2^-126 absolute where |x| > 80 (expf(-x) leaves the fp32 range at 88.7: the quotient is then 0 where
                   the value is |x| 2^-128 at most).
                   (The argument allowance is not only the rounding of a difference d: the compiler's expansion of expf is
                   exp2(a), a = (ph - E) + pl with ph = fl(x log2e), E = rint(ph), pl the product's residual; under
                   -ffp-contract=fast ph - E is contracted to fma(x, log2e, -E), which counts the residual twice: up to half an
                   ulp of ph in the exponent, e |x| relative.  So expf(d) carries 2 e + e |d| wherever it stands.)
    rmsnorm        ss = sum x^2: ceil(D / 1024) serial adds per thread + 6 shuffle levels + 16 waves + the product = depth_ss;
                   rs = rsqrtf(ss / D + eps): rel_rs = e (depth_ss / 2 + 5) [+ sum |x| F_x / (ss + D eps) behind a GEMM];
                   y = w (x rs): E = |w| rs F_x + |y| (rel_rs + 2 e)
    swiglu         silu(g) u, one rounding more: E = |u| E_silu(g) + |silu(g)| F_u + 2 e |act|  (|g| <= 80 on the pointwise kernel)
    rope           y1 = x1 c - x2 s, y2 = x2 c + x1 s, products and sum rounded separately: the bits of torch eager on the kernel's own
                   x (tasu_f32_rope, and the q|k|v finisher on an exact sum); behind an N(0, 1) sum
                   E = |c| F_1 + |s| F_2 + e (|x1 c| + |x2 s| + |y|)
    attention      s_j = scale sum_d q_d k_jd: 16 serial products per lane + 3 shuffle levels + the product + the scale = 21:
                   Es_j = 21 e scale sum_d |q_d k_jd|;  e_j = expf(s_j - m): delta_j = 2 e + e |s_j - m| + Es_j relative (the error
                   of m itself is a common factor of every e_j and of their sum);  the sum: ceil(n / NT) serial + 6 levels + NW
                   waves;  1 / sum: e;  p = e_j inv: e;  o = sum_j p_j v_j: ceil(n / NW) serial over the wave's share + NW partials
                   + the product:  E_o = sum_j p_j |v_j| (delta_j + sum_i p_i delta_i + e (ceil(n / NT) + ceil(n / NW) + 2 NW + 9))
                   NT / NW = 256 / 4 (prefill, bidirectional), 512 / 8 (decode).  Rows without a visible key: zeros, exactly.
    fsmn           out += sum_j w_j v_j + v: ksize + 1 serial adds, the products, the add into out:
                   E = (ksize + 2) e (sum |w v| + |v| + |out_0|)
    cross-entropy  exact max (first column on ties), S = sum expf(x - m): ceil(V / 1024) serial + 6 + 16 = depth;
                   E_lse = e |lse| + 4 e |log S| + 2 e + e depth + sum_j P_j e (|d_j| + 2);  loss = lse - x_label: E_lse + e |loss|;
                   g = k (expf(x - lse) - [c = label]): A_g = k p (E_lse + e |x - lse| + 2 e) + 2 e |g|, absolute; unlabelled rows
                   and pad columns: 0.  Every row keeps max - min <= 40.
    kv_fill, embed_merge, the fragment-order copy: copies, exact.

GUARDS.  Every output, workspace and cache starts as NaN (integers -7); every operand has NaN guard rows behind it and NaN in the gap
of a leading dimension greater than its width, so a read past the range stays inside the allocation and shows in the result;
everything outside what a call owes must keep its bits (the runs assert it); calls that take a workspace run twice, equal bits.

No rms-ratio check for the GEMMs: a blocked CPU sum is not a fair comparator for a serial K chain."""
import collections
import math

import torch

from row_ref64 import LIMIT, NAN, Ref, bits, cdiv, check, e, gen, nan, same_bits, untouched, worst_of  # noqa: F401

F64, F32, I32 = torch.float64, torch.float32, torch.int32
HD = 128
GUARD = 3                                                        # NaN rows behind every operand and output
EPS = 1e-6
TINY = 2.0 ** -126
MAX_KEYS, MAX_REP = 2048, 8


def ident(t):
    return t


def case_id(c):
    return "-".join(str(getattr(c, f)) for f in c._fields)


# ------------------------------------------------------------------------------------------------ guarded buffers
def operand(t, ld=None, dev=ident):
    """t [R, C] as a view of a NaN buffer [R + GUARD, ld] on the device (row stride ld)"""
    R, C = t.shape
    full = nan(R + GUARD, ld or C, dtype=t.dtype) if t.dtype != I32 else torch.full((R + GUARD, ld or C), -7, dtype=I32)
    full[:R, :C] = t
    return dev(full)[:R, :C]


def vec(t, dev=ident):
    """t [n] with a guard tail (NaN; integers -7)"""
    tail = torch.full((GUARD,), -7, dtype=I32) if t.dtype == I32 else nan(GUARD, dtype=t.dtype)
    return dev(torch.cat([t, tail]))[:t.numel()]


def output(R, C, ld=None, dev=ident, init=None, dtype=F32):
    """(the whole NaN buffer [R + GUARD, ld], its [R, C] view); init: what the view holds before the call (in-place residual)"""
    full = nan(R + GUARD, ld or C) if dtype == F32 else torch.full((R + GUARD, ld or C), -7, dtype=dtype)
    if init is not None:
        full[:R, :C] = init
    full = dev(full)
    return full, full[:R, :C]


def owed(full, R, C, what):
    """the [R, C] block of a finished buffer on the CPU, after asserting that everything outside it kept its bits"""
    full = full.cpu()
    assert untouched(full[R:]), f"{what}: rows >= {R} were written"
    assert untouched(full[:R, C:]), f"{what}: columns >= {C} were written"
    return full[:R, :C].contiguous()


# ------------------------------------------------------------------------------------------------ F32Torch: the fp32 restatement
def silu32(x):
    return x / (1 + torch.exp(-x))


def rope_eager(x, cos, sin):
    """x [M, heads, 128] fp32, cos / sin [M, 64]: x cos + rotate_half(x) sin as torch eager rounds it"""
    c, s = torch.cat([cos, cos], -1)[:, None, :], torch.cat([sin, sin], -1)[:, None, :]
    rot = torch.cat([-x[..., 64:], x[..., :64]], -1)
    return x * c + rot * s


class F32Torch:
    """plain torch fp32 on the CPU under HipOps' f32_* names and signatures (a test helper: the CPU file and the mutants run
    through it).  Outputs are written into the caller's views; workspaces are ignored."""
    name = "f32torch"

    def _prod(self, a, w, M, N, K):
        return a[:M, :K] @ w[:N, :K].t()

    def _epilogue(self, v, bias, resid, act, M, N):
        if bias is not None:
            v = v + bias[:N]
        v = silu32(v) if act == 1 else (v.clamp_min(0) if act == 2 else v)
        return resid[:M, :N] + v if resid is not None else v

    def f32_gemm(self, a, w, c, M, N, K, bias=None, resid=None, act=0, ws=None):
        c[:M, :N] = self._epilogue(self._prod(a, w, M, N, K), bias, resid, act, M, N)

    def f32_gemm_stream(self, a, w, c, M, N, K, ks, bias=None, resid=None, act=0, ws=None):
        self.f32_gemm(a, w, c, M, N, K, bias, resid, act, ws)

    def _mean_sq(self, x, D):
        return x.pow(2).sum(-1, keepdim=True) / D

    def f32_rmsnorm(self, x, w, y, M, D, eps):
        xv = x[:M, :D]
        y[:M, :D] = w[:D] * (xv * torch.rsqrt(self._mean_sq(xv, D) + eps))

    def f32_gemm_resid_rmsnorm(self, a, w, x, norm_w, y, M, N, K, eps, ws, resid=None, bias=None):
        self.f32_gemm(a, w, x, M, N, K, bias=bias, resid=resid)
        self.f32_rmsnorm(x, norm_w, y, M, N, eps)

    def f32_swiglu(self, gu, act, M, I):
        act[:M, :I] = silu32(gu[:M, :I]) * gu[:M, I:2 * I]

    def f32_gemm_swiglu(self, a, wgu, gu, act, M, I, K, ws):
        g = self._prod(a, wgu, M, 2 * I, K)
        if gu is not None:
            gu[:M, :2 * I] = g
        self.f32_swiglu(g, act, M, I)

    def _slot(self, slot):
        return slot

    def f32_rope(self, qkv, cos, sin, M, H, G, kc=None, vc=None, slot=None, ctx=0, inverse=False):
        x = qkv[:M].view(M, H + 2 * G, HD)
        x[:, :H + G] = rope_eager(x[:, :H + G].clone(), cos[:M], -sin[:M] if inverse else sin[:M])
        if kc is not None:
            rows, sl = torch.arange(M), self._slot(slot[:M]).long()
            kc.view(-1, ctx, G * HD)[rows, sl] = x[:, H:H + G].reshape(M, -1)
            vc.view(-1, ctx, G * HD)[rows, sl] = x[:, H + G:].reshape(M, -1)

    def f32_gemm_qkv_rope(self, a, wqkv, bias, qkv, cos, sin, M, H, G, K, ws, kc=None, vc=None, slot=None, ctx=0):
        self.f32_gemm(a, wqkv, qkv, M, (H + 2 * G) * HD, K, bias=bias)
        self.f32_rope(qkv, cos, sin, M, H, G, kc, vc, slot, ctx)

    def f32_kv_fill(self, qkv, kc, vc, B, S, H, G, nb, ctx):
        x = qkv[:B * S].view(B, S, H + 2 * G, HD)
        kc.view(-1, ctx, G * HD)[0:B * nb:nb, :S] = x[:, :, H:H + G].reshape(B, S, -1)
        vc.view(-1, ctx, G * HD)[0:B * nb:nb, :S] = x[:, :, H + G:].reshape(B, S, -1)

    def _softmax_pv(self, q, k, v, scale):
        p = torch.softmax((q @ k.t()) * scale, -1)
        return p @ v

    def f32_attn_prefill(self, qkv, kstart, out, B, S, H, G, scale, klen=None):
        x, rep = qkv[:B * S].view(B, S, H + 2 * G, HD), H // G
        o = out[:B * S].view(B, S, H, HD)
        o.zero_()
        for b in range(B):
            hi = min(int(klen[b]), S) if klen is not None else None
            for s in range(S):
                lo, top = (0, hi) if klen is not None else (int(kstart[b]), s + 1)
                if s < lo or top <= lo or (klen is not None and s >= top):
                    continue
                for g in range(G):
                    o[b, s, g * rep:(g + 1) * rep] = self._softmax_pv(x[b, s, g * rep:(g + 1) * rep], x[b, lo:top, H + g],
                                                                      x[b, lo:top, H + G + g], scale)

    def _keys(self, kc, vc, index, m, lo, hi, ctx, G):
        rows, pos = index[m, lo:hi].long(), torch.arange(lo, hi)
        return kc.view(-1, ctx, G, HD)[rows, pos], vc.view(-1, ctx, G, HD)[rows, pos]

    def f32_attn_decode(self, qkv, kc, vc, index, kstart, lens, out, M, H, G, ctx, scale):
        rep = H // G
        x, o = qkv[:M].view(M, H + 2 * G, HD), out[:M].view(M, H, HD)
        o.zero_()
        for m in range(M):
            lo, hi = int(kstart[m]), int(lens[m])
            if hi <= lo:
                continue
            k, v = self._keys(kc, vc, index.view(-1, ctx), m, lo, hi, ctx, G)
            for g in range(G):
                o[m, g * rep:(g + 1) * rep] = self._softmax_pv(x[m, g * rep:(g + 1) * rep], k[:, g], v[:, g], scale)

    def f32_fsmn(self, v, ldv, w, lens, out, B, T, D, ksize):
        left = (ksize - 1) // 2
        vv, o = v[:B * T, :D].reshape(B, T, D), out[:B * T].view(B, T, D)
        for b in range(B):
            n = int(lens[b])
            for t in range(n):
                r = torch.zeros(D)
                for j in range(ksize):
                    tt = t + j - left
                    if 0 <= tt < n:
                        r = r + w[:D, j] * vv[b, tt]
                o[b, t] += r + vv[b, t]

    def f32_embed_merge(self, table, proj, kind, idx, x, M, D):
        for m in range(M):
            k, i = int(kind[m]), int(idx[m])
            x[m, :D] = table[i, :D] if k == 1 else (proj[i, :D] if k == 2 else torch.zeros(D))

    def _argmax(self, x):
        return x.argmax(-1)

    def _pad_columns(self, d, V):
        d[:, V:] = 0

    def f32_ce(self, logits, labels, M, V, row_loss, row_hit, row_argmax=None, row_lse=None, dlogits=None, inv_count=None):
        x = logits[:M, :V].clone()
        lab = labels[:M].long()
        on = (lab >= 0) & (lab < V)
        lse = torch.logsumexp(x, -1)
        am = self._argmax(x)
        xl = x.gather(1, torch.where(on, lab, torch.zeros_like(lab))[:, None])[:, 0]
        row_loss[:M] = torch.where(on, lse - xl, torch.zeros(M))
        row_hit[:M] = (on & (am == lab)).to(I32)
        if row_argmax is not None:
            row_argmax[:M] = am.to(I32)
        if row_lse is not None:
            row_lse[:M] = lse
        if dlogits is not None:
            k = torch.where(on, inv_count[0].expand(M), torch.zeros(M))[:, None]
            onehot = (torch.arange(V)[None, :] == lab[:, None]).to(F32)
            dlogits[:M, :V] = k * (torch.exp(x - lse[:, None]) - onehot)
            self._pad_columns(dlogits[:M], V)


# ------------------------------------------------------------------------------------------------ GEMMs
# route: "tile" (tasu_f32_gemm_nt) or the forced streaming kernel's ks; ws: workspace floats (0: none; -1: 16 M N); ld*: extra
# floats beyond the width; profile: exact | n01 | outlier (n01 with residual column 1 x 2^10; needs resid)
Gemm = collections.namedtuple("Gemm", "route M N K act bias resid profile lda ldw ldc ws")


def tile_ksplit(M, N, K, ws):
    """f32_tile_ksplit of csrc/fp32.hip restated (ws: workspace floats, 0 = none)"""
    tiles = cdiv(N, 64) * cdiv(M, 64)
    ks = 1
    if ws and tiles < 1024:
        ks = min(8, cdiv(1024, tiles))
        while ks > 1 and ((K // 32) % ks or ks * M * N > ws):
            ks -= 1
    return ks


def stream_walks(N, ksplit, cus):
    """(nbx, the set of walk lengths) of the streaming kernel's workgroups"""
    tiles = cdiv(N, 16)
    nbx = max(1, min(tiles, cus // ksplit))
    return nbx, {cdiv(tiles - bx, nbx) for bx in range(nbx)}


def walk_N(length, cus, ksplit=16):
    """an N whose workgroups all walk `length` tiles at this ksplit, the last tile partial"""
    return 16 * max(1, cus // ksplit) * length - 5


def ws_floats(c):
    return 16 * max(c.M, 64) * c.N if c.ws < 0 else c.ws


TILE_SHAPES = [(1, 1, 32), (64, 64, 32), (65, 70, 96)]
TILE_CASES = ([Gemm("tile", M, N, K, 0, False, False, p, 0, 0, 0, 0) for M, N, K in TILE_SHAPES for p in ("exact", "n01")]
              + [Gemm("tile", 65, 70, K, 0, True, False, p, 0, 0, 0, -1) for K in (256, 224, 160, 96, 64, 32) for p in ("exact", "n01")]
              + [Gemm("tile", 65, 70, 256, 0, False, False, "exact", 0, 0, 0, 4 * 65 * 70 + 9)]          # the workspace holds 4 slabs
              + [Gemm("tile", 65, 70, 96, act, b, r, p, 4, 8, 3, ws) for act in (0, 1, 2) for b in (False, True) for r in (False, True)
                 for p, ws in (("exact", 0), ("n01", -1))]
              + [Gemm("tile", 33, 250, 384, 0, True, True, "outlier", 0, 4, 1, ws) for ws in (0, -1)])
TILE_KSPLITS = {256: 8, 224: 7, 160: 5, 96: 3, 64: 2, 32: 1}

STREAM_M = (1, 16, 17, 32, 33, 48, 49, 64)
STREAM_EXACT = [Gemm(ks, M, 40, 128 * ks * sp, 0, True, False, "exact", 0, 0, 0, -1) for ks in range(1, 7) for sp in (1, 2, 16) for M in STREAM_M]
STREAM_N01 = ([Gemm(ks, M, N, 128 * ks * sp, act, b, r, p, lda, ldw, ldc, -1)
               for (ks, sp) in ((1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (1, 4))
               for (M, N, act, b, r, p, lda, ldw, ldc) in ((1, 20, 0, False, False, "n01", 0, 0, 0), (17, 31, 1, True, True, "n01", 4, 8, 3),
                                                           (33, 100, 0, True, True, "outlier", 0, 4, 1), (64, 25, 2, True, False, "n01", 4, 0, 0))])
STREAM_NS = [Gemm(2, 33, N, 512, 0, True, False, p, 0, 4, 2, -1) for N in (1, 3, 16, 20, 25, 31) for p in ("exact", "n01")]
STREAM_WALKS = (1, 2, 3, 4, 5, 7)


def gemm_inputs(c):
    g = gen(7, c.M, c.N, c.K, c.act, 0 if c.route == "tile" else c.route)
    M, N, K = c.M, c.N, c.K
    if c.profile == "exact":
        a = torch.randint(-4, 5, (M, K), generator=g).to(F32)
        w = torch.randint(-4, 5, (N, K), generator=g).to(F32)
        bias = torch.randint(-32, 33, (N,), generator=g).to(F32) / 4
        resid = torch.randint(-32, 33, (M, N), generator=g).to(F32) / 4
        assert 16 * K < 2 ** 24
    else:
        a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
        bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        assert K <= 512
        if c.profile == "outlier":
            assert c.resid
            resid[:, min(1, N - 1)] *= 1024.0
    return dict(a=a, w=w, bias=bias if c.bias else None, resid=resid if c.resid else None, case=c)


def gemm_sum(d):
    """(the float64 product + bias, its bound F without the residual term)"""
    c = d["case"]
    a, w = d["a"].to(F64), d["w"].to(F64)
    s, A = a @ w.t(), a.abs() @ w.abs().t()
    if d["bias"] is not None:
        s, A = s + d["bias"].to(F64), A + d["bias"].to(F64).abs()
    F = torch.zeros_like(s) if c.profile == "exact" else (c.K + 2) * e * A
    return s, F


def silu_ref(x, F):
    t = x / (1 + torch.exp(-x))
    return t, 1.1 * F + e * t.abs() * (5 + x.abs() / (1 + torch.exp(x))) + TINY * x.abs() * (x.abs() > 80).to(F64)


def gemm_reference(d):
    c = d["case"]
    s, F = gemm_sum(d)
    if c.act == 1:
        s, F = silu_ref(s, F)
    elif c.act == 2:
        s = s.clamp_min(0)
    if d["resid"] is not None:
        r = d["resid"].to(F64)
        s = r + s
        if c.profile != "exact" or c.act == 1:
            F = F + e * (r.abs() + s.abs())
    if c.profile == "exact" and c.act != 1:
        assert torch.equal(s.to(F32).to(F64), s)
        return Ref({}, {"c": s.to(F32)})
    return Ref({"c": (s, F)}, {})


def _call_gemm(ops, c, a, w, cv, bias, resid, ws):
    if c.route == "tile":
        ops.f32_gemm(a, w, cv, c.M, c.N, c.K, bias=bias, resid=resid, act=c.act, ws=ws)
    else:
        ops.f32_gemm_stream(a, w, cv, c.M, c.N, c.K, c.route, bias=bias, resid=resid, act=c.act, ws=ws)


def run_gemm(ops, d, dev=ident, sync=lambda: None):
    """the case through ops (in-place residual), twice when it has a workspace: {"c"}"""
    c = d["case"]
    M, N, K = c.M, c.N, c.K
    a, w = operand(d["a"], K + c.lda, dev), operand(d["w"], K + c.ldw, dev)
    bias = vec(d["bias"], dev) if c.bias else None
    res = []
    for _ in range(2 if c.ws else 1):
        ws = dev(nan(ws_floats(c))) if c.ws else None
        full, cv = output(M, N, N + c.ldc, dev, init=d["resid"])
        _call_gemm(ops, c, a, w, cv, bias, cv if c.resid else None, ws)
        sync()
        res.append(owed(full, M, N, f"gemm {case_id(c)}"))
    if len(res) == 2:
        same_bits(res[1], res[0], f"gemm {case_id(c)}, second run")
    return {"c": res[0]}


def fragment_order(w):
    """the fragment-order copy of w [N, K] as the header defines it: [tile][K / 16][lane = 16 g + n][4], rows >= N zero"""
    N, K = w.shape
    T = cdiv(N, 16)
    wp = torch.zeros(T * 16, K, dtype=w.dtype)
    wp[:N] = w
    return wp.view(T, 16, K // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1)


# ---- finishers
# route: "unsplit" (no workspace: one K range, the kernel behind it) | "slabs" (the tile kernel's K-range slabs) | "stream" (a 32 MB
# matrix: the streaming kernel's slabs, exact profile); scales: row scales span 2^-10 .. 2^10
Fin = collections.namedtuple("Fin", "op route M N K profile")
FIN_CASES = ([Fin(op, route, M, N, K, p) for op in ("norm", "swiglu") for route in ("unsplit", "slabs")
              for (M, N, K, p) in ((5, 70, 64, "exact"), (33, 250, 256, "n01"), (21, 1030, 128, "scales"))]
             + [Fin("norm", route, 33, 250, 384, "outlier") for route in ("unsplit", "slabs")])
Qkv = collections.namedtuple("Qkv", "route M H G K profile cache slot")
QKV_CASES = [Qkv(route, M, H, G, K, p, cache, slot) for route in ("unsplit", "slabs")
             for (M, H, G, K, p, cache, slot) in ((3, 2, 1, 64, "exact", False, "zero"), (5, 12, 2, 128, "n01", True, "zero"),
                                                  (4, 28, 4, 64, "n01", True, "last"), (7, 16, 2, 256, "exact", True, "last"),
                                                  (2, 16, 2, 64, "n01", False, "zero"))]
FIN_STREAM = [Fin("norm", "stream", 33, 2048, 4096, "exact"), Fin("swiglu", "stream", 5, 1024, 4096, "exact")]
QKV_STREAM = Qkv("stream", 17, 12, 2, 4096, "exact", True, "last")
CTX_QKV = 5


def split(c):
    return c.route != "unsplit"


def streams(M, N, K, ws):
    """tasu_f32_gemm_streams restated for the cases here (the lab-only switches aside)"""
    return M <= 64 and K % 128 == 0 and N * K * 4 >= 32 << 20 and any((K // 128) % ks == 0 and ((K // 128) // ks == 1 or
           ((K // 128) // ks <= 16 and (K // 128) // ks * 64 * N <= ws)) for ks in range(1, 7))


def fin_ws(c, N):
    return 16 * 64 * N if split(c) else 0


def fin_inputs(c):
    N = 2 * c.N if c.op == "swiglu" else c.N
    base = Gemm("tile", c.M, N, c.K, 0, c.op == "norm", c.op == "norm", "exact" if c.profile == "exact" else ("outlier" if c.profile == "outlier" else "n01"),
                0, 0, 0, fin_ws(c, N))
    d = gemm_inputs(base)
    g = gen(11, c.M, c.N, c.K)
    if c.profile == "scales":
        sc = 2.0 ** torch.linspace(-10, 10, c.M).round()
        d["a"] = d["a"] * sc[:, None]
        if d["resid"] is not None:
            d["resid"] = d["resid"] * sc[:, None]
            d["bias"] = None
    d["norm_w"] = torch.randn(c.N, generator=g) if c.profile != "exact" else torch.randint(-4, 5, (c.N,), generator=g).to(F32)
    d["fin"] = c
    assert streams(c.M, N, c.K, fin_ws(c, N)) == (c.route == "stream")
    assert c.route == "stream" or (tile_ksplit(c.M, N, c.K, fin_ws(c, N)) > 1) == (c.route == "slabs")
    return d


def rmsnorm_ref(x, Fx, w, D, eps=EPS):
    ss = (x * x).sum(-1, keepdim=True)
    rs = torch.rsqrt(ss / D + eps)
    depth = cdiv(D, 1024) + 6 + 16 + 1
    rel = e * (depth / 2 + 5) + (x.abs() * Fx).sum(-1, keepdim=True) / (ss + D * eps)
    y = w * (x * rs)
    return y, w.abs() * rs * Fx + y.abs() * (rel + 2 * e)


def fin_reference(d):
    c = d["fin"]
    s, F = gemm_sum(d)
    if c.op == "norm":
        r = d["resid"].to(F64)
        x = r + s
        Fx = F + e * (r.abs() + x.abs()) if c.profile != "exact" else F
        y, Ey = rmsnorm_ref(x, Fx, d["norm_w"].to(F64), c.N)
        if c.profile == "exact":
            return Ref({"y": (y, Ey)}, {"x": x.to(F32)})
        return Ref({"x": (x, Fx), "y": (y, Ey)}, {})
    g, u, Fg, Fu = s[:, :c.N], s[:, c.N:], F[:, :c.N], F[:, c.N:]
    t, Et = silu_ref(g, Fg)
    act = t * u
    ref = Ref({"act": (act, u.abs() * Et + t.abs() * Fu + 2 * e * act.abs())}, {})
    if c.route == "unsplit":
        if c.profile == "exact":
            ref.exact["gu"] = s.to(F32)
        else:
            ref.tol["gu"] = (s, F)
    return ref


def run_fin(ops, d, dev=ident, sync=lambda: None, gu_none=None, ldx=0):
    """gu_none: no gu scratch (the default on the split route, which never touches it)"""
    c = d["fin"]
    M, N, K = c.M, c.N, c.K
    NN = 2 * N if c.op == "swiglu" else N
    a, w = operand(d["a"], K + 4, dev), operand(d["w"], K + 8, dev)
    res = []
    for _ in range(2 if split(c) else 1):
        ws = dev(nan(fin_ws(c, NN))) if split(c) else None
        if c.op == "norm":
            xf, xv = output(M, N, N + ldx, dev, init=d["resid"])
            yf, yv = output(M, N, None, dev)
            ops.f32_gemm_resid_rmsnorm(a, w, xv, vec(d["norm_w"], dev), yv, M, N, K, EPS, ws, resid=xv,
                                       bias=vec(d["bias"], dev) if d["bias"] is not None else None)
            sync()
            res.append({"x": owed(xf, M, N, "gemm_resid_rmsnorm x"), "y": owed(yf, M, N, "gemm_resid_rmsnorm y")})
        else:
            gf, gv = output(M, NN, None, dev)
            af, av = output(M, N, None, dev)
            ops.f32_gemm_swiglu(a, w, None if (split(c) if gu_none is None else gu_none) else gv, av, M, N, K, ws)
            sync()
            out = {"act": owed(af, M, N, "gemm_swiglu act")}
            if c.route == "unsplit":
                out["gu"] = owed(gf, M, NN, "gemm_swiglu gu")
            else:
                assert untouched(gf.cpu()), "gemm_swiglu: the split route wrote gu"
            res.append(out)
    if len(res) == 2:
        for k in res[0]:
            same_bits(res[1][k], res[0][k], f"{case_id(c)} second run, {k}")
    return res[0]


def rope_tables(M, g):
    ang = torch.rand(M, 64, generator=g) * 6.0 - 3.0
    return ang.cos(), ang.sin()


def qkv_inputs(c):
    N = (c.H + 2 * c.G) * HD
    d = gemm_inputs(Gemm("tile", c.M, N, c.K, 0, True, False, c.profile, 0, 0, 0, 16 * 64 * N if split(c) else 0))
    d["cos"], d["sin"] = rope_tables(c.M, gen(13, c.M, c.H))
    d["slot"] = torch.full((c.M,), 0 if c.slot == "zero" else CTX_QKV - 1, dtype=I32)
    d["qkv_case"] = c
    assert streams(c.M, N, c.K, 16 * 64 * N if split(c) else 0) == (c.route == "stream")
    assert c.route == "stream" or (tile_ksplit(c.M, N, c.K, 16 * 64 * N if split(c) else 0) > 1) == (c.route == "slabs")
    return d


def rope_ref(x, F, cos, sin, H, G):
    """x, F [M, H + 2G, 128] float64; the q and k heads rotated, with the bound"""
    c, s = cos.to(F64)[:, None, :], sin.to(F64)[:, None, :]
    x1, x2, F1, F2 = x[:, :H + G, :64], x[:, :H + G, 64:], F[:, :H + G, :64], F[:, :H + G, 64:]
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    E1 = c.abs() * F1 + s.abs() * F2 + e * ((x1 * c).abs() + (x2 * s).abs() + y1.abs())
    E2 = c.abs() * F2 + s.abs() * F1 + e * ((x2 * c).abs() + (x1 * s).abs() + y2.abs())
    return torch.cat([torch.cat([y1, y2], -1), x[:, H + G:]], 1), torch.cat([torch.cat([E1, E2], -1), F[:, H + G:]], 1)


def qkv_reference(d):
    c = d["qkv_case"]
    s, F = gemm_sum(d)
    M, NH = c.M, c.H + 2 * c.G
    if c.profile == "exact":
        x = s.to(F32).view(M, NH, HD).clone()
        x[:, :c.H + c.G] = rope_eager(x[:, :c.H + c.G].clone(), d["cos"], d["sin"])
        return Ref({}, {"qkv": x.view(M, -1)})
    y, E = rope_ref(s.view(M, NH, HD), F.view(M, NH, HD), d["cos"], d["sin"], c.H, c.G)
    return Ref({"qkv": (y.reshape(M, -1), E.reshape(M, -1))}, {})


def cache_check(kc, vc, qkv, slot, M, H, G, ctx, what):
    """the finished caches [M + GUARD, ctx, G * 128] (CPU): slot[m] of row m holds the bits of qkv's k / v heads, all else NaN"""
    want_k, want_v = nan(*kc.shape), nan(*vc.shape)
    x = qkv.view(M, H + 2 * G, HD)
    rows = torch.arange(M)
    want_k[rows, slot.long()] = x[:, H:H + G].reshape(M, -1)
    want_v[rows, slot.long()] = x[:, H + G:].reshape(M, -1)
    same_bits(kc, want_k, f"{what}: k cache (slot, other positions, other rows)")
    same_bits(vc, want_v, f"{what}: v cache (slot, other positions, other rows)")


def run_qkv(ops, d, dev=ident, sync=lambda: None):
    c = d["qkv_case"]
    M, H, G, K = c.M, c.H, c.G, c.K
    N = (H + 2 * G) * HD
    a, w = operand(d["a"], K + 4, dev), operand(d["w"], K + 8, dev)
    res = []
    for _ in range(2 if split(c) else 1):
        ws = dev(nan(16 * 64 * N)) if split(c) else None
        qf, qv = output(M, N, None, dev)
        kc = dev(nan(M + GUARD, CTX_QKV, G * HD)) if c.cache else None
        vc = dev(nan(M + GUARD, CTX_QKV, G * HD)) if c.cache else None
        ops.f32_gemm_qkv_rope(a, w, vec(d["bias"], dev), qv, operand(d["cos"], None, dev), operand(d["sin"], None, dev), M, H, G, K, ws,
                              kc=kc, vc=vc, slot=vec(d["slot"], dev) if c.cache else None, ctx=CTX_QKV if c.cache else 0)
        sync()
        q = owed(qf, M, N, "gemm_qkv_rope qkv")
        if c.cache:
            cache_check(kc.cpu(), vc.cpu(), q, d["slot"], M, H, G, CTX_QKV, f"gemm_qkv_rope {case_id(c)}")
        res.append({"qkv": q})
    if len(res) == 2:
        same_bits(res[1]["qkv"], res[0]["qkv"], f"{case_id(c)} second run")
    return res[0]


# ------------------------------------------------------------------------------------------------ row and pointwise kernels
Rms = collections.namedtuple("Rms", "M D profile")
RMS_CASES = [Rms(4, D, "n01") for D in (1, 128, 1023, 1024, 1025, 3584)] + [Rms(21, 1025, "scales"), Rms(3, 1023, "zero_row")]


def rms_inputs(c):
    g = gen(17, c.M, c.D)
    x, w = torch.randn(c.M, c.D, generator=g), torch.randn(c.D, generator=g)
    if c.profile == "scales":
        x *= (2.0 ** torch.linspace(-10, 10, c.M).round())[:, None]
    if c.profile == "zero_row":
        x[1] = 0
    return dict(x=x, w=w, case=c)


def rms_reference(d):
    c = d["case"]
    x = d["x"].to(F64)
    y, E = rmsnorm_ref(x, torch.zeros_like(x), d["w"].to(F64), c.D)
    return Ref({"y": (y, E)}, {})


def run_rms(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    yf, yv = output(c.M, c.D, None, dev)
    ops.f32_rmsnorm(operand(d["x"], None, dev), vec(d["w"], dev), yv, c.M, c.D, EPS)
    sync()
    return {"y": owed(yf, c.M, c.D, "rmsnorm")}


Rope = collections.namedtuple("Rope", "M H G cache inverse")
ROPE_CASES = [Rope(5, 2, 1, False, False), Rope(5, 2, 1, False, True), Rope(3, 12, 2, True, False), Rope(9, 28, 4, True, False)]


def run_rope(ops, c, dev=ident, sync=lambda: None):
    """tasu_f32_rope: (got, want) bits -- torch eager with +-sin on the q / k heads, the v heads untouched, the cache a copy"""
    M, H, G = c.M, c.H, c.G
    N, g = (H + 2 * G) * HD, gen(19, M, H, G)
    x = torch.randn(M, N, generator=g)
    cos, sin = rope_tables(M, g)
    slot = torch.randint(0, CTX_QKV, (M,), generator=g).to(I32)
    qf, qv = output(M, N, None, dev, init=x)
    kc = dev(nan(M + GUARD, CTX_QKV, G * HD)) if c.cache else None
    vc = dev(nan(M + GUARD, CTX_QKV, G * HD)) if c.cache else None
    ops.f32_rope(qv, operand(cos, None, dev), operand(sin, None, dev), M, H, G, kc=kc, vc=vc, slot=vec(slot, dev) if c.cache else None,
                 ctx=CTX_QKV if c.cache else 0, inverse=c.inverse)
    sync()
    got = owed(qf, M, N, "rope")
    want = x.view(M, H + 2 * G, HD).clone()
    want[:, :H + G] = rope_eager(want[:, :H + G].clone(), cos, -sin if c.inverse else sin)
    if c.cache:
        cache_check(kc.cpu(), vc.cpu(), got, slot, M, H, G, CTX_QKV, f"rope {case_id(c)}")
    return got, want.view(M, N)


Fill = collections.namedtuple("Fill", "B S H G nb ctx")
FILL_CASES = [Fill(1, 1, 2, 1, 1, 1), Fill(2, 5, 4, 2, 3, 9), Fill(3, 7, 2, 2, 2, 7)]


def run_kv_fill(ops, c, dev=ident, sync=lambda: None):
    B, S, H, G, nb, ctx = c
    x = torch.randn(B * S, (H + 2 * G) * HD, generator=gen(23, B, S))
    kc, vc = dev(nan(B * nb + GUARD, ctx, G * HD)), dev(nan(B * nb + GUARD, ctx, G * HD))
    ops.f32_kv_fill(operand(x, None, dev), kc, vc, B, S, H, G, nb, ctx)
    sync()
    wk, wv = nan(B * nb + GUARD, ctx, G * HD), nan(B * nb + GUARD, ctx, G * HD)
    x4 = x.view(B, S, H + 2 * G, HD)
    for b in range(B):
        wk[b * nb, :S] = x4[b, :, H:H + G].reshape(S, -1)
        wv[b * nb, :S] = x4[b, :, H + G:].reshape(S, -1)
    same_bits(kc.cpu(), wk, f"kv_fill {case_id(c)} k cache")
    same_bits(vc.cpu(), wv, f"kv_fill {case_id(c)} v cache")


Swi = collections.namedtuple("Swi", "M I")
SWI_CASES = [Swi(1, 1), Swi(3, 257), Swi(5, 1000)]


def swi_inputs(c):
    g = gen(29, c.M, c.I)
    gu = torch.randn(c.M, 2 * c.I, generator=g)
    gu[:, :c.I] *= 20
    gu[:, :c.I].clamp_(-80, 80)
    gu[0, 0] = 0.0
    if c.I > 4:
        gu[0, 1], gu[0, 2], gu[0, 3] = 80.0, -80.0, -0.0
    return dict(gu=gu, case=c)


def swi_reference(d):
    c = d["case"]
    gu = d["gu"].to(F64)
    t, Et = silu_ref(gu[:, :c.I], torch.zeros(c.M, c.I, dtype=F64))
    act = t * gu[:, c.I:]
    return Ref({"act": (act, gu[:, c.I:].abs() * Et + 2 * e * act.abs())}, {})


def run_swi(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    af, av = output(c.M, c.I, None, dev)
    ops.f32_swiglu(operand(d["gu"], None, dev), av, c.M, c.I)
    sync()
    return {"act": owed(af, c.M, c.I, "swiglu")}


Emb = collections.namedtuple("Emb", "M D ldp")
EMB_CASES = [Emb(1, 1, 0), Emb(7, 130, 0), Emb(9, 257, 5)]


def run_embed(ops, c, dev=ident, sync=lambda: None):
    M, D, ldp = c
    g = gen(31, M, D)
    table, proj = torch.randn(6, D, generator=g), torch.randn(4, D, generator=g)
    kind = (torch.arange(M) % 3).to(I32)
    idx = torch.where(kind == 1, torch.arange(M) % 6, torch.arange(M) % 4).to(I32)
    xf, xv = output(M, D, None, dev)
    ops.f32_embed_merge(operand(table, None, dev), operand(proj, D + ldp, dev), vec(kind, dev), vec(idx, dev), xv, M, D)
    sync()
    want = torch.zeros(M, D)
    for m in range(M):
        if kind[m] == 1:
            want[m] = table[idx[m]]
        elif kind[m] == 2:
            want[m] = proj[idx[m]]
    same_bits(owed(xf, M, D, "embed_merge"), want, f"embed_merge {case_id(c)}")


Fsmn = collections.namedtuple("Fsmn", "B T D ksize ldv lens")
FSMN_CASES = [Fsmn(3, 9, 130, 11, 7, (0, 1, 9)), Fsmn(2, 1, 256, 11, 0, (1, 0)), Fsmn(3, 14, 300, 4, 600, (14, 5, 13)), Fsmn(1, 30, 50, 11, 0, (30,))]


def fsmn_inputs(c):
    g = gen(37, c.B, c.T, c.D, c.ksize)
    return dict(v=torch.randn(c.B * c.T, c.D, generator=g), w=torch.randn(c.D, c.ksize, generator=g),
                out0=torch.randn(c.B * c.T, c.D, generator=g), lens=torch.tensor(c.lens, dtype=I32), case=c)


def fsmn_reference(d):
    c = d["case"]
    B, T, D, ks = c.B, c.T, c.D, c.ksize
    left = (ks - 1) // 2
    v, w, o0 = d["v"].to(F64).view(B, T, D), d["w"].to(F64), d["out0"].to(F64).view(B, T, D)
    ref, E = o0.clone(), torch.zeros(B, T, D, dtype=F64)
    for b in range(B):
        n = c.lens[b]
        for t in range(n):
            r, A = v[b, t].clone(), v[b, t].abs()
            for j in range(ks):
                tt = t + j - left
                if 0 <= tt < n:
                    r, A = r + w[:, j] * v[b, tt], A + (w[:, j] * v[b, tt]).abs()
            ref[b, t] = o0[b, t] + r
            E[b, t] = (ks + 2) * e * (A + o0[b, t].abs())
    return Ref({"out": (ref.view(B * T, D), E.view(B * T, D))}, {})


def run_fsmn(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    of, ov = output(c.B * c.T, c.D, None, dev, init=d["out0"])
    ops.f32_fsmn(operand(d["v"], c.D + c.ldv, dev), c.D + c.ldv, dev(torch.cat([d["w"].reshape(-1), nan(GUARD)]))[:c.D * c.ksize].view(c.D, c.ksize),
                 vec(d["lens"], dev), ov, c.B, c.T, c.D, c.ksize)
    sync()
    return {"out": owed(of, c.B * c.T, c.D, "fsmn")}


# ------------------------------------------------------------------------------------------------ attention
def attn_rows(q, k, v, allow, scale, NT, NW):
    """q [R, Q, 128], k / v [n, 128], allow [Q, n] bool (float64): (o, E) [R, Q, 128]; a query without a visible key: 0, E = 0"""
    s, A = (q @ k.t()) * scale, (q.abs() @ k.abs().t()) * scale
    s = s.masked_fill(~allow, -math.inf)
    m = s.amax(-1, keepdim=True)
    dead = torch.isinf(m)
    m = torch.where(dead, torch.zeros_like(m), m)
    dd = torch.where(allow, s - m, torch.zeros_like(s))
    assert float(dd.min()) >= -40.0, float(dd.min())
    p = torch.where(allow, torch.exp(dd), torch.zeros_like(s))
    S = p.sum(-1, keepdim=True)
    P = p / torch.where(dead, torch.ones_like(S), S)
    delta = e * (2 + dd.abs() + 21 * A)
    n = allow.sum(-1, keepdim=True).to(F64)
    depth = torch.ceil(n / NT) + torch.ceil(n / NW) + 2 * NW + 9
    rel = delta + (P * delta).sum(-1, keepdim=True) + e * depth
    return P @ v, (P * rel) @ v.abs()


Pre = collections.namedtuple("Pre", "B S H G mode kstart klen profile")
# mode causal: keys [kstart[b], s]; klen: keys [0, min(klen[b], S)) for the queries below it (H != G: the causal kernel's klen form,
# H = G: the bidirectional kernel)
PRE_CASES = ([Pre(2, 65, rep, 1, "causal", (0, 9), None, "n01") for rep in range(1, 9)]
             + [Pre(1, 63, 2 * rep, 2, "causal", (5,), None, "n01") for rep in (1, 3, 4, 5, 8)]
             + [Pre(1, S, 4, 2, "causal", (0,), None, "n01") for S in (1, 2, 63, 64, 129)]
             + [Pre(3, 64, 12, 2, "causal", (0, 63, 30), None, "peaked"), Pre(2, 257, 6, 1, "causal", (0, 256), None, "n01"),
                Pre(3, 40, 4, 2, "klen", None, (1, 21, 40), "n01"), Pre(2, 40, 6, 2, "klen", None, (43, 0), "n01"),
                Pre(4, 13, 3, 3, "klen", None, (0, 1, 13, 11), "n01"), Pre(5, 64, 2, 2, "klen", None, (0, 1, 64, 29, 67), "peaked"),
                Pre(2, 13, 1, 1, "klen", None, (16, 5), "n01")])
PRE_LONG = Pre(1, 2048, 8, 1, "causal", (0,), None, "n01")


def pre_inputs(c):
    g = gen(41, c.B, c.S, c.H, c.G)
    qkv = torch.randn(c.B * c.S, (c.H + 2 * c.G) * HD, generator=g)
    if c.profile == "peaked":
        qkv[:, :(c.H + c.G) * HD] *= 1.6
    return dict(qkv=qkv, case=c)


def pre_reference(d):
    c = d["case"]
    B, S, H, G = c.B, c.S, c.H, c.G
    rep = H // G
    x = d["qkv"].to(F64).view(B, S, H + 2 * G, HD)
    o, E = torch.zeros(B, S, H, HD, dtype=F64), torch.zeros(B, S, H, HD, dtype=F64)
    ar = torch.arange(S)
    for b in range(B):
        if c.mode == "causal":
            allow = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= c.kstart[b])
        else:
            hi = min(c.klen[b], S)
            allow = (ar[None, :] < hi) & (ar[:, None] < hi)
        step = max(1, (1 << 23) // (S * S))                      # heads per pass: bounds the [n, S, S] temporaries
        for h0 in range(0, H, step):
            for g in {h // rep for h in range(h0, min(H, h0 + step))}:
                lo, hi = max(h0, g * rep), min(h0 + step, (g + 1) * rep, H)
                oo, EE = attn_rows(x[b, :, lo:hi].transpose(0, 1), x[b, :, H + g], x[b, :, H + G + g], allow, HD ** -0.5, 256, 4)
                o[b, :, lo:hi], E[b, :, lo:hi] = oo.transpose(0, 1), EE.transpose(0, 1)
    return Ref({"out": (o.view(B * S, H * HD), E.view(B * S, H * HD))}, {})


def run_pre(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    of, ov = output(c.B * c.S, c.H * HD, None, dev)
    ks = vec(torch.tensor(c.kstart, dtype=I32), dev) if c.kstart is not None else None
    kl = vec(torch.tensor(c.klen, dtype=I32), dev) if c.klen is not None else None
    ops.f32_attn_prefill(operand(d["qkv"], None, dev), ks, ov, c.B, c.S, c.H, c.G, HD ** -0.5, klen=kl)
    sync()
    return {"out": owed(of, c.B * c.S, c.H * HD, f"attn_prefill {case_id(c)}")}


Dec = collections.namedtuple("Dec", "H G nb ctx rows profile")       # rows: (kstart, lens) per beam row
DEC_VISIBLE = (1, 7, 64, 65, 128, 129, 256, 257, 321, 328)
_DEC_ROWS = tuple((0, n) for n in DEC_VISIBLE) + ((0, 0), (7, 328), (300, 329), (329, 329), (4, 4 + 321), (9, 5))
DEC_CASES = ([Dec(rep, 1, 4, 336, _DEC_ROWS, "n01") for rep in range(1, 9)]
             + [Dec(8, 2, 4, 336, _DEC_ROWS[6:], "peaked"), Dec(10, 2, 2, 330, ((0, 321), (2, 2), (1, 258)), "n01")])
DEC_LONG = Dec(8, 1, 1, 2048, ((0, 2048),), "n01")


def wave_shares(n, NW=8):
    """the keys each decode wave sums in phase 2 (f32_attn_group: qn = ceil(n / NW))"""
    qn = cdiv(n, NW)
    return [min(n, min(n, w * qn) + qn) - min(n, w * qn) for w in range(NW)]


def dec_inputs(c):
    M, Wd = len(c.rows), c.G * HD
    g = gen(43, c.H, c.G, c.ctx, M)
    qkv = nan(M, (c.H + 2 * c.G) * HD)
    qkv[:, :c.H * HD] = torch.randn(M, c.H * HD, generator=g) * (1.6 if c.profile == "peaked" else 1.0)
    kc, vc = nan(M, c.ctx, Wd), nan(M, c.ctx, Wd)
    index = torch.arange(M, dtype=I32)[:, None].repeat(1, c.ctx)
    for m, (lo, hi) in enumerate(c.rows):
        if hi <= lo:
            continue
        u0 = m // c.nb * c.nb                                     # the utterance's beam rows: the index scatters over them
        nrows = min(c.nb, M - u0)
        index[m, lo:hi] = (u0 + torch.randint(0, nrows, (hi - lo,), generator=g)).to(I32)
        rows, pos = index[m, lo:hi].long(), torch.arange(lo, hi)
        fresh = torch.isnan(kc[rows, pos, 0])
        kc[rows[fresh], pos[fresh]] = torch.randn(int(fresh.sum()), Wd, generator=g) * (1.6 if c.profile == "peaked" else 1.0)
        vc[rows[fresh], pos[fresh]] = torch.randn(int(fresh.sum()), Wd, generator=g)
    return dict(qkv=qkv, kc=kc, vc=vc, index=index, kstart=torch.tensor([r[0] for r in c.rows], dtype=I32),
                lens=torch.tensor([r[1] for r in c.rows], dtype=I32), case=c)


def dec_reference(d):
    c = d["case"]
    M, H, G, rep = len(c.rows), c.H, c.G, c.H // c.G
    q = d["qkv"][:, :H * HD].to(F64).view(M, H, HD)
    o, E = torch.zeros(M, H, HD, dtype=F64), torch.zeros(M, H, HD, dtype=F64)
    for m, (lo, hi) in enumerate(c.rows):
        if hi <= lo:
            continue
        rows, pos = d["index"][m, lo:hi].long(), torch.arange(lo, hi)
        k, v = d["kc"][rows, pos].to(F64).view(-1, G, HD), d["vc"][rows, pos].to(F64).view(-1, G, HD)
        assert not bool(torch.isnan(k).any() | torch.isnan(v).any())
        for g in range(G):
            oo, EE = attn_rows(q[m, g * rep:(g + 1) * rep, None], k[:, g], v[:, g], torch.ones(1, hi - lo, dtype=torch.bool), HD ** -0.5, 512, 8)
            o[m, g * rep:(g + 1) * rep], E[m, g * rep:(g + 1) * rep] = oo[:, 0], EE[:, 0]
    return Ref({"out": (o.view(M, -1), E.view(M, -1))}, {})


def run_dec(ops, d, dev=ident, sync=lambda: None, index=None, lens=None):
    c = d["case"]
    M = len(c.rows)
    of, ov = output(M, c.H * HD, None, dev)
    kc, vc = (dev(torch.cat([t, nan(GUARD, c.ctx, c.G * HD)])) for t in (d["kc"], d["vc"]))
    ops.f32_attn_decode(operand(d["qkv"], None, dev), kc, vc, operand(d["index"] if index is None else index, None, dev), vec(d["kstart"], dev),
                        vec(d["lens"] if lens is None else lens, dev), ov, M, c.H, c.G, c.ctx, HD ** -0.5)
    sync()
    return {"out": owed(of, M, c.H * HD, f"attn_decode {case_id(c)}")}


# ------------------------------------------------------------------------------------------------ cross-entropy
Ce = collections.namedtuple("Ce", "V ld dl aux")                 # dl: none | two | inplace; aux: row_argmax / row_lse given
CE_CASES = [Ce(V, ld, dl, aux) for (V, ld) in ((1, 0), (1023, 0), (1024, 3), (1025, 0), (4097, 7))
            for (dl, aux) in (("two", True), ("inplace", False), ("none", True))]
CE_M = 9


def ce_inputs(c):
    """rows: labels -100, 0, V - 1, V, V + 5, mid; row 6: tied maxima (the first column wins); rows 7 / 8 peaked, 8 at its label"""
    V, M = c.V, CE_M
    g = gen(47, V, c.ld)
    x = torch.randn(M, V, generator=g) * 1.5
    lab = torch.tensor([-100, 0, V - 1, V, V + 5, V // 2, V // 3, 0, V // 2], dtype=I32)
    if V > 8:
        x[6, V // 5], x[6, V - 2], x[6, V // 2] = 9.0, 9.0, 9.0
        x[7, V - 3] = 25.0
        x[8, V // 2] = 28.0
    assert float((x.max(-1).values - x.min(-1).values).max()) <= 40.0
    return dict(x=x, labels=lab, inv=torch.tensor([1.0 / 7]), case=c)


def ce_reference(d):
    c = d["case"]
    V, M = c.V, CE_M
    x, lab = d["x"].to(F64), d["labels"].long()
    on = (lab >= 0) & (lab < V)
    m = x.amax(-1, keepdim=True)
    dj = x - m
    p = torch.exp(dj)
    S = p.sum(-1, keepdim=True)
    P = p / S
    lse = m + torch.log(S)
    depth = cdiv(V, 1024) + 6 + 16
    E_lse = e * lse.abs() + 4 * e * torch.log(S).abs() + 2 * e + e * depth + (P * e * (dj.abs() + 2)).sum(-1, keepdim=True)
    xl = x.gather(1, torch.where(on, lab, torch.zeros_like(lab))[:, None])
    loss = torch.where(on[:, None], lse - xl, torch.zeros_like(lse))
    E_loss = torch.where(on[:, None], E_lse + e * loss.abs(), torch.zeros_like(lse))
    am = torch.stack([torch.nonzero(x[r] == m[r])[0, 0] for r in range(M)]).to(I32)
    ref = Ref({"row_loss": (loss, E_loss)}, {"row_hit": (on & (am.long() == lab)).to(I32)})
    if c.aux:
        ref.exact["row_argmax"] = am
        ref.tol["row_lse"] = (lse, E_lse)
    if c.dl != "none":
        k = torch.where(on, d["inv"].to(F64).expand(M), torch.zeros(M, dtype=F64))[:, None]
        pp = torch.exp(x - lse)
        gq = k * (pp - (torch.arange(V)[None, :] == lab[:, None]).to(F64))
        Eg = k * pp * (E_lse + e * (x - lse).abs() + 2 * e) + 2 * e * gq.abs()
        pad = torch.zeros(M, c.ld, dtype=F64)
        ref.tol["dlogits"] = (torch.cat([gq, pad], 1), torch.cat([Eg, pad], 1))
    return ref


def run_ce(ops, d, dev=ident, sync=lambda: None):
    c = d["case"]
    V, M, ld = c.V, CE_M, c.V + c.ld
    lf = nan(M + GUARD, ld)
    lf[:M, :V] = d["x"]                                          # (pad columns of the logits NaN: never read)
    lf = dev(lf)
    rl, rh = dev(nan(M + GUARD)), dev(torch.full((M + GUARD,), -7, dtype=I32))
    ra = dev(torch.full((M + GUARD,), -7, dtype=I32)) if c.aux else None
    rs = dev(nan(M + GUARD)) if c.aux else None
    dl = None if c.dl == "none" else (lf if c.dl == "inplace" else dev(nan(M + GUARD, ld)))
    ops.f32_ce(lf[:M], vec(d["labels"], dev), M, V, rl, rh, row_argmax=ra, row_lse=rs, dlogits=dl, inv_count=dev(d["inv"]) if dl is not None else None)
    sync()
    out = {}
    for name, t in (("row_loss", rl), ("row_hit", rh), ("row_argmax", ra), ("row_lse", rs), ("dlogits", dl)):
        if t is None:
            continue
        t = t.cpu()
        assert untouched(t[M:]), f"ce {case_id(c)}: {name} rows >= M were written"
        out[name] = t[:M].reshape(M, -1) if t.dtype == F32 else t[:M]
    if c.dl == "none":
        same_bits(lf.cpu()[:M, :V], d["x"], "ce without dlogits: the logits")
    return out


# ------------------------------------------------------------------------------------------------ the older metric (for the mutant table)
def old_metric(got, ref):
    """max |a - b| / max |b| over the whole tensor: what tests/test_gpu_fp32_ops.py asserts (< 1e-5; GEMMs < 2e-5)"""
    got, ref = got.to(F64), ref.to(F64)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
