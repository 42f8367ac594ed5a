"""TEST HELPER (not a test, never shipped): a plain float64 restatement of the bf16 attention operator -- forward, backward and
the rotary backward -- on the exact bf16 input values, with a first-order rounding-error bound for every element it returns.
Explicit softmax and matmuls, no fused library attention, nothing shared with the kernels or with tests/fake_ops.py.

Conventions: P is the masked, normalised softmax; a query row with no visible key has P = 0, o = 0 and lse = 0 (what
csrc/attention.hip writes); u = 2^-8 is the unit roundoff of bf16 under round-to-nearest-even.  Each bound mirrors one rounding
point of the kernels (P rounded to bf16 before P.V and P^T.dO, dS rounded to bf16, delta taken from the bf16 `out`, outputs rounded
to bf16; dq is rounded twice, before and after the rotation):

    o      = P v                              Eo   = u (P|v| + |o|)
    delta  = sum_d do.o                       Edl  = sum_d |do| Eo
    dp     = do v^T ;  ds = P (dp - delta)    Eds  = u|ds| + P.Edl
    dq_rot = scale . ds k                     Edq  = scale . Eds|k| + u|dq_rot|
    dv     = sum_heads P^T do                 Edv  = u sum_heads P^T|do| + u|dv|
    dk_rot = scale sum_heads ds^T q           Edk  = scale sum_heads Eds^T|q|
    inverse rotation (x1 c + x2 s, x2 c - x1 s) of dq_rot, dk_rot:
                                              E'   = (E1|c| + E2|s|, E2|c| + E1|s|) + u|result|
    lse    = m + log sum exp(s - m)           Else = (128 + 3) 2^-24 (A + |lse| + 1),  A_i = scale max_j sum_d |q_id k_jd|
                                                     (j over the keys row i sees)

`assert_within(got, ref, E, limit)` holds a result to |got - ref| <= limit . E on EVERY element (where E = 0 the result must be
exactly 0) and names the worst element when it fails.  LIMIT = 1.1 is derived, not measured: the bound is rigorous to first order,
and the 10 % covers the fp32 accumulation (worst at the longest sequence the kernels serve: 4096 . 2^-24 / 2^-8 = 6 %) and the
relative error of lse (about 1e-5) that enters every P of the backward.

The module also holds the case list the CPU and the GPU file share (CASES), the seeded inputs of a case (make_inputs) and the
run of the torch double on them (run_double)."""
import collections
import math

import torch

HD = 128
U = 2.0 ** -8
LIMIT = 1.1
F64 = torch.float64
BF = torch.bfloat16

Ref = collections.namedtuple("Ref", "out E_out lse E_lse dqkv E_dqkv")


def _unrotate(x, E, c, s):
    """inverse rotate-half rotation of x [S, n, 128] with its bound; c, s [S, 1, 64]"""
    x1, x2, E1, E2 = x[..., :64], x[..., 64:], E[..., :64], E[..., 64:]
    r = torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], -1)
    Er = torch.cat([E1 * c.abs() + E2 * s.abs(), E2 * c.abs() + E1 * s.abs()], -1) + U * r.abs()
    return r, Er


def reference(qkv, key_mask, dout, cos, sin, B, S, H, G, scale, causal):
    """qkv [M, (H+2G)*128] bf16 (rotated), key_mask [B, Spad] uint8, dout [M, H*128] bf16, cos / sin [M, 64] fp32.
    Returns Ref: out [B, S, H, 128], lse [B, S, H, 1], dqkv [B, S, H+2G, 128] (the gradient of the UNROTATED q | k | v), each
    with its bound tensor, float64."""
    rep = H // G
    x = qkv.view(B, S, H + 2 * G, HD).to(F64)
    dO = dout.view(B, S, H, HD).to(F64)
    km = key_mask.view(B, -1)[:, :S].bool()
    cs, sn = cos.view(B, S, 1, 64).to(F64), sin.view(B, S, 1, 64).to(F64)
    tri = torch.tril(torch.ones(S, S, dtype=torch.bool)) if causal else None
    out, E_out = torch.zeros(B, S, H, HD, dtype=F64), torch.zeros(B, S, H, HD, dtype=F64)
    lse, E_lse = torch.zeros(B, S, H, 1, dtype=F64), torch.zeros(B, S, H, 1, dtype=F64)
    d, E_d = torch.zeros(B, S, H + 2 * G, HD, dtype=F64), torch.zeros(B, S, H + 2 * G, HD, dtype=F64)
    chunk = max(1, min(rep, (1 << 21) // (S * S)))               # heads per pass: bounds the [n, S, S] temporaries
    for b in range(B):
        allow = km[b][None, :].expand(S, S)
        if causal:
            allow = allow & tri
        hide = ~allow
        for g in range(G):
            k, v = x[b, :, H + g], x[b, :, H + G + g]           # [S, 128]
            ak, av = k.abs(), v.abs()
            dk, Edk = torch.zeros(S, HD, dtype=F64), torch.zeros(S, HD, dtype=F64)
            dv, Adv = torch.zeros(S, HD, dtype=F64), torch.zeros(S, HD, dtype=F64)
            for h0 in range(g * rep, (g + 1) * rep, chunk):
                h1 = min(h0 + chunk, (g + 1) * rep)
                n = h1 - h0
                q, do = x[b, :, h0:h1].transpose(0, 1), dO[b, :, h0:h1].transpose(0, 1)      # [n, S, 128]
                sc = (q @ k.t()) * scale
                sc.masked_fill_(hide, -math.inf)
                m = sc.amax(-1, keepdim=True)
                dead = torch.isinf(m)
                m = torch.where(dead, torch.zeros_like(m), m)
                P = torch.exp(sc - m)
                l = P.sum(-1, keepdim=True)
                l = torch.where(dead, torch.ones_like(l), l)
                P /= l
                ls = torch.where(dead, torch.zeros_like(m), m + torch.log(l))
                A = scale * (q.abs() @ ak.t()).masked_fill_(hide, 0.0).amax(-1, keepdim=True)
                lse[b, :, h0:h1] = ls.transpose(0, 1)
                E_lse[b, :, h0:h1] = ((128 + 3) * 2.0 ** -24 * (A + ls.abs() + 1)).transpose(0, 1)
                o = P @ v
                Eo = U * (P @ av + o.abs())
                out[b, :, h0:h1], E_out[b, :, h0:h1] = o.transpose(0, 1), Eo.transpose(0, 1)
                delta = (do * o).sum(-1, keepdim=True)
                Edl = (do.abs() * Eo).sum(-1, keepdim=True)
                ds = P * (do @ v.t() - delta)
                Eds = U * ds.abs() + P * Edl
                dq = scale * (ds @ k)
                Edq = scale * (Eds @ ak) + U * dq.abs()
                d[b, :, h0:h1], E_d[b, :, h0:h1] = _unrotate(dq.transpose(0, 1), Edq.transpose(0, 1), cs[b], sn[b])
                Pt, dst, Edst = (t.reshape(n * S, S).t() for t in (P, ds, Eds))
                dv += Pt @ do.reshape(n * S, HD)
                Adv += Pt @ do.abs().reshape(n * S, HD)
                dk += scale * (dst @ q.reshape(n * S, HD))
                Edk += scale * (Edst @ q.abs().reshape(n * S, HD))
            dkr, Edkr = _unrotate(dk[:, None], Edk[:, None], cs[b], sn[b])
            d[b, :, H + g], E_d[b, :, H + g] = dkr[:, 0], Edkr[:, 0]
            d[b, :, H + G + g], E_d[b, :, H + G + g] = dv, U * Adv + U * dv.abs()
    return Ref(out, E_out, lse, E_lse, d, E_d)


# ------------------------------------------------------------------------------------------------ the checker
Check = collections.namedtuple("Check", "ok rms worst message")


def check_within(got, ref, E, limit, what=""):
    """got / ref / E [B, S, heads, D].  ok: every element finite with |got - ref| <= limit . E (E = 0: got exactly 0);
    rms: rms(err / E) over the elements with E > 0; worst: the largest err / E (inf for a non-finite value or a non-zero where
    E = 0); message: the worst element, for a failure report."""
    got = got.to(F64)
    assert got.shape == ref.shape == E.shape, (what, got.shape, ref.shape, E.shape)
    err = (got - ref).abs()
    pos = E > 0
    ratio = torch.where(pos, err / torch.where(pos, E, torch.ones_like(E)), torch.zeros_like(E))
    rms = float(ratio[pos].pow(2).mean().sqrt()) if bool(pos.any()) else 0.0
    score = torch.where(pos, ratio, torch.where(err > 0, torch.full_like(E, math.inf), torch.zeros_like(E)))
    score = torch.where(torch.isfinite(got), score, torch.full_like(E, math.inf))
    bad = score > limit
    worst = float(score.max()) if score.numel() else 0.0
    i = int(score.argmax())
    idx = []
    for n in reversed(got.shape):
        idx.append(i % n)
        i //= n
    b, s, h, dd = reversed(idx)
    message = (f"{what}: {int(bad.sum())} of {got.numel()} elements outside {limit} x E; worst at (b={b}, s={s}, head={h}, d={dd}): "
               f"got {float(got[b, s, h, dd])!r}, reference {float(ref[b, s, h, dd])!r}, bound E {float(E[b, s, h, dd]):.3e}, "
               f"|err| / E = {worst:.3f}; token {s} lies in query / key tile {s // 64} (rows {s // 64 * 64}-{s // 64 * 64 + 63}, "
               f"row {s % 64} of it)")
    return Check(not bool(bad.any()), rms, worst, message)


def assert_within(got, ref, E, limit, what=""):
    """check_within that raises, naming the worst element; returns rms(err / E)."""
    c = check_within(got, ref, E, limit, what)
    assert c.ok, c.message
    return c.rms


def blocks(dqkv, ref, B, S, H, G):
    """(name, got, ref, E) of the q, k and v blocks of a finished dqkv [M, (H+2G)*128], for a separate report each"""
    g4 = dqkv.view(B, S, H + 2 * G, HD)
    for name, lo, hi in (("dq", 0, H), ("dk", H, H + G), ("dv", H + G, H + 2 * G)):
        yield name, g4[:, :, lo:hi], ref.dqkv[:, :, lo:hi], ref.E_dqkv[:, :, lo:hi]


# ------------------------------------------------------------------------------------------------ cases and inputs
Case = collections.namedtuple("Case", "B S H G mask causal profile dense")

# the smallest shapes at which each mechanism can fail (not the workload's shapes)
SHAPES_SHORT = [(2, 1, 4, 2),            # one key
                (2, 63, 8, 2),           # 4 heads per group, short tile
                (3, 65, 16, 2),          # 8 heads per group, one row in the second tile
                (3, 64, 2, 1),           # exact tile
                (1, 19, 6, 2), (2, 100, 4, 2), (2, 130, 10, 2), (1, 70, 28, 4),      # 3, 2, 5, 7 heads per group
                (2, 128, 4, 4),          # H = G: the GQA kernel refuses, the policy takes the per-head kernels
                (2, 256, 12, 2),         # the single-pass limit
                (1, 257, 4, 2),          # first Spad the single-pass kernels refuse; 5 tiles on a 4-slot ring
                (2, 300, 12, 2)]         # more tiles than ring slots
SHAPES_LONG = [(1, 628, 12, 2),          # more tiles than ring slots
               (1, 1100, 4, 2),          # 18 tiles
               (1, 4096, 2, 1),          # the GQA kernel's mask table full
               (1, 4097, 2, 1)]          # past it: kernel = GQA is a bad argument, the policy takes the per-head kernels


def _cases():
    out = []
    for B, S, H, G in SHAPES_SHORT:
        for mask in ("right", "left", "none", "holes", "empty0"):
            if mask == "empty0" and B < 2:
                continue
            for causal in (True, False):
                out.append(Case(B, S, H, G, mask, causal, "n01", False))
                if mask in ("none", "left"):
                    out.append(Case(B, S, H, G, mask, causal, "peaked", False))
            if mask in ("right", "left"):
                out.append(Case(B, S, H, G, mask, True, "n01", True))
    for B, S, H, G in SHAPES_LONG:
        # (one sequence per batch: make_mask's "right" pads nothing here, so "holes" is the long shapes' masked-key case)
        out += [Case(B, S, H, G, "none", True, "n01", False), Case(B, S, H, G, "right", True, "n01", False),
                Case(B, S, H, G, "none", False, "n01", False), Case(B, S, H, G, "holes", True, "n01", False)]
    return out


CASES = _cases()


def case_id(c):
    return f"{c.B}x{c.S}x{c.H}x{c.G}-{c.mask}-{'causal' if c.causal else 'bidir'}-{c.profile}-{'dense' if c.dense else 'live'}"


def make_mask(B, S, kind):
    """right / left / none: as tests/test_gpu_ops.py::make_mask; holes: every third key off, phase b % 3; empty0: batch row 0
    with no visible key at all"""
    Spad = (S + 63) // 64 * 64
    m = torch.zeros(B, Spad, dtype=torch.uint8)
    for b in range(B):
        n = S - (b * 7) % max(S // 2, 1)
        if kind == "right":
            m[b, :n] = 1
        elif kind == "left":
            m[b, S - n:S] = 1
        elif kind == "holes":
            m[b, :S] = (torch.arange(S) % 3 != b % 3).to(torch.uint8)
        elif kind == "empty0":
            m[b, :S] = 0 if b == 0 else 1
        else:
            m[b, :S] = 1
    return m


def make_inputs(c):
    """Seeded inputs of a case: dict(qkv, km, dout, cos, sin) + the scalars.  N(0, 1) everywhere; "peaked": the q and k blocks
    x 3 (a near one-hot softmax: the forward's online rescale, the backward's large lse); dout zeroed on the rows of masked
    tokens as in the model unless `dense`; cos / sin: the fp32 rotary table of positions 0 .. S-1."""
    B, S, H, G = c.B, c.S, c.H, c.G
    M, LD = B * S, (H + 2 * G) * HD
    gen = torch.Generator().manual_seed(1000 * S + 10 * H + G)
    qkv = torch.randn(M, LD, generator=gen)
    if c.profile == "peaked":
        qkv[:, :(H + G) * HD] *= 3.0
    qkv = qkv.to(BF)
    km = make_mask(B, S, c.mask)
    dout = torch.randn(M, H * HD, generator=gen).to(BF)
    if not c.dense:
        dout.view(B, S, H * HD)[~km[:, :S].bool()] = 0
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.float32) / HD))
    ang = torch.arange(S, dtype=torch.float32).repeat(B)[:, None] * inv[None]
    return dict(qkv=qkv, km=km, dout=dout, cos=ang.cos(), sin=ang.sin(), B=B, S=S, H=H, G=G, scale=HD ** -0.5, causal=c.causal)


def reference_of(inp):
    return reference(inp["qkv"], inp["km"], inp["dout"], inp["cos"], inp["sin"], inp["B"], inp["S"], inp["H"], inp["G"], inp["scale"],
                     inp["causal"])


def run_double(fake, inp, km_bwd=None, dout_bwd=None):
    """forward -> attn_bwd_fused of the torch double (tests/fake_ops.py) on the inputs: (out [M, H*128] bf16, lse [B, H, Spad],
    dqkv [M, (H+2G)*128] bf16).  km_bwd / dout_bwd: another key mask / dout for the backward only (the mutants of the CPU file)."""
    B, S, H, G = inp["B"], inp["S"], inp["H"], inp["G"]
    M, LD, Spad = B * S, (H + 2 * G) * HD, (S + 63) // 64 * 64
    out, lse = torch.zeros(M, H * HD, dtype=BF), torch.zeros(B * H * Spad)
    fake.attn_fwd(inp["qkv"], None, inp["km"], out, lse, B, S, H, G, inp["scale"], inp["causal"])
    dqkv = torch.zeros(M, LD, dtype=BF)
    fake.attn_bwd_fused(inp["qkv"], inp["km"] if km_bwd is None else km_bwd, inp["dout"] if dout_bwd is None else dout_bwd, out, lse,
                        torch.zeros(B * H * Spad), inp["cos"], inp["sin"], dqkv, torch.zeros(M, H * HD), torch.zeros(M, H * HD),
                        B, S, H, G, inp["scale"], inp["causal"])
    return out, lse, dqkv


def lse_rows(lse, B, S, H):
    """lse [B, H, Spad] -> the rows < S as [B, S, H, 1]"""
    return lse.view(B, H, -1)[:, :, :S].permute(0, 2, 1).unsqueeze(-1)


def double_rms(fake, inp, ref):
    """rms(err / E) of the torch double on the inputs: dict(out, dq, dk, dv) -- the yardstick of the kernels' second check"""
    B, S, H, G = inp["B"], inp["S"], inp["H"], inp["G"]
    out, _, dqkv = run_double(fake, inp)
    r = {"out": check_within(out.view(B, S, H, HD), ref.out, ref.E_out, LIMIT).rms}
    for name, got, want, E in blocks(dqkv, ref, B, S, H, G):
        r[name] = check_within(got, want, E, LIMIT).rms
    return r
