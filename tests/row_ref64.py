"""TEST HELPER (not a test, never shipped): plain float64 restatements of the bf16 step's ROW-REDUCTION kernels -- RMSNorm and
LayerNorm forward / backward and the column sums (csrc/norm.hip), the fused cross-entropy and its reduction (csrc/ce.hip), the
softmax pair of the cross-attention projector (csrc/cross_attn.hip), the row softmax and the PSD statistics / gather
(csrc/encoder_aux.hip) -- on the exact input values, each with a first-order bound E for every element it returns.  Nothing is
shared with the kernels or with tests/fake_ops.py.  `check_within` / `Check` are those of tests/attn_ref64.py, U = 2^-8 and
RMS_RATIO = 1.5 those of tests/decode_ref64.py; e = 2^-24 is the unit roundoff of fp32.

RULES.  A bf16 output has E = u |ref| + A, an fp32 output E = A, A the fp32 allowance below; an integer output, and any output
whose A is 0 (a max of the inputs, a pad column, a row behind a -1 entry, the exact-integer profiles), must have the reference's
value exactly.  LIMIT = 1.0: every allowance is inside E.  A fixed-order sum of n terms t_i carries depth . e . sum |t_i|, depth
the longest chain of fp32 additions a term passes through in THAT kernel (serial adds per lane, 6 shuffle levels per wave, the
serial adds over waves / slabs / row lanes); where a kernel has several forms the larger depth is taken.  The bounds of cancelling
results (x - mean, dp - sum P dp, p - 1 at the label, w dy - x^ dot) are absolute.

Constants.  An fp32 +, *, / : e relative.  rsqrtf: 2 ulp = 4 e.  expf (cross_attn.hip, encoder_aux.hip; the correctly reduced
library function): 1 ulp = 2 e, and its argument x - m, the difference of two inputs up to 40 apart, e |x - m| absolute, which the
exponential turns into as much relative: a term of a softmax sum carries e (|d| + 3), d = x - m (the product with 1 / sum
included).  __expf (ce.hip; exp2 of the scaled argument): e (4 |d| + 4), the form derived for the decode attention
(tests/decode_ref64.py, e_j).  __logf of a sum S >= 1: 4 e |log S| + 2 e absolute.

    RMSNorm forward      ss = sum x^2: 4 ceil(D / 256) serial adds per lane + 6 shuffle levels + the product = depth_ss;
      (norm.hip)         rstd = rsqrtf(ss / D + eps):  A_r = rstd e (depth_ss / 2 + 5)     (half the sum's relative error, the
                         division and the addition, rsqrtf);  y = bf16(w (x rstd)):  A_y = |y| (A_r / rstd + 2 e)
    RMSNorm backward     rstd is an INPUT.  dot = sum (w dy) x rstd / D: three products per term, the same summation,
                         E_dot = (depth + 4) e sum |w dy x rstd| / D  (the generic form multiplies ((w dy) x) rstd, the register
                         form (w dy) first and reuses it: three roundings either way, the larger depth is the same);
                         dx = base + rstd (w dy - x rstd dot):
                         A_dx = rstd (3 e |w dy| + 4 e |x rstd dot| + |x rstd| E_dot) + e |dx|;   dx_bf16: u |dx| + A_dx
    LayerNorm forward    two passes.  depth_s = max(16, 4 ceil(D / 1024)) + 11 (wave kernel: 16 serial + 6 levels; block kernel:
                         4 per 1024-column step, a tail step, 6 levels, 4 waves);  E_mu = (depth_s + 1) e sum |x| / D;
                         q = sum (x - mu)^2:  E_q = 2 E_mu sum |x - mu| + (depth_s + 3) e q;  v = q / D + eps,
                         E_v = E_q / D + 2 e v;  rstd: E_r = rstd (E_v / (2 v) + 4 e);
                         y = (x - mu) rstd g + b:  A_y = |g| (|d| E_r + rstd E_mu + 2 e |d| rstd) + e |d rstd g| + e |y|
    layernorm_bwd_params dgamma = sum_r dy x^, x^ = (x - mean) rstd (mean, rstd INPUTS): ceil(R / 16) serial adds per slab, 16
                         slabs in order: A = (ceil(R / 16) + 16 + 3) e sum |dy x^|;  dbeta: (ceil(R / 16) + 16) e sum |dy|
    colsum               16 row lanes of ceil(R / 16) serial adds, 16 LDS adds: A = (ceil(R / 16) + 16) e sum |x|
    cross-entropy        lse = m + log S, S = sum exp(x - m).  ce_reg_kernel (dlogits given, no argmax buffer, V >= 8192,
                         ldv / 8 <= 20480): exact max, depth = 8 ceil(nv / 1024) + 6 + 16.  ce_kernel: a running (max, sum) per
                         thread, rescaled by __expf when the max moves (at most once per chunk: n_r = ceil(nv / 256) times, each
                         6 e: the exponential's constant, the product and the rounding of its argument), 8 more combine levels
                         of the same kind: depth = 8 n_r + 8, rescales 6 (n_r + 8) e.  The arguments of all the exponentials a
                         term passes telescope to d_j = m - x_j.
                         E_lse = e |lse| + 4 e |log S| + 2 e + e (depth + rescales) + sum_j P_j e (4 d_j + 4);
                         row_loss = lse - x_label: E_lse + e |loss|;  g = bf16((__expf(x - lse) - [c = label]) inv_count):
                         A_g = inv_count p (E_lse + e (4 |x - lse| + 4)) + 2 e |g|, absolute (p - 1 cancels at a peaked label)
    ce_reduce            ceil(M / 256) serial + 6 + 4: out[0] = sum loss / c: ((depth + 1) e sum |loss|) / c; hits and count are
                         integers below 2^24: out[1] = h / c: e h / c, out[2] = c exact, out[3] = 1 / c: e / c
    scale_softmax_rows   t = bf16(fp32(s) / denom) is reproduced exactly (IEEE division, round to nearest even): stats[0] = max t
                         has the reference's bits.  depth = 8 ceil(V / 2048) + 11;  rel_inv = e (depth + 1) + sum_j P_j e (|d_j|
                         + 3);  stats[1] = 1 / sum: inv rel_inv;  p = bf16(expf(t - m) inv): u p + p (e (|d| + 3) + rel_inv + e)
    softmax_bwd_rows     stats are INPUTS.  P = expf(t - m) inv: A_P = P e (|d| + 4);  dot = sum P dp: depth = ceil(V / 256) + 10,
                         E_dot = sum |P dp| e (|d| + 5 + depth);  q = P (dp - dot): A_q = P (E_dot + e |dp - dot|) + A_P |dp -
                         dot| + e |q|;  ds = bf16(bf16(q) / denom): u |ds| + (1 + u) (u |q| + A_q) / denom + e |ds|
    softmax_rows         depth = ceil(V / 256) + 10; y = expf(x - m) / sum (fp32): y (e (|d| + 3) + rel_inv + e)
    psd_logit_stats      one pass, a (max, sum) per thread rescaled by expf when the max moves: at most n_c = ceil(V / 2048) + 1
                         times and once more to the row's max, each 4 e; depth = 8 ceil(V / 2048) + 11;
                         rel_inv = e (depth + 1 + 4 (n_c + 1)) + sum_j P_j e (2 d_j + 3);  fstat = (m exact, inv rel_inv);
                         fblank = expf(x_blank - m) inv: (e (|d| + 3) + rel_inv + e) fblank;  fid: first index of the maximum
    psd_gather_softmax   fstat is an INPUT.  out = sum_t expf(x_t - m_t) inv_t / len: sum_t P_t e (|d_t| + 4 + len) / len + e out

Every logit row keeps max - min <= 40 (asserted by `logit_rows`): every exponential and product is a normal fp32 number.

The module also holds the case lists, the seeded inputs and the runs (`run_*`: NaN-filled outputs and workspaces, guard rows that
must keep their bits) that tests/test_row_ref64_cpu.py (through the torch double) and tests/test_gpu_row_f64.py (through HipOps)
share."""
import collections
import math

import torch

from attn_ref64 import Check, assert_within, check_within  # noqa: F401  (one checker for all the float64 reference modules)
from decode_ref64 import RMS_RATIO, U  # noqa: F401

e = 2.0 ** -24
LIMIT = 1.0
EPS_RMS, EPS_LN = 1e-6, 1e-5
LN_SPLIT = 16                                                    # TASU_LN_BWD_SPLIT of include/tasu_hip.h
F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
NAN = float("nan")

Ref = collections.namedtuple("Ref", "tol exact")               # tol: name -> (ref, E) float64 [R, C]; exact: name -> tensor (its bits)


def cdiv(a, b):
    return (a + b - 1) // b


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))


def nan(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype)


def bits(t):
    return t.contiguous().view({BF: torch.int16, F32: torch.int32, I32: torch.int32}[t.dtype])


def untouched(t):
    """every element still holds the NaN bits (integers: the -7 pattern) it was filled with"""
    fill = torch.full_like(t, -7) if t.dtype == I32 else torch.full_like(t, NAN)
    return torch.equal(bits(t), bits(fill))


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not torch.equal(bits(got), bits(want)):
        bad = torch.nonzero(bits(got) != bits(want))
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ from the exact result, first at {i}: "
                             f"got {got[i].item()!r}, reference {want[i].item()!r}")


def check(got, ref, what, limit=LIMIT):
    """one run's outputs (name -> CPU tensor) against a Ref: the bits of `exact`, limit x E on `tol`; returns the largest |err| / E"""
    worst = 0.0
    for name, want in ref.exact.items():
        same_bits(got[name], want, f"{what} {name}")
    for name, (want, E) in ref.tol.items():
        g = got[name].reshape(want.shape)
        c = check_within(g.reshape(1, want.shape[0], 1, -1), want.reshape(1, want.shape[0], 1, -1), E.reshape(1, want.shape[0], 1, -1),
                         limit, f"{what} {name} (s = row, d = column)")
        assert c.ok, c.message
        worst = max(worst, c.worst)
    return worst


def worst_of(got, ref):
    """the largest |err| / E without raising (inf for a wrong bit): the mutants' score"""
    w = 0.0
    for name, want in ref.exact.items():
        if not torch.equal(bits(got[name]), bits(want)):
            w = math.inf
    for name, (want, E) in ref.tol.items():
        n = want.shape[0]
        w = max(w, check_within(got[name].reshape(1, n, 1, -1), want.reshape(1, n, 1, -1), E.reshape(1, n, 1, -1), LIMIT).worst)
    return w


def rms_stat(got, want, E):
    """the second check's statistic of a bf16 output: rms(err / (u |ref|)) over the elements whose fp32 allowance A = E - u |ref|
    is at most a tenth of u |ref|; (rms, count)"""
    mag = U * want.abs()
    keep = (mag > 0) & (E - mag <= 0.1 * mag)
    n = int(keep.sum())
    if n == 0:
        return 0.0, 0
    return float((((got.to(F64).reshape(want.shape) - want).abs() / mag.clamp_min(1e-300))[keep]).pow(2).mean().sqrt()), n


def walk_columns(D, chunk=256, lane_w=4):
    """the columns a one-hot profile walks over: both ends of the first vector, of the first chunk, the row's last vector, and
    the first column of the last lane's vector in every chunk's last position"""
    cols = {0, 1, 3, 4, 255, 256, 257, D - 4, D - 1, chunk - lane_w + chunk * ((D - 1) // chunk), chunk - lane_w + chunk * ((D - 1) // chunk - 1)}
    return sorted(c for c in cols if 0 <= c < D)


def logit_rows(x):
    """asserts max - min <= 40 on every row: no exponential underflows to a subnormal"""
    xf = x.to(F64)
    assert float((xf.amax(-1) - xf.amin(-1)).max()) <= 40.0, "a logit row spans more than 40"
    return x


def first_argmax(x):
    """first index of the row maximum of [R, V]"""
    V = x.shape[-1]
    m = x.amax(-1, keepdim=True)
    return torch.where(x == m, torch.arange(V).expand_as(x), torch.full_like(x, V, dtype=torch.long)).amin(-1)


def _call(ops, to):
    """(ops, to) of a run: `to` moves an input / a NaN-filled output to where `ops` computes (identity for the torch double)"""
    return ops, (to or (lambda t: t))


def _back(*ts):
    if any(t is not None and t.is_cuda for t in ts):
        torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in ts]


GUARD = 3                                                        # guard rows behind every row-major output


# ================================================================================================ RMSNorm forward
RmsCase = collections.namedtuple("RmsCase", "form M D profile")
RMS_D = [4, 252, 256, 260, 512, 1028, 1536, 3584]


def _rms_fwd_cases():
    out = [RmsCase("plain", M, D, "n01") for D in RMS_D for M in (1, 64, 65, 67)]
    out += [RmsCase("plain", 0, D, "onehot") for D in RMS_D]
    out += [RmsCase("plain", 5, D, "scaled") for D in (256, 260, 3584)]
    out += [RmsCase("ld", M, D, "n01") for D in (256, 260, 3584) for M in (1, 67)]
    out += [RmsCase("frag", M, D, "n01") for D in (256, 512, 1536) for M in (1, 17, 64)]
    out += [RmsCase("rows", n, D, "n01") for D in (256, 260, 1536) for n in (6, 70)]
    return out


RMS_FWD_CASES = _rms_fwd_cases()


def case_id(c):
    return "-".join(str(v) for v in c)


def _rms_x(M, D, profile, seed):
    g = gen(M, D, seed)
    if profile == "onehot":
        cols = walk_columns(D)
        x = torch.zeros(len(cols), D)
        x[torch.arange(len(cols)), torch.tensor(cols)] = 2.0 ** (torch.arange(len(cols)) % 5 - 2).to(F32)
        return x
    x = torch.randn(M, D, generator=g)
    if profile == "scaled":                                     # rows x 2^-10, x 2^10, all zero, as they are
        x[0] *= 2.0 ** -10
        x[1] *= 2.0 ** 10
        x[2] = 0
    return x


def rms_fwd_inputs(c):
    x = _rms_x(c.M, c.D, c.profile, 1)
    M = x.shape[0]
    d = dict(x=x, w=1 + 0.1 * torch.randn(c.D, generator=gen(c.D, 2)), M=M, D=c.D, form=c.form, src=None, n=M)
    if c.form == "rows":                                         # -1 entries, a duplicated source row, n no multiple of 4
        n = c.M
        d["x"] = _rms_x(n + 3, c.D, "n01", 3)
        src = (torch.arange(n) * 5) % (n + 3)
        src[1::4] = -1
        src[3] = src[0]
        d["src"], d["n"], d["M"] = src.to(I32), n, n + 3
    return d


def rms_depth(D):
    return 4 * cdiv(D, 256) + 6 + 1


def rms_fwd_reference(d):
    x, w, D = d["x"].to(F64), d["w"].to(F64), d["D"]
    if d["src"] is not None:
        ok = (d["src"] >= 0).to(F64)[:, None]
        x = x[d["src"].long().clamp_min(0)]
    else:
        ok = torch.ones(x.shape[0], 1, dtype=F64)
    r = (x.pow(2).mean(-1, keepdim=True) + EPS_RMS).rsqrt() * ok
    rel_r = e * (rms_depth(D) / 2 + 5)
    y = w * x * r
    return Ref({"rstd": (r, r * rel_r), "y": (y, U * y.abs() + y.abs() * (rel_r + 2 * e))}, {})


def run_rms_fwd(ops, d, to=None, frag_attr=None):
    """y, rstd (None where the form has none) of one RMSNorm forward; `frag_attr`: the object whose dec_frag selects the layout"""
    ops, to = _call(ops, to)
    n, D, form = d["n"], d["D"], d["form"]
    x, w = to(d["x"]), to(d["w"])
    rstd = to(nan(n + GUARD))
    if form == "frag":
        y = to(nan(64 + GUARD, D, dtype=BF))
        ops.dec_frag = True
        try:
            ops.dec_rmsnorm(x, w, y, EPS_RMS)
        finally:
            ops.dec_frag = False
        (y,) = _back(y)
        return {"y_raw": y, "rstd": None}
    ldy = D + 64 if form == "ld" else D
    buf = to(nan(n + GUARD, ldy, dtype=BF))
    if form == "rows":
        ops.rmsnorm_fwd_rows(x, to(d["src"]), w, buf[:n], rstd[:n], EPS_RMS)
    else:
        ops.rmsnorm_fwd(x, w, buf[:n, :D], rstd[:n], EPS_RMS)
    buf, rstd = _back(buf, rstd)
    assert untouched(buf[n:]) and untouched(buf[:, D:]) and untouched(rstd[n:]), f"rmsnorm_fwd {form}: guard rows / columns were written"
    return {"y": buf[:n, :D], "rstd": rstd[:n, None]}


# ================================================================================================ RMSNorm backward
BwdCase = collections.namedtuple("BwdCase", "form M D acc bf profile")


def _rms_bwd_cases():
    out, k = [], 0
    for D in RMS_D:
        for M in (1, 5, 64, 65, 67):
            out.append(BwdCase("plain", M, D, k & 1, (k >> 1) & 1, "n01"))
            k += 1
    out += [BwdCase("plain", 5, D, acc, bf, "scaled") for D in (256, 260, 3584) for acc in (0, 1) for bf in (0, 1)]
    out += [BwdCase("plain", 0, D, 0, 1, "onehot") for D in RMS_D]
    out += [BwdCase(form, M, D, 0, bf, "n01") for form in ("rows", "resid") for D in (256, 260, 1536, 3584) for M, bf in ((7, 1), (67, 0))]
    return out


RMS_BWD_CASES = _rms_bwd_cases()


def rms_bwd_inputs(c):
    x = _rms_x(c.M, c.D, c.profile, 4)
    M, D = x.shape[0], c.D
    w = 1 + 0.1 * torch.randn(D, generator=gen(D, 5))
    slot = None
    nc = M
    if c.form != "plain":                                        # every third row behind a -1; the others permuted into compact rows
        live = [m for m in range(M) if m % 3 != 0]
        nc = len(live)
        slot = torch.full((M,), -1, dtype=I32)
        slot[torch.tensor(live)] = torch.randperm(nc, generator=gen(M, 6)).to(I32)
    g = gen(M, D, 7)
    dy = torch.randn(nc, D, generator=g).to(BF)
    xs = x.to(F64)
    rfull = (xs.pow(2).mean(-1) + EPS_RMS).rsqrt().to(F32)      # an input: the kernel and the reference get the same fp32 values
    rstd = rfull if slot is None else torch.zeros(nc).index_put_((slot[slot >= 0].long(),), rfull[slot >= 0])
    return dict(x=x, w=w, dy=dy, rstd=rstd, slot=slot, M=M, D=D, form=c.form, acc=c.acc, bf=c.bf,
                base=torch.randn(M, D, generator=g) if c.acc else None,
                resid=torch.randn(nc, D, generator=g) if c.form == "resid" else None)


def rms_bwd_reference(d):
    x, w, D, M = d["x"].to(F64), d["w"].to(F64), d["D"], d["M"]
    if d["slot"] is None:
        ok, s = torch.ones(M, 1, dtype=F64), torch.arange(M)
    else:
        ok, s = (d["slot"] >= 0).to(F64)[:, None], d["slot"].long().clamp_min(0)
    dy, r = d["dy"].to(F64)[s], d["rstd"].to(F64)[s][:, None]
    base = d["base"].to(F64) if d["base"] is not None else (d["resid"].to(F64)[s] if d["resid"] is not None else torch.zeros(M, D, dtype=F64))
    t1 = w * dy
    xr = x * r
    dot = (t1 * xr).sum(-1, keepdim=True) / D
    E_dot = (rms_depth(D) + 4) * e * (t1 * xr).abs().sum(-1, keepdim=True) / D
    t2 = xr * dot
    dx = (base + r * (t1 - t2)) * ok
    A = (r * (3 * e * t1.abs() + 4 * e * t2.abs() + xr.abs() * E_dot) + e * dx.abs()) * ok
    tol = {"dx": (dx, A)}
    if d["bf"]:
        tol["dx_bf16"] = (dx, U * dx.abs() + A)
    return Ref(tol, {})


def run_rms_bwd(ops, d, to=None):
    ops, to = _call(ops, to)
    M, D = d["M"], d["D"]
    dx = nan(M + GUARD, D)
    if d["acc"]:
        dx[:M] = d["base"]
    dx, dxb = to(dx), to(nan(M + GUARD, D, dtype=BF)) if d["bf"] else None
    args = [to(d["dy"]), to(d["x"]), to(d["w"]), to(d["rstd"])]
    b = None if dxb is None else dxb[:M]
    if d["form"] == "plain":
        ops.rmsnorm_bwd(*args, dx[:M], b, bool(d["acc"]))
    elif d["form"] == "rows":
        ops.rmsnorm_bwd_rows(*args, to(d["slot"]), dx[:M], b)
    else:
        ops.rmsnorm_bwd_rows_resid(*args, to(d["slot"]), to(d["resid"]), dx[:M], b)
    dx, dxb = _back(dx, dxb)
    assert untouched(dx[M:]) and (dxb is None or untouched(dxb[M:])), "rmsnorm_bwd: guard rows were written"
    out = {"dx": dx[:M]}
    if dxb is not None:
        out["dx_bf16"] = dxb[:M]
    return out


# ================================================================================================ LayerNorm forward
LnCase = collections.namedtuple("LnCase", "R D ldx ldy off f32 stats profile")


def _ln_cases():
    out, k = [], 0
    shapes = [(4, 4, 4, 0), (512, 512, 512, 0), (560, 560, 576, 0), (1020, 1020, 1020, 0), (1024, 1024, 1024, 0),    # wave kernel
              (1028, 1028, 1028, 0), (203, 256, 256, 0),                                                            # block: vector body + tail
              (1027, 1027, 1027, 0), (512, 512, 512, 1)]                                                            # block: scalar body
    for D, ldx, ldy, off in shapes:
        for profile in ("n01", "offset", "posterior"):
            for f32 in (0, 1):
                out.append(LnCase(5, D, ldx, ldy, off, f32, k % 3 != 0, profile))
                k += 1
    out += [LnCase(R, D, D, D, 0, f32, 1, "n01") for R in (1, 4) for D in (512, 1028) for f32 in (0, 1)]
    out += [LnCase(0, D, D, D, 0, 0, 1, "onehot") for D in (512, 1028)]
    out += [LnCase(3, 25055, 25088, 25088, 0, f32, 1, p) for f32, p in ((0, "posterior"), (1, "n01"), (0, "offset"))]
    return out


LN_CASES = _ln_cases()


def ln_inputs(c):
    D = c.D
    g = gen(c.R, D, c.off, 11)
    if c.profile == "onehot":
        cols = walk_columns(D, 1024)
        xs = torch.zeros(len(cols), D)
        xs[torch.arange(len(cols)), torch.tensor(cols)] = 2.0 ** (torch.arange(len(cols)) % 5 - 2).to(F32)
    elif c.profile == "posterior":                               # the rows of tests/test_gpu_ops.py::test_layernorm
        xs = torch.randn(c.R, D, generator=g).abs() * 0.01
        xs[torch.arange(c.R), torch.arange(c.R) % D] += 0.9
    else:
        xs = torch.randn(c.R, D, generator=g) + (1000.0 if c.profile == "offset" else 0.0)
    R = xs.shape[0]
    buf = nan(R * c.ldx + c.off + 4)                             # pad columns of x hold NaN; `off` elements in front: x 4 bytes in
    x = buf[c.off:c.off + R * c.ldx].view(R, c.ldx)
    x[:, :D] = xs
    return dict(x=x, xbuf=buf, gamma=1 + 0.1 * torch.randn(D, generator=g), beta=0.1 * torch.randn(D, generator=g), R=R, D=D, ldx=c.ldx,
                ldy=c.ldy, off=c.off, f32=c.f32, stats=c.stats)


def ln_depth(D):
    return max(16, 4 * cdiv(D, 1024)) + 11


def ln_stats64(xs, D):
    """(mu, q, v, rstd, E_mu, E_r) of float64 rows [R, D]"""
    mu = xs.mean(-1, keepdim=True)
    E_mu = (ln_depth(D) + 1) * e * xs.abs().sum(-1, keepdim=True) / D
    dd = xs - mu
    q = dd.pow(2).sum(-1, keepdim=True)
    E_q = 2 * E_mu * dd.abs().sum(-1, keepdim=True) + (ln_depth(D) + 3) * e * q
    v = q / D + EPS_LN
    r = v.rsqrt()
    return mu, r, E_mu, r * ((E_q / D + 2 * e * v) / (2 * v) + 4 * e)


def ln_reference(d):
    D, R = d["D"], d["R"]
    xs, ga, be = d["x"][:, :D].to(F64), d["gamma"].to(F64), d["beta"].to(F64)
    mu, r, E_mu, E_r = ln_stats64(xs, D)
    dd = xs - mu
    y = dd * r * ga + be
    A = ga.abs() * (dd.abs() * E_r + r * E_mu + 2 * e * dd.abs() * r) + e * (dd * r * ga).abs() + e * y.abs()
    yp, Ep = torch.zeros(R, d["ldy"], dtype=F64), torch.zeros(R, d["ldy"], dtype=F64)   # pad columns: exactly 0
    yp[:, :D], Ep[:, :D] = y, (A if d["f32"] else U * y.abs() + A)
    tol = {"y": (yp, Ep)}
    if d["stats"]:
        tol["mean"], tol["rstd"] = (mu, E_mu), (r, E_r)
    return Ref(tol, {})


def run_ln(ops, d, to=None):
    ops, to = _call(ops, to)
    R, D = d["R"], d["D"]
    xb = to(d["xbuf"])
    x = xb[d["off"]:d["off"] + R * d["ldx"]].view(R, d["ldx"])
    y = to(nan(R + GUARD, d["ldy"], dtype=F32 if d["f32"] else BF))
    mean, rstd = (to(nan(R + GUARD)), to(nan(R + GUARD))) if d["stats"] else (None, None)
    ops.layernorm_fwd(x, to(d["gamma"]), to(d["beta"]), y[:R], None if mean is None else mean[:R], None if rstd is None else rstd[:R], R, D, EPS_LN)
    y, mean, rstd = _back(y, mean, rstd)
    assert untouched(y[R:]), "layernorm_fwd: guard rows were written"
    out = {"y": y[:R]}
    if d["stats"]:
        assert untouched(mean[R:]) and untouched(rstd[R:]), "layernorm_fwd: statistics past R were written"
        out["mean"], out["rstd"] = mean[:R, None], rstd[:R, None]
    return out


# ================================================================================================ layernorm_bwd_params, colsum
ColCase = collections.namedtuple("ColCase", "op R C profile")
LNB_CASES = [ColCase("lnb", R, D, p) for R in (1, LN_SPLIT - 1, LN_SPLIT, LN_SPLIT + 1, 70) for D in (203, 256, 560) for p in ("n01", "exact")]
COLSUM_CASES = [ColCase("colsum", R, C, p) for R in (1, 15, 16, 17, 333) for C in (1, 31, 32, 33, 200, 203) for p in ("n01", "exact")]


def col_inputs(c):
    R, C = c.R, c.C
    ld = (C + 1) // 2 * 2 + 8                                    # even, larger than C
    g = gen(R, C, 21)
    dy = nan(R, ld, dtype=BF)
    dy[:, :C] = (torch.randint(-8, 9, (R, C), generator=g).to(F32) if c.profile == "exact" else torch.randn(R, C, generator=g)).to(BF)
    d = dict(op=c.op, R=R, C=C, ld=ld, dy=dy, profile=c.profile)
    if c.op == "lnb":
        x = nan(R, ld)
        x[:, :C] = torch.randn(R, C, generator=g) * 2 + 0.5
        mu, r, _, _ = ln_stats64(x[:, :C].to(F64), C)
        d.update(x=x, mean=mu[:, 0].to(F32), rstd=r[:, 0].to(F32))   # inputs: the same fp32 values for the kernel and the reference
    return d


def col_reference(d):
    R, C = d["R"], d["C"]
    dy = d["dy"][:, :C].to(F64)
    depth = cdiv(R, 16) + 16
    tol, exact = {}, {}
    s = dy.sum(0, keepdim=True)
    name = "dbeta" if d["op"] == "lnb" else "out"
    if d["profile"] == "exact":                                  # integers below 2^24: exact in fp32 in any order
        exact[name] = s[0].to(F32)
    else:
        tol[name] = (s, depth * e * dy.abs().sum(0, keepdim=True))
    if d["op"] == "lnb":
        t = dy * (d["x"][:, :C].to(F64) - d["mean"].to(F64)[:, None]) * d["rstd"].to(F64)[:, None]
        tol["dgamma"] = (t.sum(0, keepdim=True), (depth + 3) * e * t.abs().sum(0, keepdim=True))
    return Ref(tol, exact)


def run_col(ops, d, to=None):
    ops, to = _call(ops, to)
    R, C = d["R"], d["C"]
    if d["op"] == "colsum":
        out = to(nan(C + 8))
        ops.colsum(to(d["dy"]), out[:C], R, C)
        (out,) = _back(out)
        assert untouched(out[C:]), "colsum: elements past C were written"
        return {"out": out[:C]}
    dg, db, ws = to(nan(C + 8)), to(nan(C + 8)), to(nan(2 * LN_SPLIT * C + 8))
    ops.layernorm_bwd_params(to(d["dy"]), to(d["x"]), to(d["mean"]), to(d["rstd"]), dg[:C], db[:C], ws, R, C)
    dg, db, ws = _back(dg, db, ws)
    assert untouched(dg[C:]) and untouched(db[C:]) and untouched(ws[2 * LN_SPLIT * C:]), "layernorm_bwd_params: wrote past D / past its workspace"
    return {"dgamma": dg[:C], "dbeta": db[:C]}


# ================================================================================================ cross-entropy
CeCase = collections.namedtuple("CeCase", "M V ldv argmax dl profile")    # dl: "two" buffers, "inplace", None (no gradient)
REG_CHUNKS = 1024 * 20


def ce_kernel_of(c):
    """which kernel tasu_ce_fwd_bwd launches (csrc/ce.hip)"""
    return "reg" if c.dl and not c.argmax and c.ldv // 8 <= REG_CHUNKS and c.V >= 8192 else "online"


def _ce_cases():
    out = []
    for V, ldv, am, dl in [(5, 8, 0, "two"), (8, 8, 0, "two"), (1000, 1024, 0, "two"), (1000, 1024, 1, "inplace"), (2048, 2048, 0, "two"),
                           (2056, 2056, 0, "inplace"), (2056, 2056, 1, "two"), (8200, 8200, 1, "two"), (9001, 9088, 0, None),
                           (8192, 8192, 0, "two"), (8200, 8200, 0, "inplace"), (9001, 9088, 0, "two"), (9001, 9088, 0, "inplace")]:
        out += [CeCase(6, V, ldv, am, dl, p) for p in ("n01", "peak", "ties")]
    out += [CeCase(3, 151936, 151936, 1, "two", "n01"), CeCase(2, 163841, 163848, 0, "two", "n01"),           # ce_kernel
            CeCase(3, 151936, 151936, 0, "inplace", "n01"), CeCase(3, 151936, 151936, 0, "two", "peak"),      # ce_reg_kernel
            CeCase(3, 163840, 163840, 0, "inplace", "n01"), CeCase(3, 163840, 163840, 0, "two", "ties")]
    return out


CE_CASES = _ce_cases()


def tie_pairs(V, stride):
    """column pairs that hold a duplicated maximum: two lanes of one wave, two waves, two chunks of one thread (`stride` threads
    per row); those that fit under V"""
    pairs = [(8 * 3 + 1, 8 * 40 + 2), (8 * 5, 8 * 200 + 7), (8 * 7 + 3, 8 * (7 + stride) + 3)]
    return [(a, b) for a, b in pairs if b < V] or [(0, V - 1)]


def peak_rows(M, V, stride):
    """rows of the peaked profile: one per walked column where the row is short enough to afford them"""
    return max(M, len(walk_columns(V, 8 * stride, 8))) if V < 100000 else M


def _logits(M, V, profile, stride, g):
    if profile == "peak":                                        # one logit 30 above a flat row, the column walking
        x = torch.full((M, V), -2.0)
        cols = walk_columns(V, 8 * stride, 8)
        peak = torch.tensor([cols[m % len(cols)] for m in range(M)])
        x[torch.arange(M), peak] = 28.0
        return x.to(BF), peak
    x = (torch.randn(M, V, generator=g) * 3).to(BF)
    if profile == "ties":
        top = x.float().amax(-1)
        pairs = tie_pairs(V, stride)
        for m in range(M - 1):
            a, b = pairs[m % len(pairs)]
            x[m, a] = x[m, b] = (top[m] + 1).to(BF)
        x[M - 1] = x[M - 1, 0]                                   # a constant row: argmax 0
    return x, None


def ce_inputs(c):
    M, V, ldv = c.M, c.V, c.ldv
    g = gen(M, V, ldv, 31)
    stride = 1024 if ce_kernel_of(c) == "reg" else 256
    if c.profile == "peak":
        M = peak_rows(M, V, stride)
    x, peak = _logits(M, V, c.profile, stride, g)
    logit_rows(x)
    arg = first_argmax(x.to(F64))
    lab = torch.randint(0, V, (M,), generator=g)
    lab[0] = arg[0]                                              # the argmax of the row (peaked: p - 1 cancels)
    lab[1] = V - 1
    if M > 2:
        lab[2] = -100
    if M > 3:
        lab[3], lab[4] = 0, (V - 1) // 8 * 8                     # column 0; the first column of the (partly padded) last chunk
    if c.profile == "peak":
        lab[5::2] = arg[5::2]                                    # more labels on a walking peak
    lg = nan(M, ldv, dtype=BF)                                   # pad columns [V, ldv) hold NaN
    lg[:, :V] = x
    cnt = float((lab >= 0).sum())
    return dict(logits=lg, labels=lab.to(I32), M=M, V=V, ldv=ldv, argmax=c.argmax, dl=c.dl, inv=torch.tensor([1.0 / cnt]), kernel=ce_kernel_of(c))


def ce_reference(d):
    M, V, ldv = d["M"], d["V"], d["ldv"]
    x = d["logits"][:, :V].to(F64)
    lab = d["labels"].long()
    live = lab >= 0
    m = x.amax(-1, keepdim=True)
    dj = m - x
    p = torch.exp(-dj)
    S = p.sum(-1, keepdim=True)
    lse = m + S.log()
    nv = ldv // 8
    if d["kernel"] == "reg":
        order = 8 * cdiv(nv, 1024) + 6 + 16
    else:
        n_r = cdiv(nv, 256)
        order = 8 * n_r + 8 + 6 * (n_r + 8)
    E_lse = e * lse.abs() + 4 * e * S.log() + 2 * e + e * order + (p / S * e * (4 * dj + 4)).sum(-1, keepdim=True)
    xl = x.gather(1, lab.clamp_min(0)[:, None])
    loss = torch.where(live[:, None], lse - xl, torch.zeros_like(lse))
    arg = first_argmax(x)
    tol = {"row_loss": (loss, torch.where(live[:, None], E_lse + e * loss.abs(), torch.zeros_like(lse)))}
    exact = {"row_hit": (live & (arg == lab)).to(I32)}
    if d["argmax"]:
        exact["row_argmax"] = arg.to(I32)
    if d["dl"]:
        ic = float(d["inv"][0])
        P = torch.exp(x - lse)
        g = P.clone()
        g[torch.arange(M), lab.clamp_min(0)] -= 1.0
        g = g * ic * live[:, None]
        A = (ic * P * (E_lse + e * (4 * (x - lse).abs() + 4)) + 2 * e * g.abs()) * live[:, None]
        gp, Ep = torch.zeros(M, ldv, dtype=F64), torch.zeros(M, ldv, dtype=F64)            # pad columns, ignored rows: exactly 0
        gp[:, :V], Ep[:, :V] = g, U * g.abs() + A
        tol["dlogits"] = (gp, Ep)
    return Ref(tol, exact)


def run_ce(ops, d, to=None):
    ops, to = _call(ops, to)
    M, ldv = d["M"], d["ldv"]
    lg = torch.cat([d["logits"], nan(GUARD, ldv, dtype=BF)])
    moved = to(lg)
    lg = lg.clone() if moved is lg else moved
    rl, rh = to(nan(M + GUARD)), to(torch.full((M + GUARD,), -7, dtype=I32))
    ra = to(torch.full((M + GUARD,), -7, dtype=I32)) if d["argmax"] else None
    dl = None if d["dl"] is None else (lg[:M] if d["dl"] == "inplace" else to(nan(M + GUARD, ldv, dtype=BF)))
    ops.ce_fwd_bwd(lg[:M], to(d["labels"]), M, d["V"], rl[:M], rh[:M], None if ra is None else ra[:M], None if dl is None else dl[:M], to(d["inv"]) if dl is not None else None)
    rl, rh, ra, dl, lg = _back(rl, rh, ra, dl, lg)
    assert untouched(rl[M:]) and untouched(rh[M:]) and (ra is None or untouched(ra[M:])) and untouched(lg[M:]), "ce_fwd_bwd: rows past M were written"
    out = {"row_loss": rl[:M, None], "row_hit": rh[:M]}
    if ra is not None:
        out["row_argmax"] = ra[:M]
    if dl is not None:
        if d["dl"] == "two":
            assert untouched(dl[M:]), "ce_fwd_bwd: gradient rows past M were written"
            same_bits(lg[:M], d["logits"], "ce_fwd_bwd: the logits of a two-buffer call")
        out["dlogits"] = dl[:M]
    return out


RedCase = collections.namedtuple("RedCase", "M profile")
CE_REDUCE_CASES = [RedCase(M, p) for M in (1, 255, 256, 257, 4096) for p in ("n01", "exact")] + [RedCase(257, "ignored")]


def red_inputs(c):
    M = c.M
    g = gen(M, 41)
    lab = torch.randint(0, 100, (M,), generator=g).to(I32)
    lab[1::3] = -100
    if c.profile == "ignored":
        lab[:] = -100
    live = lab >= 0
    loss = (torch.randint(0, 256, (M,), generator=g).to(F32) / 16 if c.profile == "exact" else torch.randn(M, generator=g).abs() * 3) * live
    hit = (torch.randint(0, 2, (M,), generator=g) * live).to(I32)
    return dict(M=M, loss=loss, hit=hit, labels=lab, profile=c.profile)


def red_reference(d):
    l, h, c = float(d["loss"].to(F64).sum()), float(d["hit"].sum()), float((d["labels"] >= 0).sum())
    if c == 0:                                                   # the mean over nothing: 0 / 0
        return Ref({}, {"count": torch.tensor([0.0])})
    ref = torch.tensor([[l / c, h / c, c, 1 / c]], dtype=F64)
    if d["profile"] == "exact":                                  # every sum a dyadic below 2^24 units: exact in any order
        return Ref({}, {"out": (torch.tensor(l).to(F32) / torch.tensor(c).to(F32)).reshape(1).to(F32), "count": torch.tensor([c]),
                        "acc": (torch.tensor(h) / torch.tensor(c)).reshape(1).to(F32), "inv": (1 / torch.tensor(c)).reshape(1).to(F32)})
    depth = cdiv(d["M"], 256) + 10
    E = torch.tensor([[(depth + 1) * e * float(d["loss"].to(F64).abs().sum()) / c, e * h / c, 0.0, e / c]], dtype=F64)
    return Ref({"out4": (ref, E)}, {})


def run_red(ops, d, to=None):
    ops, to = _call(ops, to)
    out = to(nan(4 + GUARD))
    ops.ce_reduce(to(d["loss"]), to(d["hit"]), to(d["labels"]), d["M"], out[:4])
    (out,) = _back(out)
    assert untouched(out[4:]), "ce_reduce: wrote past its four outputs"
    return {"out4": out[None, :4], "out": out[0:1], "acc": out[1:2], "count": out[2:3], "inv": out[3:4]}


# ================================================================================================ the projector's softmax pair
SmCase = collections.namedtuple("SmCase", "R V ld off denom stats profile")
SQ96 = math.sqrt(96.0)


def _sm_cases():
    out, k = [], 0
    for V, ld in [(8, 8), (1000, 1024), (1003, 1008), (1003, 1003), (2048, 2048), (2056, 2056)]:
        for profile in ("n01", "peak", "ties"):
            for denom in ((8.0, SQ96) if ld in (1008, 2056) else ((8.0,) if k % 2 else (SQ96,))):
                out.append(SmCase(5, V, ld, 0, denom, k % 3 != 1, profile))
                k += 1
    out += [SmCase(1, 8, 8, 0, 8.0, 1, "n01"), SmCase(1, 1003, 1008, 0, SQ96, 0, "n01"), SmCase(5, 1000, 1024, 1, SQ96, 1, "n01"),
            SmCase(5, 2056, 2056, 1, 8.0, 1, "peak"), SmCase(1, 151936, 151936, 0, SQ96, 1, "n01"), SmCase(1, 151936, 151936, 0, 8.0, 1, "peak")]
    return out


SM_CASES = _sm_cases()


def sm_inputs(c):
    R, V, ld = peak_rows(c.R, c.V, 256) if c.profile == "peak" else c.R, c.V, c.ld
    g = gen(R, V, ld, c.off, 51)
    x, _ = _logits(R, V, c.profile, 256, g)
    s = (x.float() * 8.0).to(BF)                                 # the scores before the division (8: exact, t = x when denom = 8)
    t = (s.float() / torch.tensor(c.denom, dtype=F32)).to(BF)    # IEEE fp32 division, round to nearest even: the kernel's t, exactly
    logit_rows(t)
    buf = nan((R + GUARD) * ld + c.off + 8, dtype=BF)
    sv = buf[c.off:c.off + R * ld].view(R, ld)
    sv[:, :V] = s
    dp = nan(R, ld, dtype=BF)
    dp[:, :V] = torch.randn(R, V, generator=g).to(BF)
    t64 = t.to(F64)
    m = t64.amax(-1, keepdim=True)
    inv = 1.0 / torch.exp(t64 - m).sum(-1, keepdim=True)
    stats_in = torch.cat([m, inv], 1).to(F32)                    # the backward's input: the reference's statistics in fp32
    return dict(sbuf=buf, t=t, dp=dp, R=R, V=V, ld=ld, off=c.off, denom=c.denom, denom32=float(torch.tensor(c.denom, dtype=F32)), stats=c.stats, stats_in=stats_in)


def sm_reference(d):
    R, V, ld = d["R"], d["V"], d["ld"]
    t = d["t"].to(F64)
    m = t.amax(-1, keepdim=True)
    dj = m - t
    p = torch.exp(-dj)
    S = p.sum(-1, keepdim=True)
    P = p / S
    depth = 8 * cdiv(V, 2048) + 11
    rel_inv = e * (depth + 1) + (P * e * (dj + 3)).sum(-1, keepdim=True)
    pp, Ep = torch.zeros(R, ld, dtype=F64), torch.zeros(R, ld, dtype=F64)
    pp[:, :V], Ep[:, :V] = P, U * P + P * (e * (dj + 3) + rel_inv + e)
    fwd = {"p": (pp, Ep)}
    if d["stats"]:
        fwd["stats"] = (torch.cat([m, 1 / S], 1), torch.cat([torch.zeros_like(m), rel_inv / S], 1))
    # backward, on the fp32 statistics it is given
    mi, inv = d["stats_in"][:, 0:1].to(F64), d["stats_in"][:, 1:2].to(F64)
    Pb = torch.exp(t - mi) * inv
    A_P = Pb * e * (dj + 4)
    dp = d["dp"][:, :V].to(F64)
    dot = (Pb * dp).sum(-1, keepdim=True)
    E_dot = ((Pb * dp).abs() * e * (dj + 5 + cdiv(V, 256) + 10)).sum(-1, keepdim=True)
    q = Pb * (dp - dot)
    A_q = Pb * (E_dot + e * (dp - dot).abs()) + A_P * (dp - dot).abs() + e * q.abs()
    ds = q / d["denom32"]                                        # the fp32 value the kernel divides by
    dsp, Edp = torch.zeros(R, ld, dtype=F64), torch.zeros(R, ld, dtype=F64)
    dsp[:, :V], Edp[:, :V] = ds, U * ds.abs() + (1 + U) * (U * q.abs() + A_q) / d["denom32"] + e * ds.abs()
    return Ref(fwd, {}), Ref({"ds": (dsp, Edp)}, {})


def _sm_view(buf, d):
    return buf[d["off"]:d["off"] + d["R"] * d["ld"]].view(d["R"], d["ld"])


def run_sm_fwd(ops, d, to=None):
    ops, to = _call(ops, to)
    R, V, ld = d["R"], d["V"], d["ld"]
    p = to(nan(R + GUARD, ld, dtype=BF))
    stats = to(nan(R + GUARD, 2)) if d["stats"] else None
    ops.scale_softmax_rows(_sm_view(to(d["sbuf"]), d), p[:R], R, V, d["denom"], None if stats is None else stats[:R])
    p, stats = _back(p, stats)
    assert untouched(p[R:]) and (stats is None or untouched(stats[R:])), "scale_softmax_rows: rows past R were written"
    out = {"p": p[:R]}
    if stats is not None:
        out["stats"] = stats[:R]
    return out


def run_sm_bwd(ops, d, to=None):
    ops, to = _call(ops, to)
    R, V, ld = d["R"], d["V"], d["ld"]
    ds = to(nan(R + GUARD, ld, dtype=BF))
    ops.softmax_bwd_rows(_sm_view(to(d["sbuf"]), d), to(d["stats_in"]), to(d["dp"]), ds[:R], R, V, d["denom"])
    (ds,) = _back(ds)
    assert untouched(ds[R:]), "softmax_bwd_rows: rows past R were written"
    return {"ds": ds[:R]}


# ================================================================================================ softmax_rows
SrCase = collections.namedtuple("SrCase", "R V ld bf profile")
SR_CASES = [SrCase(5, V, ld, bf, p) for V, ld in [(1, 4), (203, 256), (256, 256), (257, 260)] for bf in (0, 1) for p in ("n01", "peak")] + \
           [SrCase(2, 25055, 25088, bf, "n01") for bf in (0, 1)]


def sr_inputs(c):
    g = gen(c.R, c.V, c.bf, 61)
    R = peak_rows(c.R, c.V, 32) if c.profile == "peak" else c.R  # (one column per thread and step: a "chunk" of 256 columns)
    xb, _ = _logits(R, c.V, c.profile, 32, g)
    xs = xb if c.bf else (torch.randn(R, c.V, generator=g) * 3 if c.profile == "n01" else xb.float())
    logit_rows(xs)
    x = nan(R, c.ld, dtype=BF if c.bf else F32)
    x[:, :c.V] = xs
    return dict(x=x, R=R, V=c.V, ld=c.ld)


def sr_reference(d):
    R, V, ld = d["R"], d["V"], d["ld"]
    x = d["x"][:, :V].to(F64)
    dj = x.amax(-1, keepdim=True) - x
    p = torch.exp(-dj)
    P = p / p.sum(-1, keepdim=True)
    rel_inv = e * (cdiv(V, 256) + 10 + 1) + (P * e * (dj + 3)).sum(-1, keepdim=True)
    y, E = torch.zeros(R, ld, dtype=F64), torch.zeros(R, ld, dtype=F64)
    y[:, :V], E[:, :V] = P, P * (e * (dj + 3) + rel_inv + e)
    return Ref({"y": (y, E)}, {})


def run_sr(ops, d, to=None):
    ops, to = _call(ops, to)
    R = d["R"]
    y = to(nan(R + GUARD, d["ld"]))
    ops.softmax_rows(to(d["x"]), y[:R], R, d["V"])
    (y,) = _back(y)
    assert untouched(y[R:]), "softmax_rows: rows past R were written"
    return {"y": y[:R]}


# ================================================================================================ PSD from the logits
PsdCase = collections.namedtuple("PsdCase", "V profile")
PSD_CASES = [PsdCase(V, p) for V in (8, 203, 2056, 25055) for p in ("n01", "late", "ties")]
PSD_B, PSD_T, PSD_BSTRIDE, PSD_TOUT = 2, 9, 11, 5
PSD_LENS = (9, 4)
PSD_SEGS = ([(0, 1), (1, 2), (3, 5), (8, 1)], [(0, 2), (2, 1), (3, 1)])      # (start, length) of the kept segments; new_lens 4 and 3 < Tout


def psd_inputs(c):
    V = c.V
    ld = cdiv(V, 8) * 8
    B, T, bs = PSD_B, PSD_T, PSD_BSTRIDE
    g = gen(V, 71)
    x, _ = _logits(B * bs, V, "ties" if c.profile == "ties" else "n01", 256, g)
    if c.profile == "late":                                      # the maximum arrives late: the last vector, the scalar tail, the last column
        cols = sorted({V - 1, (V & ~7) - 1 if V >= 8 else 0, min(V & ~7, V - 1), max(V - 9, 0)})
        for r in range(B * bs):
            x[r, cols[r % len(cols)]] = (x[r].float().amax() + 6).to(BF)
    logit_rows(x)
    lg = nan(B * bs, ld, dtype=BF)                               # pad columns, the rows past T of a batch and the frames past lens: NaN
    lg[:, :V] = x
    for b in range(B):
        lg[b * bs + PSD_LENS[b]:(b + 1) * bs] = NAN
    ss, sl = torch.zeros(B, T, dtype=I32), torch.zeros(B, T, dtype=I32)
    for b, segs in enumerate(PSD_SEGS):
        for j, (s0, n) in enumerate(segs):
            ss[b, j], sl[b, j] = s0, n
    x3 = lg.view(B, bs, ld)[:, :T, :V].to(F64)
    m = x3.amax(-1)
    inv = 1 / torch.exp(x3 - m[..., None]).sum(-1)
    live = torch.arange(T)[None] < torch.tensor(PSD_LENS)[:, None]
    fstat_in = torch.where(live[..., None], torch.stack([m, inv], -1), torch.zeros(B, T, 2, dtype=F64)).to(F32)   # the gather's input
    return dict(logits=lg, V=V, ld=ld, lens=torch.tensor(PSD_LENS, dtype=I32), seg_start=ss, seg_len=sl,
                new_lens=torch.tensor([len(s) for s in PSD_SEGS], dtype=I32), fstat_in=fstat_in, live=live)


def psd_reference(d):
    V, ld = d["V"], d["ld"]
    B, T, bs, Tout = PSD_B, PSD_T, PSD_BSTRIDE, PSD_TOUT
    live = d["live"].reshape(-1)
    x = d["logits"].view(B, bs, ld)[:, :T, :V].to(F64).reshape(B * T, V)
    x = torch.where(live[:, None], x, torch.zeros_like(x))
    m = x.amax(-1, keepdim=True)
    dj = m - x
    p = torch.exp(-dj)
    S = p.sum(-1, keepdim=True)
    n_c = cdiv(V, 2048) + 1
    rel_inv = e * (8 * cdiv(V, 2048) + 11 + 1 + 4 * (n_c + 1)) + (p / S * e * (2 * dj + 3)).sum(-1, keepdim=True)
    lv = live[:, None].to(F64)
    fstat = torch.cat([m, 1 / S], 1) * lv
    fb = p[:, 0:1] / S
    stats = Ref({"fstat": (fstat, torch.cat([torch.zeros_like(m), rel_inv / S], 1) * lv),
                 "fblank": (fb * lv, fb * (e * (dj[:, 0:1] + 3) + rel_inv + e) * lv)},
                {"fid": torch.where(live, first_argmax(x), torch.full((B * T,), -1)).to(I32)})
    # the gather, on the fp32 statistics it is given
    st = d["fstat_in"].to(F64)
    x3 = x.view(B, T, V)
    out, E = torch.zeros(B * Tout, ld, dtype=F64), torch.zeros(B * Tout, ld, dtype=F64)
    for b, segs in enumerate(PSD_SEGS):
        for j, (s0, n) in enumerate(segs):
            dd = x3[b, s0:s0 + n] - st[b, s0:s0 + n, 0:1]
            P = torch.exp(dd) * st[b, s0:s0 + n, 1:2]
            o = P.sum(0) / n
            out[b * Tout + j, :V], E[b * Tout + j, :V] = o, (P * e * (dd.abs() + 4 + n)).sum(0) / n + e * o
    return stats, Ref({"out": (out, E)}, {})


def run_psd_stats(ops, d, to=None):
    ops, to = _call(ops, to)
    n = PSD_B * PSD_T
    fid, fb, fs = to(torch.full((n + GUARD,), -7, dtype=I32)), to(nan(n + GUARD)), to(nan(2 * (n + GUARD)))
    ops.psd_logit_stats(to(d["logits"]), to(d["lens"]), fid[:n], fb[:n], fs[:2 * n], PSD_B, PSD_T, PSD_BSTRIDE, d["V"], 0)
    fid, fb, fs = _back(fid, fb, fs)
    assert untouched(fid[n:]) and untouched(fb[n:]) and untouched(fs[2 * n:]), "psd_logit_stats: wrote past B x T frames"
    return {"fid": fid[:n], "fblank": fb[:n, None], "fstat": fs[:2 * n].view(n, 2)}


def run_psd_gather(ops, d, to=None):
    ops, to = _call(ops, to)
    n = PSD_B * PSD_TOUT
    out = to(nan(n + GUARD, d["ld"]))
    ops.psd_gather_softmax(to(d["logits"]), to(d["fstat_in"].reshape(-1)), to(d["seg_start"].reshape(-1)), to(d["seg_len"].reshape(-1)),
                           to(d["new_lens"]), out[:n], PSD_B, PSD_T, PSD_BSTRIDE, PSD_TOUT, d["V"])
    (out,) = _back(out)
    assert untouched(out[n:]), "psd_gather_softmax: rows past B x Tout were written"
    return {"out": out[:n]}
