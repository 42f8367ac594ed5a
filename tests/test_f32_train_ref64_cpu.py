"""The float64 references of the fp32 training kernels (tests/f32_train_ref64.py) checked on the CPU: the plain-torch fp32
restatement (F32TrainTorch) stays within 1.0 x E on every case the GPU file runs (S = 2048 of the attention backward replaced by
S = 257; the 52-split cross-attention case kept); float64 autograd of each definition agrees with the hand-written float64
backward at 1e-12; the restated plan_splits agrees with tasu_f32_ca_workspace_floats on every case; the entry points refuse bad
pitches and shapes before any launch (the library loads without a GPU); and the mutants of the restatement -- the faults the older
tensor-wide metrics can miss -- score above 1.0 E (the MUTANT lines; DESIGN's section on the fp32 training kernels holds the table).
expf's allowance 2 e + e |d| is derived and emulated in tests/test_f32_ref64_cpu.py::test_expf_allowance_covers_the_contracted_expansion;
the sigmoid mutant below runs that emulation through the SwiGLU backward and must stay inside E."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import f32_train_ref64 as T

F64, F32, I32 = torch.float64, torch.float32, torch.int32
HD = T.HD
_worst = {}


@pytest.fixture(scope="module")
def dbl():
    return T.F32TrainTorch()


def hold(op, what, got, ref):
    w = T.check(got, ref, f"{op} {what}")
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST restatement {op} {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")
    return w


def agree(a, b, what):
    """two float64 forms of one definition: 1e-12 of the result's scale"""
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= 1e-12 * scale, (what, float((a - b).abs().max()), scale)


# ------------------------------------------------------------------------------------------------ the restatement within E
@pytest.mark.parametrize("case", T.RMSB_CASES, ids=T.case_id)
def test_restatement_rmsnorm_bwd(dbl, case):
    d = T.rmsb_inputs(case)
    got = T.run_rmsb(dbl, d)
    hold("rmsnorm_bwd", T.case_id(case), got, T.rmsb_reference(d))


def test_restatement_pointwise(dbl):
    for case in T.SWIB_CASES:
        d = T.swib_inputs(case)
        hold("swiglu_bwd", T.case_id(case), T.run_swib(dbl, d), T.swib_reference(d))
    for n in T.SILU_NS:
        d = T.silu_inputs(n)
        hold("silu", f"n = {n}", T.run_silu(dbl, d), T.silu_reference(d))
    for n in T.RELU_NS:
        T.run_relu(dbl, n)


@pytest.mark.parametrize("case", T.DROP_CASES, ids=T.case_id)
def test_restatement_lora_dropout(dbl, case):
    d = T.drop_inputs(case)
    hold("lora_dropout", T.case_id(case), T.run_drop(dbl, d), T.drop_reference(d))


def test_restatement_reductions_and_copies(dbl):
    for case in T.COLS_CASES:
        d = T.cols_inputs(case)
        hold("colsum", T.case_id(case), T.run_cols(dbl, d), T.cols_reference(d))
    for case in T.LNP_CASES:
        d = T.lnp_inputs(case)
        hold("layernorm_bwd_params", T.case_id(case), T.run_lnp(dbl, d), T.lnp_reference(d))
    for R in T.TR_SIZES:
        for C in T.TR_SIZES:
            for Rpad in T.tr_rpads(R):
                T.run_transpose(dbl, R, C, Rpad)
    for n, D, rows in T.GATHER_CASES:
        T.run_gather(dbl, n, D, rows)


@pytest.mark.parametrize("case", T.ATTB_CASES, ids=T.attb_id)
def test_restatement_attn_bwd(dbl, case):
    d = T.attb_inputs(case)
    hold("attn_bwd", T.attb_id(case), T.run_attb(dbl, d), T.attb_reference(d))


@pytest.mark.parametrize("dh", T.CA_DHS)
def test_restatement_ca_attn(dbl, dh):
    for case in T.ca_cases(dh) + ([T.CA_MANY] if dh == 16 else []):
        d = T.ca_inputs(case)
        fwd = T.run_ca(dbl, d)
        hold("ca_attn", T.case_id(case), fwd, T.ca_reference(d))
        out32, lse32 = T.ca_handed(d)
        hold("ca_attn_bwd", T.case_id(case), T.run_ca_bwd(dbl, d, out32, lse32), T.ca_bwd_reference(d, out32, lse32))
        hold("ca_attn_bwd_chain", T.case_id(case), T.run_ca_bwd(dbl, d, fwd["out"], fwd["lse"]), T.ca_bwd_reference(d))   # its own forward's out / lse


# ------------------------------------------------------------------------------------------------ the references against autograd
def test_row_references_against_float64_autograd():
    d = T.rmsb_inputs(T.Rmsb(3, 1025, "outlier", 0))
    x, w, dy = d["x"].to(F64).requires_grad_(True), d["w"].to(F64), d["dy"].to(F64)
    y = w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + T.EPS32))
    (gx,) = torch.autograd.grad(y, x, dy)
    agree(T.rmsb_reference(d).tol["dx"][0], gx, "rmsnorm_bwd")
    d1 = dict(d, case=T.Rmsb(3, 1025, "outlier", 1))
    agree(T.rmsb_reference(d1).tol["dx"][0], d["dx0"].to(F64) + gx, "rmsnorm_bwd, accumulate")

    c = T.Swib(3, 85)
    d = T.swib_inputs(c)
    keep = (d["gu"][:, :c.I].abs() <= 80).to(F64)                 # (float64 autograd of silu at +-100 is exact as well; the mask keeps the scale)
    gu = d["gu"].to(F64).requires_grad_(True)
    act = torch.nn.functional.silu(gu[:, :c.I]) * gu[:, c.I:]
    agree(T.swib_reference(d).tol["dgu"][0] * torch.cat([keep, keep], 1), torch.autograd.grad(act, gu, d["dact"].to(F64))[0] * torch.cat([keep, keep], 1), "swiglu_bwd")

    d = T.silu_inputs(257)
    x = d["x"].to(F64).requires_grad_(True)
    ref = T.silu_reference(d)
    agree(ref.tol["fwd"][0][0], torch.nn.functional.silu(x).detach(), "silu")
    agree(ref.tol["bwd"][0][0], torch.autograd.grad(torch.nn.functional.silu(x), x, d["dy"].to(F64))[0], "silu backward")

    d = T.lnp_inputs(T.Lnp(50, 203, 208, 212, "outlier"))
    gam, bet = torch.ones(203, dtype=F64, requires_grad=True), torch.zeros(203, dtype=F64, requires_grad=True)
    y = (d["x"].to(F64) - d["mean"].to(F64)[:, None]) * d["rstd"].to(F64)[:, None] * gam + bet
    gg, gb = torch.autograd.grad(y, (gam, bet), d["dy"].to(F64))
    ref = T.lnp_reference(d)
    agree(ref.tol["dgamma"][0][0], gg, "dgamma")
    agree(ref.tol["dbeta"][0][0], gb, "dbeta")


@pytest.mark.parametrize("case", [T.ATTB_CASES[2], T.ATTB_CASES[8], T.ATTB_CASES[12]], ids=T.attb_id)
def test_attn_bwd_reference_against_float64_autograd(case):
    """autograd of the masked softmax attention over the live queries, per batch row; lse against logsumexp, delta against sum P dP"""
    d = T.attb_inputs(case)
    B, S, H, G, rep = case.B, case.S, case.H, case.G, case.H // case.G
    ref = T.attb_reference(d)
    want = ref.tol["dqkv"][0].view(B, S, H + 2 * G, HD)
    ar = torch.arange(S)
    for b in range(B):
        lo = int(d["kstart"][b])
        if lo >= S:
            assert not bool(want[b].any())
            continue
        x = d["qkv"].to(F64).view(B, S, H + 2 * G, HD)[b].clone().requires_grad_(True)
        q, k, v = x[:, :H].transpose(0, 1), x[:, H:H + G].repeat_interleave(rep, 1).transpose(0, 1), x[:, H + G:].repeat_interleave(rep, 1).transpose(0, 1)
        allow = (ar[None, :] <= ar[:, None]) & (ar[None, :] >= lo)
        s = ((q[:, lo:] @ k.transpose(1, 2)) * HD ** -0.5).masked_fill(~allow[lo:], -math.inf)
        P = torch.softmax(s, -1)
        o = (P @ v).transpose(0, 1)
        do = d["dout"].to(F64).view(B, S, H, HD)[b]
        (gx,) = torch.autograd.grad(o, x, do[lo:])
        agree(want[b], gx, f"dqkv of batch row {b}")
        agree(ref.tol["lse"][0].view(B, H, S)[b][:, lo:], torch.logsumexp(s, -1).detach(), "lse")
        agree(ref.tol["delta"][0].view(B, H, S)[b][:, lo:], (P * (do[lo:].transpose(0, 1) @ v.transpose(1, 2))).sum(-1).detach(), "delta")


@pytest.mark.parametrize("case", [T.Ca(16, 3, 5, 65, "n01"), T.Ca(144, 3, 33, 63, "onehot"), T.Ca(512, 1, 17, 33, "flat")], ids=T.case_id)
def test_ca_references_against_float64_autograd(case):
    d = T.ca_inputs(case)
    R, H, dh = case.R, case.H, case.dh
    denom = float(torch.tensor(dh ** 0.5, dtype=F32))
    q = d["q"].to(F64).requires_grad_(True)
    kh = T.ca_heads(d["table"], H)
    qh = q.view(R, H, dh).transpose(0, 1)
    s = (qh @ kh.transpose(1, 2)) / denom
    o = torch.softmax(s, -1) @ kh
    out = o.transpose(0, 1).reshape(R, -1)
    (gq,) = torch.autograd.grad(out, q, d["dout"].to(F64))
    ref = T.ca_reference(d)
    agree(ref.tol["out"][0], out.detach(), "out")
    agree(ref.tol["lse"][0], torch.logsumexp(s, -1).t().detach(), "lse")
    dq = T.ca_bwd64(qh.detach(), kh, o.detach(), T.ca_heads(d["dout"], H), torch.logsumexp(s, -1, keepdim=True).detach(), denom)[0]
    agree(dq.transpose(0, 1).reshape(R, -1), gq, "dq")
    out32, lse32 = T.ca_handed(d)                                # what the backward is handed: the fp32 roundings of the same forward
    assert float((out32.to(F64) - out.detach()).abs().max()) <= T.e * float(out.detach().abs().max())
    assert float((lse32.to(F64) - torch.logsumexp(s, -1).t().detach()).abs().max()) <= T.e * float(torch.logsumexp(s, -1).detach().abs().max())


# ------------------------------------------------------------------------------------------------ the case lists, the plan, the refusals
def _lib():
    from ps_slm_amd import _lib
    return _lib.load()


def test_case_lists_reach_what_they_claim():
    assert {c.D for c in T.RMSB_CASES} == {1, 64, 1023, 1024, 1025, 2049, 3584} and {c.M for c in T.RMSB_CASES} == {1, 3}
    assert {(c.profile, c.acc) for c in T.RMSB_CASES} == {(p, a) for p in ("scales", "outlier", "zero_row") for a in (0, 1)}
    assert {c.M * c.I for c in T.SWIB_CASES} >= {1, 255, 256, 257} and T.Swib(3, 85) in T.SWIB_CASES and T.Swib(2, 129) in T.SWIB_CASES
    g = T.point_inputs(257, 1)[0].tolist()
    assert all(v in g for v in (0.0, 45.0, -45.0, 80.0, -80.0, 100.0, -100.0)) and any(v == 0 and math.copysign(1, v) < 0 for v in g)
    assert {(c.M, c.C) for c in T.DROP_CASES} == {(1, 1), (3, 85), (5, 256), (2, 257)} and all(c.ldx > c.C and c.ldo > c.C for c in T.DROP_CASES)
    assert {c.sid for c in T.DROP_CASES} == {0, 1, 70000} and all(c.step > 0 for c in T.DROP_CASES)
    assert {c.p for c in T.DROP_CASES} == {0.0, 0.5, 0.1, 0.25, 0.999999}
    assert {(c.R, c.C) for c in T.COLS_CASES} == {(R, C) for R in (1, 2, 1000) for C in (1, 255, 256, 257)} and all(c.ld > c.C for c in T.COLS_CASES)
    assert {(c.R, c.D) for c in T.LNP_CASES} == {(R, D) for R in (1, 50) for D in (1, 203, 256, 257)}
    assert all(c.lddy != c.ldx and c.lddy > c.D and c.ldx > c.D for c in T.LNP_CASES)
    assert T.tr_rpads(33) == [33, 34, 64, 73] and T.tr_rpads(32) == [32, 33, 72] and T.tr_rpads(1) == [1, 2, 32, 41]
    assert {c.H // c.G for c in T.ATTB_CASES if c.G == 1} == set(range(1, 9))
    assert {(c.H, c.G) for c in T.ATTB_CASES} >= {(12, 2), (28, 4), (16, 2)} and {c.S for c in T.ATTB_CASES} == {1, 2, 64, 65, 257}
    assert all(c.B == 3 for c in T.ATTB_CASES) and {k for c in T.ATTB_CASES for k in c.kstart} == {"0", "mid", "last", "all"}
    assert T.ATTB_LONG.S == 2048 and T.ATTB_LONG.H // T.ATTB_LONG.G == 8
    assert (2 * 8 * HD + 2 * 8 * 2048 + 4 * 8 * HD + 4 * 8) * 4 == 152 * 1024 + 128                  # the first launch's LDS at REP = 8, S = 2048
    for dh in T.CA_DHS:
        cs = T.ca_cases(dh)
        rows, kt = T.ca_rows(dh), T.ca_kt(dh)
        assert {c.R for c in cs} >= {1, rows, rows + 1} and {c.V for c in cs} >= {1, kt - 1, kt, kt + 1} and {c.H for c in cs} >= {1, 3}
        assert {c.profile for c in cs} == {"n01", "onehot", "flat", "int"} and all(c.profile == "flat" for c in cs if c.V == kt + 1)
        if dh <= 256:
            assert {c.V for c in cs} >= {257, 513} and all(T.ca_plan(c.R, 513, dh * c.H, c.H) == (2, 5) for c in cs)
    assert any(c.H == 8 for c in T.ca_cases(16)) and 63 in {c.R for c in T.ca_cases(128)}
    assert T.ca_plan(1, 16385, 128, 2) == (52, 5) and 51 * 5 < 257 <= 52 * 5 and 256 * 64 + 1 == 16385     # 257 tiles in 52 splits, the last tile one key
    assert (144 // 16) % 2 == 1 and [p * 17 // 4 for p in range(5)] == [0, 4, 8, 12, 17]             # the odd tail; the uneven part ranges


def test_restated_plan_against_the_library():
    lib = _lib()
    cases = [c for dh in T.CA_DHS for c in T.ca_cases(dh)] + [T.CA_MANY, T.Ca(64, 8, 300, 151936, "n01"), T.Ca(448, 8, 37, 1000, "n01")]
    for c in cases:
        D = c.dh * c.H
        assert lib.tasu_f32_ca_workspace_floats(c.R, c.V, D, c.H) == T.ca_ws_floats(c.R, c.V, D, c.H), c
    assert lib.tasu_f32_ca_workspace_floats(1, 1, 16, 0) == -1 and lib.tasu_f32_ca_workspace_floats(1, 1, 17, 2) == -1


def test_entry_points_refuse_before_any_launch():
    """non-null operands (host buffers nobody dereferences: the refusal comes first), bad pitches and shapes: TASU_ERR_ARG = 1"""
    lib = _lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    assert lib.tasu_f32_layernorm_bwd_params(p, 15, p, 16, p, p, p, p, 4, 16, None) == 1               # lddy < D (new with these tests)
    assert lib.tasu_f32_layernorm_bwd_params(p, 16, p, 15, p, p, p, p, 4, 16, None) == 1               # ldx < D
    assert lib.tasu_f32_layernorm_bwd_params(p, 16, p, 16, p, p, p, p, 0, 16, None) == 1
    assert lib.tasu_f32_colsum(p, 15, p, 4, 16, None) == 1
    assert lib.tasu_f32_transpose(p, 15, p, 8, 4, 16, 8, None) == 1                                      # lds < C
    assert lib.tasu_f32_transpose(p, 16, p, 7, 4, 16, 8, None) == 1                                      # ldd < Rpad
    assert lib.tasu_f32_transpose(p, 16, p, 8, 4, 16, 3, None) == 1                                      # Rpad < R
    assert lib.tasu_f32_lora_dropout(p, 15, p, 16, 4, 16, 0.1, p, 0, 0, None) == 1                       # ldx < C
    assert lib.tasu_f32_lora_dropout(p, 16, p, 16, 4, 16, 1.0, p, 0, 0, None) == 1                       # p = 1
    assert lib.tasu_f32_lora_dropout(p, 16, p, 16, 4, 16, 0.1, p, -1, 0, None) == 1                      # stream id < 0
    assert lib.tasu_f32_rmsnorm_bwd(p, p, p, p, 0, 16, 1e-6, 0, None) == 1
    assert lib.tasu_f32_swiglu_bwd(p, p, p, 4, 0, None) == 1
    assert lib.tasu_f32_silu(p, None, p, 0, None) == 1
    assert lib.tasu_f32_gather_rows(p, p, p, 0, 16, None) == 1
    assert lib.tasu_f32_attn_bwd(p, p, p, p, p, p, 1, 2049, 2, 1, 1.0, None) == 1                        # S > 2048
    assert lib.tasu_f32_attn_bwd(p, p, p, p, p, p, 1, 4, 9, 1, 1.0, None) == 1                           # REP = 9
    assert lib.tasu_f32_attn_bwd(p, p, p, p, p, p, 1, 4, 3, 2, 1.0, None) == 1                           # H % G
    a = (p + 15) // 16 * 16
    big = 1 << 20
    assert lib.tasu_f32_ca_attn_lse(a, 32, a, 4, 32, 2, 4.0, a, 32, a, 4, a, 7, None) == 1                # a workspace too small
    assert lib.tasu_f32_ca_attn_lse(a, 34, a, 4, 32, 2, 4.0, a, 32, a, 4, a, big, None) == 1              # ldq % 4
    assert lib.tasu_f32_ca_attn_lse(a, 32, a, 4, 32, 2, 4.0, a, 31, a, 4, a, big, None) == 1              # ldo < D
    assert lib.tasu_f32_ca_attn_lse(a, 48, a, 4, 48, 2, 4.0, a, 48, a, 4, a, big, None) == 1              # dh = 24
    assert lib.tasu_f32_ca_attn_lse(a + 4, 32, a, 4, 32, 2, 4.0, a, 32, a, 4, a, big, None) == 1          # q not 16-byte aligned
    assert lib.tasu_f32_ca_attn_lse(a, 32, a, 4, 32, 2, 4.0, a, 32, None, 4, a, big, None) == 1           # no lse
    assert lib.tasu_f32_ca_attn_bwd(a, 32, a, 4, 32, 2, 4.0, a, 32, a, 34, a, a, 32, 4, a, big, None) == 1    # lddo % 4
    assert lib.tasu_f32_ca_attn_bwd(a, 32, a, 4, 32, 2, 4.0, a, 32, a, 32, a, a, 31, 4, a, big, None) == 1    # lddq < D
    assert lib.tasu_f32_ca_attn_bwd(a, 32, a, 4, 32, 2, 0.0, a, 32, a, 32, a, a, 32, 4, a, big, None) == 1    # denom = 0


# ------------------------------------------------------------------------------------------------ mutants of the restatement
def expf_contracted(x):
    """expf as the compiler expands it with ph - E contracted into fma(x, log2e, -E), emulated in float32 (the derivation and the
    uncontracted form: tests/test_f32_ref64_cpu.py::test_expf_allowance_covers_the_contracted_expansion)"""
    f = np.float32
    c, cc = (np.frombuffer(struct.pack("<I", h), dtype=f)[0] for h in (0x3FB8AA3B, 0x32A5705F))
    out = np.empty(x.numel(), dtype=f)
    with np.errstate(over="ignore"):
        for i, v in enumerate(x.reshape(-1).tolist()):
            x32 = f(v)
            ph = f(x32 * c)
            pl = f(float(x32) * float(cc) + float(f(float(x32) * float(c) - float(ph))))
            E = np.rint(ph)
            base = f(float(x32) * float(c) - float(E))
            out[i] = f(min(2.0 ** float(f(base + pl)) * 2.0 ** float(max(E, -1000.0)), 1e300))
    return torch.from_numpy(out).view(x.shape)


class DAs1024(T.F32TrainTorch):
    def _rms_d(self, D):
        return 1024.0


class DotWithoutW(T.F32TrainTorch):
    def _rms_dot_w(self, w):
        return torch.ones_like(w)


class DuFromU(T.F32TrainTorch):
    def _swiglu_du(self, d, g, u, sg):
        return d * (u * self._sigmoid(u))


class ContractedExpf(T.F32TrainTorch):
    def _sigmoid(self, x):
        return 1 / (1 + expf_contracted(-x))


class LastRowSkipped(T.F32TrainTorch):
    def _colsum_rows(self, R):
        return R - 1


class PitchedMask(T.F32TrainTorch):
    def _mask_scale(self, rng, sid, M, Cn, ldx, p):
        return T.lora_keep_scale((int(rng[0]), int(rng[1])), sid, (M, ldx), p)[:, :Cn]


class OneKeyHeadLeftOut(T.F32TrainTorch):
    """the group's last (small) head left out of dK at the newest key only"""

    def f32_attn_bwd(self, qkv, dout, kstart, dqkv, lse_ws, delta_ws, B, S, H, G, scale):
        super().f32_attn_bwd(qkv, dout, kstart, dqkv, lse_ws, delta_ws, B, S, H, G, scale)
        x, do, rep = qkv[:B * S].view(B, S, H + 2 * G, HD), dout[:B * S].view(B, S, H, HD), H // G
        h = rep - 1
        s = float(x[0, S - 1, h] @ x[0, S - 1, H]) * scale
        p = math.exp(s - float(lse_ws[:B * H * S].view(B, H, S)[0, h, S - 1]))
        ds = p * (float(do[0, S - 1, h] @ x[0, S - 1, H + G]) - float(delta_ws[:B * H * S].view(B, H, S)[0, h, S - 1])) * scale
        dqkv[:B * S].view(B, S, H + 2 * G, HD)[0, S - 1, H] -= ds * x[0, S - 1, h]


def _mut(name):
    ops = T.F32TrainTorch()
    ops.mutant = name
    return ops


def _finite(t):
    return torch.nan_to_num(t.to(F64), nan=1e30)


def _old(got, ref):
    """the tensor-wide metric over the float outputs the older tests compare"""
    old = 0.0
    for name, (want, _) in ref.tol.items():
        old = max(old, T.old_metric(_finite(got[name].reshape(want.shape)), want))
    for name, want in ref.exact.items():
        old = max(old, T.old_metric(_finite(got[name]), want))
    return old


def _old_attn(got, ref, d):
    """test_attention_backward_fp32's: per batch row over the live rows of dqkv (lse and delta are not looked at)"""
    c = d["case"]
    g, r = got["dqkv"].view(c.B, c.S, -1), ref.tol["dqkv"][0].view(c.B, c.S, -1)
    return max(T.old_metric(_finite(g[b, lo:]), r[b, lo:]) for b, lo in enumerate(d["kstart"].tolist()) if lo < c.S)


def test_mutants_of_the_restatement():
    rows = []

    def record(name, limit, old, clean, mutant, ref, must_pass=False):
        c_new, m_new = T.worst_of(clean, ref), T.worst_of(mutant, ref)
        c_old, m_old = old(clean, ref), old(mutant, ref)
        rows.append((name, m_old < limit))
        print(f"MUTANT {name}: older metric {m_old:.2e} (limit {limit:.0e}: {'PASSES' if m_old < limit else 'fails'}), |err| / E {m_new:.3g}; "
              f"clean restatement {c_old:.2e} and {c_new:.3f}")
        assert c_new <= 1.0, name
        assert (m_new <= 1.0) if must_pass else (m_new > 1.0), name

    clean_ops = T.F32TrainTorch()
    d = T.rmsb_inputs(T.Rmsb(3, 1023, "scales", 0))
    ref, clean = T.rmsb_reference(d), T.run_rmsb(clean_ops, d)
    record("rmsnorm_bwd: the 1 / D of k taken as 1 / 1024 at D = 1023", 1e-5, _old, clean, T.run_rmsb(DAs1024(), d), ref)
    d = T.rmsb_inputs(T.Rmsb(3, 1025, "outlier", 0))
    record("rmsnorm_bwd: w left out of dot (outlier column)", 1e-5, _old, T.run_rmsb(clean_ops, d), T.run_rmsb(DotWithoutW(), d), T.rmsb_reference(d))

    d = T.swib_inputs(T.Swib(3, 85))
    ref, clean = T.swib_reference(d), T.run_swib(clean_ops, d)
    record("swiglu_bwd: du = d silu(u)", 1e-5, _old, clean, T.run_swib(DuFromU(), d), ref)
    d = T.swib_inputs(T.Swib(1, 257))
    ref, clean, contracted = T.swib_reference(d), T.run_swib(clean_ops, d), T.run_swib(ContractedExpf(), d)
    record("swiglu_bwd: sigmoid on the contracted expf, x = -45 included (must stay inside E)", 1e-5, _old, clean, contracted, ref, must_pass=True)
    i45 = d["gu"][0, :257].tolist().index(-45.0)
    off = abs(float(contracted["dgu"][0, i45]) - float(ref.tol["dgu"][0][0, i45])) / abs(float(ref.tol["dgu"][0][0, i45])) / T.e
    print(f"MUTANT   ... at g = -45 the contracted expf puts dg {off:.1f} e off (E allows {float(ref.tol['dgu'][1][0, i45] / ref.tol['dgu'][0][0, i45].abs()) / T.e:.1f} e)")
    assert 20 < off < 60

    d = T.cols_inputs(T.Cols(2, 257, 262, "outlier"))
    record("colsum: the last row skipped (R = 2, outlier profile)", 1e-5, _old, T.run_cols(clean_ops, d), T.run_cols(LastRowSkipped(), d), T.cols_reference(d))

    d = T.drop_inputs(T.Drop(3, 85, 88, 91, 0.1, 1, 3, 0))
    record("lora_dropout: the mask index pitched (m ldx + c)", 1e-5, _old, T.run_drop(clean_ops, d), T.run_drop(PitchedMask(), d), T.drop_reference(d))

    d = T.attb_inputs(T.Attb(3, 65, 7, 1, ("0", "mid", "last"), "outlier"))
    ref, clean = T.attb_reference(d), T.run_attb(clean_ops, d)
    old = lambda got, r: _old_attn(got, r, d)                    # noqa: E731
    for name in ("newest key dropped", "kstart off by one", "delta from the neighbouring head", "one head left out of dK", "dS without scale"):
        try:
            T.run_attb(_mut(name), d)
        except AssertionError as err:                            # an exact check inside the run caught it as well
            print(f"MUTANT attn_bwd: {name}: also caught by the run's exact checks ({str(err)[:90]})")
        got = T.run_attb(_mut(name), d, zeros=False)
        record(f"attn_bwd: {name}" + (" (the small head, outlier profile)" if "dK" in name else ""), 2e-5, old, clean, got, ref)
    record("attn_bwd: the small head left out of dK at the newest key only (outlier profile)", 2e-5, old, clean, T.run_attb(OneKeyHeadLeftOut(), d), ref)

    old_ca = lambda H: (lambda got, r: max(T.old_ca_metric(_finite(got[k]), (r.tol[k][0] if k in r.tol else r.exact[k]), H)   # noqa: E731
                                           for k in got if k != "lse"))
    c = T.Ca(128, 3, 64, 65, "flat")
    d = T.ca_inputs(c)
    ref, clean = T.ca_reference(d), T.run_ca(clean_ops, d)
    record("ca_attn: padding keys unmasked at V = KT + 1 (flat profile)", 2e-5, old_ca(3), clean, T.run_ca(_mut("padding keys unmasked"), d), ref)
    record("ca_attn: key V - 1 masked (flat profile)", 2e-5, old_ca(3), clean, T.run_ca(_mut("key V - 1 masked"), d), ref)
    c = T.Ca(128, 3, 65, 513, "onehot")
    d = T.ca_inputs(c)
    ref, clean = T.ca_reference(d), T.run_ca(clean_ops, d)
    record("ca_attn: the last split left out of the merge (V = 513)", 2e-5, old_ca(3), clean, T.run_ca(_mut("last split left out"), d), ref)
    out32, lse32 = T.ca_handed(d)
    ref, clean = T.ca_bwd_reference(d, out32, lse32), T.run_ca_bwd(clean_ops, d, out32, lse32)
    record("ca_attn_bwd: delta from out of the wrong head", 2e-5, old_ca(3), clean, T.run_ca_bwd(_mut("delta from the wrong head"), d, out32, lse32), ref)
    record("ca_attn_bwd: / denom applied once instead of twice", 2e-5, old_ca(3), clean, T.run_ca_bwd(_mut("denom applied once"), d, out32, lse32), ref)
    assert len(rows) == 17
    print("MUTANTS the older metric passes:", [n for n, p in rows if p])
