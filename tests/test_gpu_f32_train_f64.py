"""The fp32 training kernels (csrc/fp32_train.hip: tasu_f32_rmsnorm_bwd, _swiglu_bwd, _silu, _relu_bwd, _lora_dropout, _colsum,
_layernorm_bwd_params, _transpose, _gather_rows, _attn_bwd; csrc/f32_ca.hip: tasu_f32_ca_attn, _ca_attn_lse, _ca_attn_bwd) against
float64 references, element by element (tests/f32_train_ref64.py: the derivations, the cases, the runs; its own checks and the
mutants: tests/test_f32_train_ref64_cpu.py), through HipOps.  The references are computed in float64 on the device.

Every output and workspace starts as NaN, every operand has NaN guard rows and NaN in the gap of its pitch; everything outside
what a call owes must keep its bits.  Every element within 1.0 x E of the float64 value, exactly the reference's value where E = 0;
the selections, copies, masks, the integer profiles and the zeros owed to padding bit for bit; calls with a workspace twice, equal
bits.  The largest cases: the attention backward at S = 2048, REP = 8 (the first launch's largest LDS request, 152 KiB) and the
cross-attention at V = 16385 (52 splits).

Measured on MI355X (115 tests, 3.7 s for the file, the slowest 0.54 s): every check passed on the first run, no kernel line changed.
Largest |err| / E per entry point (the F64WORST lines), kernel / the torch fp32 restatement on the CPU:
    rmsnorm_bwd 0.985 / 0.985   swiglu_bwd 0.874 / 0.623   silu 0.874 / 0.652   lora_dropout 1.000 / 1.000 (one rounding)
    colsum 0.964 / 0.964   layernorm_bwd_params 0.692 / 0.692   attn_bwd 0.097 / 0.103   ca_attn 0.240 / 0.244
    ca_attn_bwd 0.166 / 0.188 on handed-in operands, 0.024 / 0.021 chained behind the forward kernel
The figures near 1 are single roundings (dx + g, out + v, one addition at R = 2) and, for the sigmoid kernels, the contracted expf
(tests/f32_ref64.py's header): g = -45 alone scores 0.831.  The mutant table and what is not reached: DESIGN section 5, "How the
fp32 training kernels are tested"."""
import pytest
import torch

import f32_train_ref64 as T

pytestmark = pytest.mark.gpu
F64, F32, I32 = torch.float64, torch.float32, torch.int32
HD = T.HD


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def cuda(t):
    return t.cuda()


def sync():
    torch.cuda.synchronize()


def nan(*shape):
    return T.nan(*shape).cuda()


_worst = {}


def hold(op, what, got, ref):
    w = T.check(got, ref, f"{op} {what}")
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {op} {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")


def refused(call, *outs):
    from ps_slm_amd.ops import TasuOpError
    with pytest.raises(TasuOpError, match="bad argument"):
        call()
    sync()
    for o in outs:
        assert T.untouched(o.cpu()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------ row and pointwise kernels
@pytest.mark.parametrize("case", T.RMSB_CASES, ids=T.case_id)
def test_rmsnorm_bwd(hip, case):
    d = T.rmsb_inputs(case)
    hold("rmsnorm_bwd", T.case_id(case), T.run_rmsb(hip, d, cuda, sync), T.rmsb_reference(d, cuda))


def test_swiglu_bwd_silu_and_relu_bwd(hip):
    for case in T.SWIB_CASES:
        d = T.swib_inputs(case)
        hold("swiglu_bwd", T.case_id(case), T.run_swib(hip, d, cuda, sync), T.swib_reference(d, cuda))
    for n in T.SILU_NS:
        d = T.silu_inputs(n)
        hold("silu", f"n = {n}", T.run_silu(hip, d, cuda, sync), T.silu_reference(d, cuda))
    for n in T.RELU_NS:
        T.run_relu(hip, n, cuda, sync)


@pytest.mark.parametrize("case", T.DROP_CASES, ids=T.case_id)
def test_lora_dropout(hip, case):
    d = T.drop_inputs(case)
    hold("lora_dropout", T.case_id(case), T.run_drop(hip, d, cuda, sync), T.drop_reference(d, cuda))


def test_colsum_and_layernorm_bwd_params(hip):
    for case in T.COLS_CASES:
        d = T.cols_inputs(case)
        hold("colsum", T.case_id(case), T.run_cols(hip, d, cuda, sync), T.cols_reference(d, cuda))
    for case in T.LNP_CASES:
        d = T.lnp_inputs(case)
        hold("layernorm_bwd_params", T.case_id(case), T.run_lnp(hip, d, cuda, sync), T.lnp_reference(d, cuda))


def test_transpose_and_gather_rows(hip):
    for R in T.TR_SIZES:
        for C in T.TR_SIZES:
            for Rpad in T.tr_rpads(R):
                T.run_transpose(hip, R, C, Rpad, cuda, sync)
    for n, D, rows in T.GATHER_CASES:
        T.run_gather(hip, n, D, rows, cuda, sync)


def test_row_kernels_refuse_what_they_do_not_serve(hip):
    R, D = 4, 16
    x = torch.ones(R + 2, D, device="cuda")
    short = torch.as_strided(x, (R, D), (D - 1, 1))                      # a pitch below the width
    v = torch.ones(D, device="cuda")
    dg, db = nan(D), nan(D)
    refused(lambda: hip.f32_layernorm_bwd_params(short, x, v, v, dg, db, R, D), dg, db)            # lddy < D
    refused(lambda: hip.f32_layernorm_bwd_params(x, short, v, v, dg, db, R, D), dg, db)            # ldx < D
    refused(lambda: hip.f32_layernorm_bwd_params(x, x, v, v, dg, db, 0, D), dg, db)
    out = nan(D)
    refused(lambda: hip.f32_colsum(short, out, R, D), out)
    dst = nan(D, 8)
    refused(lambda: hip.f32_transpose(short, dst, R, D, 8), dst)                                    # lds < C
    refused(lambda: hip.f32_transpose(x, dst, R, D, 9), dst)                                        # ldd < Rpad
    refused(lambda: hip.f32_transpose(x, dst, R, D, 3), dst)                                        # Rpad < R
    o2 = nan(R, D)
    rng = torch.tensor([1, 1], dtype=torch.int64, device="cuda")
    refused(lambda: hip.f32_lora_dropout(short, o2, R, D, 0.1, rng, 0), o2)
    refused(lambda: hip.f32_lora_dropout(x, o2, R, D, 1.0, rng, 0), o2)
    refused(lambda: hip.f32_lora_dropout(x, o2, R, D, 0.1, rng, -1), o2)
    refused(lambda: hip.f32_rmsnorm_bwd(x, x, v, o2, 0, D, 1e-6, False), o2)
    refused(lambda: hip.f32_swiglu_bwd(x, x, o2, R, 0), o2)
    refused(lambda: hip.f32_gather_rows(x, torch.zeros(2, dtype=I32, device="cuda"), o2, 0, D), o2)


# ------------------------------------------------------------------------------------------------ attention backward
@pytest.mark.parametrize("case", T.ATTB_CASES + [T.ATTB_LONG], ids=T.attb_id)
def test_attn_bwd(hip, case):
    d = T.attb_inputs(case)
    hold("attn_bwd", T.attb_id(case), T.run_attb(hip, d, cuda, sync), T.attb_reference(d, cuda))


def test_attn_bwd_refuses_what_it_does_not_serve(hip):
    z = torch.zeros(1, dtype=I32, device="cuda")
    x = torch.ones(4, 11 * HD, device="cuda")
    dq, ls, dl = nan(4, 11 * HD), nan(64), nan(64)
    refused(lambda: hip.f32_attn_bwd(x, x, z, dq, ls, dl, 1, 2049, 1, 1, 1.0), dq, ls, dl)        # S > 2048
    refused(lambda: hip.f32_attn_bwd(x, x, z, dq, ls, dl, 1, 4, 9, 1, 1.0), dq, ls, dl)           # REP = 9
    refused(lambda: hip.f32_attn_bwd(x, x, z, dq, ls, dl, 1, 4, 3, 2, 1.0), dq, ls, dl)           # H % G
    refused(lambda: hip.f32_attn_bwd(x, x, z, dq, ls, dl, 0, 4, 2, 1, 1.0), dq, ls, dl)


# ------------------------------------------------------------------------------------------------ cross-attention
def _ca(hip, case):
    D = case.dh * case.H
    assert hip.f32_ca_workspace_floats(case.R, case.V, D, case.H) == T.ca_ws_floats(case.R, case.V, D, case.H), "the split policy moved"
    d = T.ca_inputs(case)
    fwd = T.run_ca(hip, d, cuda, sync)
    hold("ca_attn", T.case_id(case), fwd, T.ca_reference(d, cuda))
    out32, lse32 = T.ca_handed(d, cuda)
    hold("ca_attn_bwd", T.case_id(case), T.run_ca_bwd(hip, d, out32, lse32, cuda, sync), T.ca_bwd_reference(d, out32, lse32, cuda))
    hold("ca_attn_bwd_chain", T.case_id(case), T.run_ca_bwd(hip, d, fwd["out"], fwd["lse"], cuda, sync), T.ca_bwd_reference(d, dev=cuda))


@pytest.mark.parametrize("dh", T.CA_DHS)
def test_ca_attn_forward_lse_and_backward(hip, dh):
    for case in T.ca_cases(dh):
        _ca(hip, case)


def test_ca_attn_52_splits(hip):
    assert T.ca_plan(T.CA_MANY.R, T.CA_MANY.V, T.CA_MANY.dh * T.CA_MANY.H, T.CA_MANY.H) == (52, 5)
    _ca(hip, T.CA_MANY)


def test_ca_attn_refuses_what_it_does_not_serve(hip):
    R, V, H, D = 4, 5, 2, 32
    q, table = torch.ones(R + 1, D + 4, device="cuda"), torch.ones(V, D, device="cuda")
    out, lse, ws = nan(R, D), nan(R, H), nan(4096)
    qv = q[:R, :D]
    refused(lambda: hip.f32_ca_attn_lse(qv, table, out, lse, R, H, ws=ws[:7]), out, lse, ws)                          # workspace too small
    refused(lambda: hip.f32_ca_attn_lse(torch.as_strided(q, (R, D), (D + 2, 1)), table, out, lse, R, H, ws=ws), out, lse, ws)   # ldq % 4
    refused(lambda: hip.f32_ca_attn_lse(qv, table, torch.as_strided(out, (R, D), (D - 1, 1)), lse, R, H, ws=ws), out, lse, ws)  # ldo < D
    refused(lambda: hip.f32_ca_attn_lse(q.view(-1)[1:1 + R * D].view(R, D), table, out, lse, R, H, ws=ws), out, lse, ws)        # q unaligned
    refused(lambda: hip.f32_ca_attn(qv, torch.ones(V, 48, device="cuda"), nan(R, 48), R, 2, ws=ws), ws)                # dh = 24
    dq = nan(R, D)
    ok = torch.ones(R, D, device="cuda")
    refused(lambda: hip.f32_ca_attn_bwd(qv, table, ok, torch.as_strided(q, (R, D), (D + 2, 1)), lse, dq, R, H, ws=ws), dq, ws)  # lddo % 4
    refused(lambda: hip.f32_ca_attn_bwd(qv, table, ok, ok, lse, torch.as_strided(dq, (R, D), (D - 1, 1)), R, H, ws=ws), dq, ws)  # lddq < D
    refused(lambda: hip.f32_ca_attn_bwd(qv, table, ok, ok, lse, dq, R, H, ws=ws[:7]), dq, ws)
