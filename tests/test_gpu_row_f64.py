"""The bf16 step's row-reduction kernels against float64 references, element by element (tests/row_ref64.py; its own checks:
tests/test_row_ref64_cpu.py), through HipOps like tests/test_gpu_ops.py:

  csrc/norm.hip         RMSNorm forward (plain, _ld, _frag, _rows; every register-resident instance and the generic kernel, one
                        and four rows per workgroup) and backward (accumulate, the bf16 copy, slot maps, the compact residual),
                        LayerNorm forward (wave kernel, block kernel with vector body + tail and with the scalar body, a
                        production-width row set), layernorm_bwd_params, colsum
  csrc/ce.hip           tasu_ce_fwd_bwd on ce_kernel and on ce_reg_kernel (two buffers and in place, ignored rows, labels at the
                        edges and at a peaked argmax, ties, pad columns, the full vocabulary and the register kernel's last
                        width), tasu_ce_reduce
  csrc/cross_attn.hip   scale_softmax_rows / softmax_bwd_rows (vector and scalar bodies, both denominators)
  csrc/encoder_aux.hip  softmax_rows, psd_logit_stats, psd_gather_softmax

Every output and workspace starts as NaN (integers: -7); guard rows, guard elements and (where the kernel owes them nothing) pad
columns must keep their bits.  Every output within 1.0 x E of the float64 value on every element, exactly the reference's value
where E = 0; integer outputs and the exact-integer profiles bit for bit.  Second check, bf16 outputs: rms(err / (u |ref|)) over
the elements whose fp32 allowance is at most a tenth of u |ref| (cases with at least 4096 of them) at most 1.5 x the torch
double's on the same inputs (the F64RATIO lines this file prints).

Measured on MI355X (411 tests, 2.0 s for the file): every check passes.  Largest |err| / E per operation (the F64WORST lines):
    rmsnorm_fwd 0.996   rmsnorm_bwd 0.996   layernorm_fwd 0.995   layernorm_bwd_params 0.156   colsum 0.003
    ce_fwd_bwd  ce_kernel 0.988  ce_reg_kernel 0.991   ce_reduce 0.741
    scale_softmax_rows 0.995   softmax_bwd_rows 0.837   softmax_rows 0.738   psd_logit_stats 0.269   psd_gather_softmax 0.959
Largest rms ratio, kernel / double: 1.000 for every bf16 output with at least 4096 eligible elements (rmsnorm_fwd y, rmsnorm_bwd
dx_bf16, layernorm_fwd y, dlogits on both kernels, scale_softmax_rows p).  Scratch mutants of four kernels fail
this file where they should; two of them (argmax ties in ce_reg_kernel, the PSD rescale) pass every older test.  No kernel
needed a fix."""
import pytest
import torch

import row_ref64 as R
from fake_ops import FakeOps
from test_gpu_ops import unfrag

pytestmark = pytest.mark.gpu
F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def cuda(t):
    return t.cuda()


def nan(*shape, dtype=F32):
    return R.nan(*shape, dtype=dtype).cuda()


_worst, _ratios = {}, {}


def hold(op, case, got, ref, double=None):
    """one run against its Ref: the element-wise check, then the rms ratio of every bf16 output against the double's"""
    what = f"{op} {R.case_id(case)}"
    w = R.check(got, ref, what)
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")
    for name, (want, E) in ref.tol.items():
        if double is None or got[name].dtype != BF:
            continue
        k, n = R.rms_stat(got[name], want, E)
        dbl, _ = R.rms_stat(double[name], want, E)
        if n < 4096:
            continue
        ratio = k / dbl if dbl > 0 else 0.0
        _ratios[(op, name)] = max(_ratios.get((op, name), 0.0), ratio)
        print(f"F64RATIO {op} {name} {ratio:.3f} kernel {k:.5f} double {dbl:.5f} over {n} elements {R.case_id(case)} "
              f"(largest so far {_ratios[(op, name)]:.3f})")
        assert k <= R.RMS_RATIO * dbl, (f"{what} {name}: rms {k:.5f} is {ratio:.2f} x the double's {dbl:.5f} (at most {R.RMS_RATIO} x: "
                                        f"a systematic error, not rounding)")


# ------------------------------------------------------------------------------------------------ csrc/norm.hip
@pytest.mark.parametrize("case", R.RMS_FWD_CASES, ids=R.case_id)
def test_rmsnorm_fwd(hip, fake, case):
    d = R.rms_fwd_inputs(case)
    ref = R.rms_fwd_reference(d)
    got = R.run_rms_fwd(hip, d, cuda)
    dbl = R.run_rms_fwd(fake, d)
    if case.form == "frag":
        n, D = d["n"], d["D"]
        raw = got["y_raw"]
        rows = unfrag(raw, D)
        assert R.untouched(rows[n:]) and R.untouched(raw[64:]), "rmsnorm_fwd_frag: rows >= M of the fragment buffer were written"
        y = nan(n + R.GUARD, D, dtype=BF)
        hip.dec_rmsnorm(cuda(d["x"]), cuda(d["w"]), y[:n], R.EPS_RMS)           # the same call row-major, no rstd
        torch.cuda.synchronize()
        y = y.cpu()
        assert R.untouched(y[n:])
        R.same_bits(rows[:n].contiguous(), y[:n], "rmsnorm_fwd_frag against the row-major form")
        got, dbl, ref = {"y": rows[:n].contiguous()}, {"y": dbl["y_raw"][:n]}, R.Ref({"y": ref.tol["y"]}, {})
    hold("rmsnorm_fwd", case, got, ref, dbl)


@pytest.mark.parametrize("case", R.RMS_BWD_CASES, ids=R.case_id)
def test_rmsnorm_bwd(hip, fake, case):
    d = R.rms_bwd_inputs(case)
    hold("rmsnorm_bwd", case, R.run_rms_bwd(hip, d, cuda), R.rms_bwd_reference(d), R.run_rms_bwd(fake, d))


@pytest.mark.parametrize("case", R.LN_CASES, ids=R.case_id)
def test_layernorm_fwd(hip, fake, case):
    d = R.ln_inputs(case)
    hold("layernorm_fwd", case, R.run_ln(hip, d, cuda), R.ln_reference(d), R.run_ln(fake, d))


@pytest.mark.parametrize("case", R.LNB_CASES + R.COLSUM_CASES, ids=R.case_id)
def test_column_sums(hip, case):
    d = R.col_inputs(case)
    hold("layernorm_bwd_params" if case.op == "lnb" else "colsum", case, R.run_col(hip, d, cuda), R.col_reference(d))


# ------------------------------------------------------------------------------------------------ csrc/ce.hip
def _ce(hip, fake, case):
    d = R.ce_inputs(case)
    ref = R.ce_reference(d)
    got = R.run_ce(hip, d, cuda)
    hold(f"ce_fwd_bwd[{d['kernel']}]", case, got, ref, R.run_ce(fake, d))
    if case.dl == "inplace":                                     # twice the same bits
        again = R.run_ce(hip, d, cuda)
        for name in got:
            R.same_bits(again[name], got[name], f"ce_fwd_bwd in place, second run, {name}")


@pytest.mark.parametrize("case", [c for c in R.CE_CASES if c.V < 100000], ids=R.case_id)
def test_cross_entropy(hip, fake, case):
    _ce(hip, fake, case)


def test_cross_entropy_full_vocabulary_rows(hip, fake):
    """V = 151,936 on both kernels, the register kernel's last width (all 20 chunks of every thread) and the first row past it"""
    big = [c for c in R.CE_CASES if c.V >= 100000]
    assert {R.ce_kernel_of(c) for c in big} == {"reg", "online"} and all(c.M <= 3 for c in big)
    for case in big:
        _ce(hip, fake, case)


@pytest.mark.parametrize("case", R.CE_REDUCE_CASES, ids=R.case_id)
def test_ce_reduce(hip, case):
    d = R.red_inputs(case)
    got = R.run_red(hip, d, cuda)
    if case.profile == "ignored":                                # the mean over nothing, as the reference's
        assert float(got["count"]) == 0.0 and bool(torch.isnan(got["out"]).all())
        return
    hold("ce_reduce", case, got, R.red_reference(d))


# ------------------------------------------------------------------------------------------------ csrc/cross_attn.hip
@pytest.mark.parametrize("case", R.SM_CASES, ids=R.case_id)
def test_scale_softmax_rows_and_backward(hip, fake, case):
    d = R.sm_inputs(case)
    fwd, bwd = R.sm_reference(d)
    hold("scale_softmax_rows", case, R.run_sm_fwd(hip, d, cuda), fwd, R.run_sm_fwd(fake, d))
    hold("softmax_bwd_rows", case, R.run_sm_bwd(hip, d, cuda), bwd, R.run_sm_bwd(fake, d))


# ------------------------------------------------------------------------------------------------ csrc/encoder_aux.hip
@pytest.mark.parametrize("case", R.SR_CASES, ids=R.case_id)
def test_softmax_rows(hip, case):
    d = R.sr_inputs(case)
    hold("softmax_rows", case, R.run_sr(hip, d, cuda), R.sr_reference(d))


@pytest.mark.parametrize("case", R.PSD_CASES, ids=R.case_id)
def test_psd_from_the_logits(hip, case):
    d = R.psd_inputs(case)
    stats, gather = R.psd_reference(d)
    hold("psd_logit_stats", case, R.run_psd_stats(hip, d, cuda), stats)
    hold("psd_gather_softmax", case, R.run_psd_gather(hip, d, cuda), gather)


# ------------------------------------------------------------------------------------------------ bad arguments
def refused(call, *outs):
    from ps_slm_amd.ops import TasuOpError
    with pytest.raises(TasuOpError, match="bad argument"):
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert R.untouched(o.cpu()), "a refused call wrote to its output"


def test_rmsnorm_refuses_what_it_does_not_serve(hip):
    w8, w256, w260 = (torch.ones(n, device="cuda") for n in (8, 256, 260))
    y, r = nan(4, 8, dtype=BF), nan(4)
    refused(lambda: hip.rmsnorm_fwd(torch.ones(4, 6, device="cuda"), w8[:6], y[:, :6].contiguous().fill_(R.NAN), r, 1e-6), r)   # D % 4
    refused(lambda: hip.rmsnorm_fwd(torch.ones(4, 8, device="cuda"), w8, torch.as_strided(y, (4, 8), (4, 1)), r, 1e-6), y, r)   # ldy < D
    yf = nan(128, 260, dtype=BF)
    hip.dec_frag = True
    try:
        refused(lambda: hip.dec_rmsnorm(torch.ones(65, 256, device="cuda"), w256, yf, 1e-6), yf)                                 # _frag, M = 65
        refused(lambda: hip.dec_rmsnorm(torch.ones(4, 260, device="cuda"), w260, yf, 1e-6), yf)                                  # _frag, D % 32
    finally:
        hip.dec_frag = False
    x, dy, rs = torch.ones(4, 8, device="cuda"), torch.ones(4, 8, dtype=BF, device="cuda"), torch.ones(4, device="cuda")
    dx, dxb = nan(4, 8), nan(4, 8, dtype=BF)
    slot = torch.arange(4, dtype=I32, device="cuda")
    refused(lambda: hip.rmsnorm_bwd_rows(dy, x, w8, rs, None, dx, dxb), dx, dxb)                                                # no slot map
    refused(lambda: hip.rmsnorm_bwd_rows_resid(dy, x, w8, rs, None, torch.ones(4, 8, device="cuda"), dx, dxb), dx, dxb)         # resid without slot
    refused(lambda: hip.rmsnorm_bwd_rows_resid(dy, x, w8, rs, slot, None, dx, dxb), dx, dxb)
    refused(lambda: hip.rmsnorm_bwd(dy[:, :6].contiguous(), x[:, :6].contiguous(), w8[:6], rs, dx[:, :6].contiguous().fill_(R.NAN), None, False))


def test_cross_entropy_refuses_what_it_does_not_serve(hip):
    lab, inv = torch.zeros(2, dtype=I32, device="cuda"), torch.ones(1, device="cuda")
    rl, rh = nan(2), torch.full((2,), -7, dtype=I32, device="cuda")
    dl12, dl16 = nan(2, 12, dtype=BF), nan(2, 16, dtype=BF)
    refused(lambda: hip.ce_fwd_bwd(torch.zeros(2, 12, dtype=BF, device="cuda"), lab, 2, 10, rl, rh, None, dl12, inv), rl, rh, dl12)   # ldv % 8
    refused(lambda: hip.ce_fwd_bwd(torch.zeros(2, 16, dtype=BF, device="cuda"), lab, 2, 20, rl, rh, None, dl16, inv), rl, rh, dl16)   # ldv < V
    refused(lambda: hip.ce_fwd_bwd(torch.zeros(2, 16, dtype=BF, device="cuda"), lab, 2, 16, rl, rh, None, dl16, None), rl, rh, dl16)  # no inv_count


def test_layernorm_colsum_and_softmax_refuse_what_they_do_not_serve(hip):
    g = torch.ones(8, device="cuda")
    y, out = nan(2, 8, dtype=BF), nan(8)
    x = torch.ones(16, device="cuda")
    refused(lambda: hip.layernorm_fwd(torch.as_strided(x, (2, 8), (4, 1)), g, g, y, None, None, 2, 8, 1e-5), y)                 # ldx < D
    refused(lambda: hip.colsum(torch.ones(3, 7, dtype=BF, device="cuda"), out, 3, 7), out)                                      # odd ld
    s, stats = torch.ones(2, 8, dtype=BF, device="cuda"), torch.ones(2, 2, device="cuda")
    p, st = nan(2, 8, dtype=BF), nan(2, 2)
    for denom in (0.0, -1.0):
        refused(lambda: hip.scale_softmax_rows(s, p, 2, 8, denom, st), p, st)
        refused(lambda: hip.softmax_bwd_rows(s, stats, s, p, 2, 8, denom), p)
    refused(lambda: hip.scale_softmax_rows(s, p, 2, 12, 8.0, st), p, st)                                                        # ld < V
    refused(lambda: hip.softmax_bwd_rows(s, stats, s, p, 2, 12, 8.0), p)
