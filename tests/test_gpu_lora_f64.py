"""The LoRA kernels and the AdamW update against float64 references, element by element (tests/lora_ref64.py; its own checks:
tests/test_lora_ref64_cpu.py), through HipOps like tests/test_gpu_lora.py:

  csrc/gemm_rank.hip     tasu_gemm_nt_rank (fp32 / bf16 out, plain / transposed store), tasu_gemm_nt_rank_group (per member, each with
                         its own K and lda), tasu_gemm_tn_rank: the bits of the exact-integer profile, |err| <= F = (K + 2) e sum |a b|
                         (bf16: u |c| + F) on N(0, 1) x 0.5, the rms ratio against the double; 0, 1 and 2 chunks per wave, one to
                         four column groups, last tiles of 1 and 15 rows, C off 16-byte alignment, NaN in every operand gap
  csrc/lora.hip          tasu_lora_apply and _group: the bits of the exact profile (every scale, drop rate, with and without the
                         residual), the interval [chain(v_lo), chain(v_hi)] on N(0, 1), x_out = fl32(x_in + y_got), the mask equal
                         to tasu_lora_dropout's and to lora_keep_scale; tasu_scale_bf16, tasu_lora_dropout, tasu_lora_dropout_norm
                         and _group, tasu_lora_refresh: bits
  csrc/elementwise.hip   tasu_transpose_bf16 as lora.py calls it (vector and scalar path): bits, zeros in the padding
  csrc/misc.hip          tasu_adamw within E_m / E_v / E_p of float64 AdamW on the constants the kernel is handed, pb = bf16(p_got)

Every output starts as NaN inside a NaN-filled buffer; every cell outside the stored block must keep its bits; every GEMM case runs
twice and must give equal bits; a bad argument must return the error and leave the output untouched.  LIMIT = 1.0 x E.

Measured on MI355X (237 tests, 6.3 s for the file; the slowest, AdamW at n = 4096 x 1024 + 4, 1.6 s): every check passes.  Largest
|err| / E (the F64WORST lines): gemm_nt_rank 0.978, gemm_nt_rank_group 0.982, gemm_tn_rank 0.014 (fp32 only), adamw m 0.626,
v 0.527, p 0.500; rms ratio kernel / double 1.000 for both bf16 GEMM outputs; every exact profile, interval, mask, refresh and
transpose bit for bit.  Scratch mutants of three kernels fail this file where they should; two of them (the
accumulate without its intermediate bf16 rounding, AdamW without decay) pass every older test.  No kernel needed a fix."""
import pytest
import torch

import lora_ref64 as L
from fake_ops import FakeOps
from test_lora_ref64_cpu import MASK_CASES, adam_check, elementwise_check, hold_gemm, mask_check, transpose_check

pytestmark = pytest.mark.gpu
F64, F32, BF, I32, I64 = torch.float64, torch.float32, torch.bfloat16, torch.int32, torch.int64


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


def cuda(t):
    return t.cuda()


_worst, _ratios = {}, {}


def note(op, what, w):
    _worst[op] = max(_worst.get(op, 0.0), w)
    print(f"F64WORST {op} {what} |err| / E {w:.3f} (largest so far for {op}: {_worst[op]:.3f})")


def rms_ratio(op, what, got, dbl, ref):
    """the bf16 output's rms(err / (u |c|)) over |c| >= 2^-6 against the double's, where at least 4096 elements qualify"""
    want = ref.tol["cb"][0]
    k, n = L.rms_u(got, want)
    kd, _ = L.rms_u(dbl, want)
    if n < 4096:
        return
    _ratios[op] = max(_ratios.get(op, 0.0), k / kd)
    print(f"F64RATIO {op} {what} {k / kd:.3f} kernel {k:.5f} double {kd:.5f} over {n} elements (largest so far {_ratios[op]:.3f})")
    assert k <= L.RMS_RATIO * kd, f"{op} {what}: rms {k:.5f} is {k / kd:.2f} x the double's {kd:.5f} (at most {L.RMS_RATIO} x)"


# ------------------------------------------------------------------------------------------------ csrc/gemm_rank.hip
@pytest.mark.parametrize("case", L.NT_CASES, ids=L.case_id)
def test_gemm_nt_rank(hip, fake, case):
    d = L.nt_inputs(case)
    ref, got = L.gemm_reference(d), L.run_nt(hip, d, cuda)
    note("gemm_nt_rank", L.case_id(case), hold_gemm(got, ref, f"gemm_nt_rank {L.case_id(case)}"))
    if case.profile == "n01":
        rms_ratio("gemm_nt_rank", L.case_id(case), got["cb"], L.run_nt(fake, d)["cb"], ref)


@pytest.mark.parametrize("case", L.TN_CASES, ids=L.case_id)
def test_gemm_tn_rank(hip, case):
    d = L.tn_inputs(case)
    note("gemm_tn_rank", L.case_id(case), hold_gemm(L.run_tn(hip, d, cuda), L.gemm_reference(d), f"gemm_tn_rank {L.case_id(case)}"))


@pytest.mark.parametrize("case", L.GROUP_CASES, ids=L.case_id)
def test_gemm_nt_rank_group(hip, fake, case):
    d = L.group_inputs(case)
    got, dbl = L.run_group(hip, d, cuda), L.run_group(fake, d)
    for t, m in enumerate(d["members"]):
        ref = L.gemm_reference(m)
        what = f"{L.case_id(case)} member {t} K {m['K']}"
        note("gemm_nt_rank_group", what, hold_gemm({"cb": got[f"cb{t}"]}, ref, f"gemm_nt_rank_group {what}"))
        if case.profile == "n01":
            rms_ratio("gemm_nt_rank_group", what, got[f"cb{t}"], dbl[f"cb{t}"], ref)


def refused(call, outs, what):
    """`call` must raise the operator error and leave every NaN-filled output as it was"""
    from ps_slm_amd.ops import TasuOpError
    with pytest.raises(TasuOpError):
        call()
    torch.cuda.synchronize()
    assert all(L.untouched(o.cpu()) for o in outs), f"{what}: a refused call wrote to its output"


def test_gemm_rank_bad_arguments_are_refused(hip):
    M, N, K = 32, 16, 128
    a, b = torch.ones(M + 1, K + 16, dtype=BF, device="cuda"), torch.ones(72, K + 16, dtype=BF, device="cuda")
    at = torch.ones(K, 256, dtype=BF, device="cuda")
    c, cb = L.nan(256, 80).cuda(), L.nan(256, 80, dtype=BF).cuda()
    flat = a.reshape(-1)
    bad = {
        "N = 65": lambda: hip.gemm_rank(a[:M, :K], b[:65, :K], c, M, 65, K, f32=True),
        "K % 64": lambda: hip.gemm_rank(a[:M, :96], b[:N, :96], c, M, N, 96, f32=True),
        "lda < K": lambda: hip.gemm_rank(flat.as_strided((M, K), (K - 8, 1), 0), b[:N, :K], c, M, N, K, f32=True),
        "lda % 8": lambda: hip.gemm_rank(flat.as_strided((M, K), (K + 4, 1), 0), b[:N, :K], cb, M, N, K),
        "ldb % 8": lambda: hip.gemm_rank(a[:M, :K], b.reshape(-1).as_strided((N, K), (K + 4, 1), 0), cb, M, N, K),
        "A 2 bytes off": lambda: hip.gemm_rank(flat.as_strided((M, K), (K + 16, 1), 1), b[:N, :K], c, M, N, K, f32=True),
        "B 2 bytes off": lambda: hip.gemm_rank(a[:M, :K], b.reshape(-1).as_strided((N, K), (K + 16, 1), 1), c, M, N, K, f32=True),
        "tn M % 64": lambda: hip.gemm_rank_tn(at[:, :96], b[:N, :K], c, 96, N, K),
        "tn N = 65": lambda: hip.gemm_rank_tn(at[:, :64], b[:65, :K], c, 64, 65, K),
        "tn K % 64": lambda: hip.gemm_rank_tn(at[:96, :64], b[:N, :96], c, 64, N, 96),
        "tn At 2 bytes off": lambda: hip.gemm_rank_tn(at.reshape(-1).as_strided((K, 64), (256, 1), 1), b[:N, :K], c, 64, N, K),
    }
    for what, call in bad.items():
        refused(call, (c, cb), what)
    # the group: 0 and 5 members (straight on the C entry point), one misaligned member
    As, Bs = [a[:M, :K]] * 5, [b[:N, :K]] * 5
    Cs = [cb[:M, 16 * t:16 * t + N] for t in range(5)]

    def group(n, As_=As):
        rc = hip.lib.tasu_gemm_nt_rank_group(n, hip._ptrs(As_), hip._ints([x.stride(0) for x in As_]), hip._ptrs(Bs), hip._ints([x.stride(0) for x in Bs]),
                                             hip._ptrs(Cs), cb.stride(0), M, N, hip._ints([K] * 5), hip._stream())
        hip._chk(rc, "tasu_gemm_nt_rank_group")
    refused(lambda: group(0), (cb,), "a group of 0")
    refused(lambda: group(5), (cb,), "a group of 5")
    refused(lambda: group(3, [As[0], flat.as_strided((M, K), (K + 16, 1), 1), As[0], As[0], As[0]]), (cb,), "a misaligned member")
    group(3)                                                    # the same call with sound arguments goes through
    torch.cuda.synchronize()
    assert float(cb[:M, :N].float().min()) == K


# ------------------------------------------------------------------------------------------------ tasu_lora_apply, _group
@pytest.mark.parametrize("case", L.APPLY_CASES, ids=L.case_id)
def test_lora_apply_exact_profile_bits(hip, case):
    d = L.apply_inputs(case, "exact")
    for s, p, resid in L.EXACT_SETTINGS:
        if case.members and resid:
            continue
        lo, hi = L.apply_reference(d, s, p, True)
        y, x = L.run_apply(hip, d, s, p, resid, cuda)
        what = f"lora_apply exact {L.case_id(case)} s={s} p={p} resid={resid}"
        L.same_bits(y, L.to_bf(lo), what + " y")
        L.check_apply(y, x, d, (lo, hi), resid, what)


@pytest.mark.parametrize("y_zero", [True, False], ids=["y0", "yn01"])
@pytest.mark.parametrize("case", L.APPLY_CASES, ids=L.case_id)
def test_lora_apply_inside_the_interval(hip, case, y_zero):
    d = L.apply_inputs(case, "n01", y_zero)
    for s, p, resid in L.N01_SETTINGS:
        resid = resid and not case.members
        lo, hi = L.apply_reference(d, s, p, False)
        y, x = L.run_apply(hip, d, s, p, resid, cuda)
        L.check_apply(y, x, d, (lo, hi), resid, f"lora_apply n01 {L.case_id(case)} y_zero={y_zero} s={s} p={p} resid={resid}")
        print(f"F64SHARE lora_apply {L.case_id(case)} y_zero={y_zero} s={s} p={p}: ends differ on {float((lo != hi).double().mean()):.4f} of the elements")


@pytest.mark.parametrize("case", MASK_CASES, ids=L.case_id)
def test_lora_apply_mask_is_the_dropout_kernels_mask(hip, case):
    for s, p in ((1.0, 0.25), (0.3, 0.05)):
        mask_check(hip, case, s, p, cuda)


def test_lora_apply_bad_arguments_are_refused(hip):
    M, N, R = 40, 24, 64
    y = L.nan(M, N + 8, dtype=BF).cuda()
    u, w = torch.ones(M, 136, dtype=BF, device="cuda"), torch.ones(N, 136, dtype=BF, device="cuda")
    xi, xo = torch.ones(M, N + 2, device="cuda"), L.nan(M, N + 2).cuda()
    rng = torch.tensor(L.RNG, dtype=I64, device="cuda")
    ok = dict(s=1.0, p=0.0, rng=None, sid=0)
    bad = {
        "N % 8": lambda: hip.lora_apply(y[:, :12], u[:, :R], w[:12, :R], M, 12, R, **ok),
        "R = 96": lambda: hip.lora_apply(y[:, :N], u[:, :96], w[:, :96], M, N, 96, **ok),
        "ldy < N": lambda: hip.lora_apply(y.reshape(-1).as_strided((M, N), (N - 8, 1), 0), u[:, :R], w[:, :R], M, N, R, **ok),
        "x_in alone": lambda: hip.lora_apply(y[:, :N], u[:, :R], w[:, :R], M, N, R, x_in=xi[:, :N], **ok),
        "x_out alone": lambda: hip.lora_apply(y[:, :N], u[:, :R], w[:, :R], M, N, R, x_out=xo[:, :N], **ok),
        "ldx % 4": lambda: hip.lora_apply(y[:, :N], u[:, :R], w[:, :R], M, N, R, x_in=xi[:, :N], x_out=xo[:, :N], **ok),
        "p = 1": lambda: hip.lora_apply(y[:, :N], u[:, :R], w[:, :R], M, N, R, s=1.0, p=1.0, rng=rng, sid=0),
        "p < 0": lambda: hip.lora_apply(y[:, :N], u[:, :R], w[:, :R], M, N, R, s=1.0, p=-0.25, rng=rng, sid=0),
        "p > 0 without rng": lambda: hip.lora_apply(y[:, :N], u[:, :R], w[:, :R], M, N, R, s=1.0, p=0.25, rng=None, sid=0),
        "a negative stream id": lambda: hip.lora_apply(y[:, :N], u[:, :R], w[:, :R], M, N, R, s=1.0, p=0.25, rng=rng, sid=-1),
        "group R = 128": lambda: hip.lora_apply_group(y[:, :N], [u[:, :128]] * 2, [w[:, :128]] * 2, M, N, 128, [1, 2]),
        "group N % 8": lambda: hip.lora_apply_group(y[:, :12], [u[:, :R]] * 2, [w[:12, :R]] * 2, M, 12, R, [1, 2]),
        "group stream id < 0": lambda: hip.lora_apply_group(y[:, :N], [u[:, :R]] * 2, [w[:, :R]] * 2, M, N, R, [1, -2], p=0.25, rng=rng),
    }
    for what, call in bad.items():
        refused(call, (y, xo), what)


# ------------------------------------------------------------------------------------------------ elementwise, refresh, transpose
@pytest.mark.parametrize("case", L.ELEM_CASES, ids=L.case_id)
def test_lora_elementwise_bits(hip, case):
    elementwise_check(hip, case, cuda)


def test_lora_elementwise_bits_past_the_grid_of_the_eight_wide_kernels(hip):
    elementwise_check(hip, L.ELEM_BIG8, cuda, big8=True)


def test_lora_refresh_bits(hip):
    d = L.refresh_inputs()
    for got, want, ent in zip(L.run_refresh(hip, d, cuda), L.refresh_reference(d), L.REFRESH_ENTRIES):
        L.same_bits(got, want, f"lora_refresh {ent}")


@pytest.mark.parametrize("case", L.TR_CASES, ids=L.case_id)
def test_transpose_as_the_adapters_call_it(hip, case):
    transpose_check(hip, case, cuda)


# ------------------------------------------------------------------------------------------------ tasu_adamw
@pytest.mark.parametrize("case", L.ADAM_CASES, ids=L.case_id)
def test_adamw(hip, case):
    w, per = adam_check(hip, case, cuda)
    for n, x in per.items():
        note(f"adamw {n}", L.case_id(case), x)


def test_adamw_bad_arguments_are_refused(hip):
    t = [L.nan(8).cuda() for _ in range(4)]
    pb = L.nan(8, dtype=BF).cuda()
    refused(lambda: hip.adamw(t[0][:6], t[1][:6], t[2][:6], t[3][:6], pb[:6], L.LR, L.BETA1, L.BETA2, L.EPS, 0.01, 3, 1.0), (t[0], t[2], t[3], pb), "n % 4")
    refused(lambda: hip.adamw(t[0], t[1], t[2], t[3], pb, L.LR, L.BETA1, L.BETA2, L.EPS, 0.01, 0, 1.0), (t[0], t[2], t[3], pb), "step = 0")
