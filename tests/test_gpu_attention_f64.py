"""The bf16 attention kernels against a float64 reference, element by element (tests/attn_ref64.py; its own checks:
tests/test_attn_ref64_cpu.py).  One reference per case; every kernel family runs on the same inputs and is held to it:

  forward    the tiled kernel (csrc/attention.hip) and the single-pass kernel (csrc/attention_sp.hip, Spad <= 256): out and lse
  backward   the per-head kernels (tasu_attn_bwd_prep + tasu_attn_bwd_rope, kernel = PER_HEAD), the single-launch GQA kernel
             (kernel = GQA, where tasu_attn_gqa_supported), the single-pass kernels (tasu_attn_bwd_fused, kernel = SP) and the
             policy entry point (tasu_attn_bwd_fused, kernel = POLICY), each fed by the out / lse of its own family's forward:
             the whole finished dqkv, the q, k and v blocks reported separately

on EVERY row < S -- the rows of masked tokens and the rows without a visible key included: the model feeds all M rows of dqkv
and of the attention output to the weight-gradient GEMMs, so a stale or non-finite word in a padded token's row poisons them.
Every output and scratch buffer (out, lse, delta, dqkv, dk_part, dv_part) starts as NaN: a row nobody writes, or a workspace read
before it is written, fails.

First check: |got - ref| <= 1.1 x E elementwise, exactly 0 where E = 0 (the bound E and the derivation of 1.1: attn_ref64.py).
Second check: rms(err / E) of out, dq, dk and dv at most 1.5 x that of the torch double (tests/fake_ops.py) on the same inputs,
computed here on the CPU: the kernels share the double's rounding points, so the statistic matches up to the association of the
fp32 sums, while a systematic bias such as truncation shows as 2.3 x or more.  Third: every backward family gives the same bits
twice.

Largest rms ratio measured per family over the case list (MI355X):
    forward    tiled 1.000                                  single pass 1.000
    backward   per-head  dq 1.010, dk 1.009, dv 1.001       GQA          dq 1.010, dk 1.009, dv 1.001
               single pass dq 1.003, dk 1.008, dv 1.001     policy       dq 1.010, dk 1.009, dv 1.001
(At S = 1 the reference's ds is exactly 0, so dq and dk are fp32 noise there: both statistics are about 1e-6.)
Scratch mutants of the kernels fail it: the GQA dK / dV sweep without the last query row -- |err| / E = 30-39 at the named dk
element; pack_pair truncating instead of rounding -- the forward bound (1.12-1.13) and the rms check (dk 1.57-1.60 x)."""
import pytest
import torch

import attn_ref64 as R
from fake_ops import FakeOps

pytestmark = pytest.mark.gpu
HD = R.HD
BF = torch.bfloat16
NAN = float("nan")
RMS_RATIO = 1.5
PER_HEAD, GQA = 1, 2                                            # TASU_ATTN_KERNEL_*


@pytest.fixture(scope="module")
def hip():
    from ps_slm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def fake():
    return FakeOps()


class State:
    """inputs (host and device), the float64 reference, the double's rms and the forwards run so far of one case"""

    def __init__(self, case, fake):
        self.case = case
        self.inp = R.make_inputs(case)
        self.ref = R.reference_of(self.inp)
        self.want_rms = R.double_rms(fake, self.inp, self.ref)
        self.dev = {k: v.cuda() for k, v in self.inp.items() if isinstance(v, torch.Tensor)}
        self.fwd = {}


_states = {}


@pytest.fixture
def state(request, fake):
    """the case's State: built once, shared by the forward and the backward test, dropped after the backward test (its last user)"""
    case = request.param
    if case not in _states:
        _states[case] = State(case, fake)
    yield _states[case]
    if request.node.name.startswith("test_backward"):
        del _states[case]


def forward(hip, st, kernel):
    """out [M, H*128], lse [B*H*Spad] of the named forward kernel, into NaN-filled buffers (device tensors, cached)"""
    if kernel not in st.fwd:
        c, i, d = st.case, st.inp, st.dev
        Spad = (c.S + 63) // 64 * 64
        out = torch.full((c.B * c.S, c.H * HD), NAN, dtype=BF, device="cuda")
        lse = torch.full((c.B * c.H * Spad,), NAN, device="cuda")
        hip.attn_fwd_on(kernel, d["qkv"], d["km"], out, lse, c.B, c.S, c.H, c.G, i["scale"], c.causal)
        torch.cuda.synchronize()
        st.fwd[kernel] = (out, lse)
    return st.fwd[kernel]


def check_rms(st, family, name, rms):
    want = st.want_rms[name]
    print(f"F64RATIO {family} {name} {rms / want if want > 0 else 0.0:.3f} kernel {rms:.5f} double {want:.5f} {R.case_id(st.case)}")
    assert rms <= RMS_RATIO * want, (f"{family} {name}: rms(err / E) {rms:.5f} is {rms / max(want, 1e-300):.2f} x the double's {want:.5f} "
                                     f"(at most {RMS_RATIO} x: a systematic error, not rounding)")


def sp_served(hip, c):
    return hip.lib.tasu_attn_sp_supported(c.S, c.H, c.G) == 1


def gqa_served(hip, c):
    return hip.lib.tasu_attn_gqa_supported(c.S, c.H, c.G) == 1


@pytest.mark.parametrize("state", R.CASES, ids=R.case_id, indirect=True)
def test_forward_against_float64(hip, state):
    c, ref = state.case, state.ref
    assert sp_served(hip, c) == ((c.S + 63) // 64 * 64 <= 256)
    for kernel in ("tiled", "sp") if sp_served(hip, c) else ("tiled",):
        out, lse = forward(hip, state, kernel)
        rms = R.assert_within(out.cpu().view(c.B, c.S, c.H, HD), ref.out, ref.E_out, R.LIMIT, f"{kernel} forward, out")
        R.assert_within(R.lse_rows(lse.cpu(), c.B, c.S, c.H), ref.lse, ref.E_lse, R.LIMIT, f"{kernel} forward, lse")
        check_rms(state, f"fwd-{kernel}", "out", rms)


def backward(hip, st, family):
    """the finished dqkv [M, (H+2G)*128] of one backward family, every buffer NaN beforehand"""
    c, i, d = st.case, st.inp, st.dev
    B, S, H, G = c.B, c.S, c.H, c.G
    M, LD, Spad = B * S, (H + 2 * G) * HD, (S + 63) // 64 * 64
    out, lse = forward(hip, st, "sp" if family == "sp" else "tiled")
    dqkv = torch.full((M, LD), NAN, dtype=BF, device="cuda")
    dkp, dvp = torch.full((M, H * HD), NAN, device="cuda"), torch.full((M, H * HD), NAN, device="cuda")
    delta = torch.full((B * H * Spad,), NAN, device="cuda")
    if family in ("per_head", "gqa"):
        hip.attn_bwd_prep(d["dout"], out, delta, None, B, S, H)
        hip.attn_bwd_rope(d["qkv"], d["km"], d["dout"], lse, delta, d["cos"], d["sin"], dqkv, dkp, dvp, B, S, H, G, i["scale"], c.causal,
                          PER_HEAD if family == "per_head" else GQA)
    else:
        hip.attn_bwd_fused(d["qkv"], d["km"], d["dout"], out, lse, delta, d["cos"], d["sin"], dqkv, dkp, dvp, B, S, H, G, i["scale"],
                           c.causal, family)
    torch.cuda.synchronize()
    return dqkv.cpu()


@pytest.mark.parametrize("state", R.CASES, ids=R.case_id, indirect=True)
def test_backward_against_float64(hip, state):
    from ps_slm_amd.ops import TasuOpError
    c, ref = state.case, state.ref
    B, S, H, G = c.B, c.S, c.H, c.G
    assert gqa_served(hip, c) == (H // G >= 2 and S <= 4096)
    families = ["per_head"] + (["gqa"] if gqa_served(hip, c) else []) + (["sp"] if sp_served(hip, c) else []) + ["policy"]
    if not gqa_served(hip, c):                                   # H == G, S > 4096: refused, not served wrongly
        with pytest.raises(TasuOpError, match="bad argument"):
            backward(hip, state, "gqa")
    for family in families:
        dqkv = backward(hip, state, family)
        for name, got, want, E in R.blocks(dqkv, ref, B, S, H, G):
            check_rms(state, family, name, R.assert_within(got, want, E, R.LIMIT, f"{family} backward, {name}"))
        again = backward(hip, state, family)
        assert torch.equal(again.view(torch.int16), dqkv.view(torch.int16)), f"{family} backward: two runs, different bits"
