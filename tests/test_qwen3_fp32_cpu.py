"""Qwen3 decoders with train_config.use_fp16=false, on the CPU: the three fp32 head-norm entry points in the header, the binding
and the library (argument errors before any launch), the capability check that took the place of the refusal (model_factory and
LLMWeights.add_layer serve an operator set whose CLASS has the three operators), and the premise the GPU tests rest on: the fp32
restatement reproduces the REAL reference's tokens on all cases of tests/golden/mid_qwen3_generate.npz and keeps them under
+-2e-5 relative logit noise."""
import ctypes
import os

import pytest
import torch

import qwen3_f32_ref as F
import qwen3_ref as R
from conftest import ROOT
from penalty_ref import same
from ps_slm_amd.config import ModelConfig, TrainConfig
from ps_slm_amd.model import F32_QK_NORM_OPS, TasuModel, f32_qk_norm_missing
from ps_slm_amd.ps_slm import model_factory
from ps_slm_amd.synthetic import qwen3_state_dict
from qwen3_f32_ops import Qwen3F32FakeOps
from qwen3_ops import Qwen3FakeOps

NAMES = ("tasu_f32_qk_norm_rope", "tasu_f32_qk_norm_bwd", "tasu_f32_gemm_qkv_norm_rope")
ERR_ARG = 1


def test_header_binding_and_library_agree():
    from ps_slm_amd import _lib
    txt = open(os.path.join(ROOT, "include", "tasu_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in txt and name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION >= 26 and f"#define TASU_ABI_VERSION {_lib.ABI_VERSION}" in txt
    lib = _lib.load()
    assert lib.tasu_abi_version() == _lib.ABI_VERSION
    from ps_slm_amd.ops import HipOps
    assert f32_qk_norm_missing(None) == () and all(callable(getattr(HipOps, n, None)) for n in F32_QK_NORM_OPS)


@pytest.fixture(scope="module")
def host():
    """host buffers: every call below is refused before any launch, so no pointer is ever dereferenced"""
    from ps_slm_amd import _lib
    buf = torch.zeros(4 * 4 * 128 + 64)
    p = buf.data_ptr()
    assert p % 16 == 0
    return _lib.load(), p, buf


def test_row_entry_points_refuse_bad_arguments_before_any_launch(host):
    lib, p, _ = host
    M, H, G, eps = 2, 2, 1, 1e-6

    def fwd(pre=p, wq=p, wk=p, cos=p, sin=p, out=p, rstd=None, M=M, H=H, G=G, eps=eps, kc=None, vc=None, slot=None, ctx=0):
        return lib.tasu_f32_qk_norm_rope(pre, wq, wk, cos, sin, out, rstd, M, H, G, ctypes.c_float(eps), kc, vc, slot, ctx, None)

    for name in ("pre", "wq", "wk", "cos", "sin", "out"):
        assert fwd(**{name: None}) == ERR_ARG, name                 # NULL operands
        assert fwd(**{name: p + 4}) == ERR_ARG, name                # misaligned 16-byte operands
    assert fwd(H=3, G=2) == ERR_ARG                                 # H % G
    assert fwd(M=0) == ERR_ARG and fwd(G=0) == ERR_ARG and fwd(eps=-1.0) == ERR_ARG
    assert fwd(out=p + 16) == ERR_ARG                               # an overlap other than out == pre
    assert fwd(kc=p) == ERR_ARG and fwd(kc=p, vc=p, slot=p, ctx=0) == ERR_ARG and fwd(kc=p + 4, vc=p, slot=p, ctx=4) == ERR_ARG

    def bwd(dqkv=p, pre=p + 4096, wq=p, wk=p, rstd=p, M=M, H=H, G=G):
        return lib.tasu_f32_qk_norm_bwd(dqkv, pre, wq, wk, rstd, M, H, G, None)

    for name in ("dqkv", "pre", "wq", "wk", "rstd"):
        assert bwd(**{name: None}) == ERR_ARG, name
    for name in ("dqkv", "pre", "wq", "wk"):
        assert bwd(**{name: p + 4}) == ERR_ARG, name
    assert bwd(H=3, G=2) == ERR_ARG and bwd(M=-1) == ERR_ARG
    assert bwd(pre=p) == ERR_ARG                                    # dqkv == pre


def test_fused_entry_point_refuses_bad_arguments_before_any_launch(host):
    lib, p, _ = host
    M, H, G, K = 2, 2, 1, 32

    def fused(A=p, lda=K, W=p, ldw=K, bias=None, qkv=p, wq=p, wk=p, cos=p, sin=p, M=M, H=H, G=G, K=K, eps=1e-6, kc=None, vc=None, slot=None,
              ctx=0, ws=None, nws=0):
        return lib.tasu_f32_gemm_qkv_norm_rope(A, lda, W, ldw, bias, qkv, wq, wk, cos, sin, M, H, G, K, ctypes.c_float(eps), kc, vc, slot, ctx,
                                               ws, nws, None)

    for name in ("A", "W", "qkv", "wq", "wk", "cos", "sin"):
        assert fused(**{name: None}) == ERR_ARG, name
        assert fused(**{name: p + 4}) == ERR_ARG, name
    assert fused(bias=p + 4) == ERR_ARG and fused(ws=p + 4, nws=1 << 20) == ERR_ARG
    assert fused(H=3, G=2) == ERR_ARG
    assert fused(M=0) == ERR_ARG and fused(K=48) == ERR_ARG and fused(eps=-1.0) == ERR_ARG and fused(lda=K + 1) == ERR_ARG
    assert fused(kc=p) == ERR_ARG and fused(kc=p, vc=p, slot=p, ctx=0) == ERR_ARG


# ------------------------------------------------------------------------------------------------ the capability check
SERVED = dict(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=False)


def factory(ops, **flags):
    tc = TrainConfig(**dict(SERVED, **flags))
    mc = ModelConfig(llm_path="synthetic:mid-qwen3", encoder_projector="linear-silu", llm_dim=256)
    return model_factory(tc, mc, device="cpu", ops=ops, init_seed=1234, with_encoder=True)[0]


def test_factory_serves_an_operator_set_with_the_fp32_head_norm():
    """use_fp16=false on a Qwen3 llm_path builds for a backend whose class has the three operators; one without them is still
    refused with the missing operators' names, and the other two Qwen3 refusals stand"""
    assert f32_qk_norm_missing(Qwen3F32FakeOps()) == () and f32_qk_norm_missing(Qwen3FakeOps()) == F32_QK_NORM_OPS
    model = factory(Qwen3F32FakeOps())
    assert model.core.geo.qk_norm and not model.core.geo.qkv_bias
    with pytest.raises(NotImplementedError, match="use_fp16") as exc:
        factory(Qwen3FakeOps())
    assert all(n in str(exc.value) for n in F32_QK_NORM_OPS)
    with pytest.raises(NotImplementedError, match="use_peft"):
        factory(Qwen3F32FakeOps(), use_peft=True, peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0))
    with pytest.raises(NotImplementedError, match="freeze_llm"):
        factory(Qwen3F32FakeOps(), freeze_llm=False)


def test_fp32_layer_set_carries_the_head_norms():
    g3 = R.mid_qwen3_geometry()
    sd = qwen3_state_dict(g3, 3)
    m = TasuModel(g3, Qwen3F32FakeOps(), "cpu")
    m.llm.keep_f32 = True
    m.load_reference_state_dict(sd)
    assert len(m.llm.f32["layers"]) == g3.llm_layers
    for l, f in enumerate(m.llm.f32["layers"]):
        p = f"llm.model.layers.{l}.self_attn."
        assert f["q_norm"].dtype == torch.float32 and f["q_norm"].shape == (128,)
        assert torch.equal(f["q_norm"], sd[p + "q_norm.weight"]) and torch.equal(f["k_norm"], sd[p + "k_norm.weight"])
        assert torch.equal(f["wqkv"], torch.cat([sd[p + f"{x}_proj.weight"] for x in "qkv"]))
    bare = {k: v for k, v in sd.items() if not k.endswith("_norm.weight") or "self_attn" not in k}
    f = TasuModel(g3, Qwen3F32FakeOps(), "cpu")
    f.llm.keep_f32 = True
    with pytest.raises(KeyError, match="q_norm"):
        f.load_reference_state_dict(bare)
    short = dict(sd)
    short["llm.model.layers.0.self_attn.k_norm.weight"] = torch.ones(64)
    with pytest.raises(KeyError, match="k_norm"):
        f.load_reference_state_dict(short)
    # a backend without the operators: the refusal names qk_norm, as before
    old = TasuModel(g3, Qwen3FakeOps(), "cpu")
    old.llm.keep_f32 = True
    with pytest.raises(NotImplementedError, match="qk_norm"):
        old.load_reference_state_dict(sd)


def test_fp32_layer_on_the_double_matches_the_restatement():
    """decode_fp32._layer_fp32's choice of operator, on the CPU double: a qk_norm geometry calls f32_gemm_qkv_norm_rope with the
    layer's q_norm / k_norm and no bias, or -- the training step's kept (pre, rstd) -- the plain GEMM and the row operator, with the
    same result"""
    from types import SimpleNamespace

    from ps_slm_amd import decode_fp32

    class Rec(Qwen3F32FakeOps):
        def __init__(self):
            super().__init__()
            self.seen = []

        def f32_gemm(self, a, w, c, M, N, K, bias=None, resid=None, act=0, ws=None):
            self.seen.append("f32_gemm")
            c[:M] = a[:M, :K] @ w[:N, :K].t()

        def f32_gemm_qkv_norm_rope(self, *a, **k):
            self.seen.append("f32_gemm_qkv_norm_rope")
            assert a[2] is None
            return super().f32_gemm_qkv_norm_rope(*a, **k)

        def f32_qk_norm_rope(self, *a, **k):
            self.seen.append("f32_qk_norm_rope")
            return super().f32_qk_norm_rope(*a, **k)

        def f32_gemm_resid_rmsnorm(self, *a, **k):
            raise StopIteration                                       # (the q|k|v stage is what is looked at)

    g3 = R.mid_qwen3_geometry()
    m = TasuModel(g3, Rec(), "cpu")
    m.llm.keep_f32 = True
    m.load_reference_state_dict(qwen3_state_dict(g3, 3))
    H, G, D = g3.llm_heads, g3.llm_kv_heads, g3.llm_dim
    rows, LDQ = 5, (H + 2 * G) * 128
    gen = torch.Generator().manual_seed(1)
    xn = torch.randn(rows, D, generator=gen)
    ang = torch.rand(rows, 64, generator=gen) * 6 - 3
    outs = []
    for keep in (None, (torch.zeros(rows, LDQ), torch.zeros(rows, H + G))):
        qkv, m.ops.seen = torch.zeros(rows, LDQ), []
        b = SimpleNamespace(x_in=None, x_mid=None, x_out=None, xn=xn, qkv=qkv, ao=None, gu=None, act=None, rows=rows, cos=ang.cos(),
                            sin=ang.sin(), ws=None, keep=keep is not None, qk=keep)
        with pytest.raises(StopIteration):
            decode_fp32._layer_fp32(m, 1, b, lambda *a: None)
        assert m.ops.seen == (["f32_gemm_qkv_norm_rope", "f32_qk_norm_rope"] if keep is None else ["f32_gemm", "f32_qk_norm_rope"])
        outs.append(qkv)
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0
    f = m.llm.f32["layers"][1]
    x = (xn @ f["wqkv"].t()).view(rows, H + 2 * G, 128)
    want = R.head_norm(x[:, :H], f["q_norm"], "fp32", g3.rms_eps)
    from f32_ref64 import rope_eager
    assert torch.allclose(outs[0].view(rows, H + 2 * G, 128)[:, :H], rope_eager(want, ang.cos(), ang.sin()), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the fixture premise
@pytest.fixture(scope="module")
def decode():
    return R.generate_cases()


def test_fp32_restatement_keeps_the_reference_tokens_under_noise_on_all_cases(decode):
    geo, sd, cases = decode
    assert len(cases) == 24
    bad = []
    for n, c in enumerate(cases):
        toks, stable = F.case_tokens(sd, geo, c, n)
        if not (stable and same(toks, c["tokens"])):
            bad.append((n, c["kw"], stable))
    assert not bad, bad


def test_penalty_and_sampled_case_are_stable_in_fp32(decode):
    """the fixture's own knob cases (pen_case / smp_case): jitter-stable in the fp32 restatement too, so no other index is taken"""
    geo, sd, cases = decode
    pen, smp, stable = F.knob_cases_fp32(sd, geo, cases)
    assert stable
    assert pen["kw"]["num_beams"] > 1 and pen["kw"]["repetition_penalty"] == 1.3 and smp["tokens"].shape[1] >= 4
    assert not same(pen["tokens"], cases[[i for i, c in enumerate(cases) if c["ids"] is pen["ids"]][0]]["tokens"])      # the penalty changes what is decoded
