"""Full fine-tuning of a Qwen3 decoder (train_config.freeze_llm=false on a qk_norm geometry), host logic on the CPU double: the
REAL host code of ps_slm_amd/full_ft.py + model.py + ps_slm.py + engine.py driven through tests/qwen3_full_ft_ops.py, against
goldens produced by the real reference with a Qwen3ForCausalLM whose every parameter trains (tools/make_golden_qwen3_full_ft.py);
the bucket's layout, the checkpoint names, and the capability check that took the place of the refusal."""
import numpy as np
import pytest
import torch

import qwen3_ref as R
from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
from ps_slm_amd.engine import TasuEngine
from ps_slm_amd.full_ft import EMBED_KEY, HEAD_KEY, NORM_KEY
from ps_slm_amd.model import Geometry, TasuModel, qk_norm_wgrad_missing, rup
from ps_slm_amd.ps_slm import model_factory
from ps_slm_amd.synthetic import MID_GEOMETRY, qwen3_state_dict, random_state_dict, synthetic_text_batch
from qwen3_full_ft_ops import GOLDENS, Qwen3FullFtFakeOps, build_ft, check_step_against_golden, golden_case, n_llm_tensors
from qwen3_ops import Qwen3FakeOps
from test_lora_cpu import run_text, to_call

HD = 128
SERVED = dict(freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=True)


def factory(ops, freeze_llm=False, seed=1234, **flags):
    tc = TrainConfig(freeze_llm=freeze_llm, **dict(SERVED, **flags))
    mc = ModelConfig(llm_path="synthetic:mid-qwen3", encoder_projector="linear-silu", llm_dim=256)
    return model_factory(tc, mc, device="cpu", ops=ops, init_seed=seed)[0]


def engine(model, lr=2e-2):
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg.update(lr=lr, gradient_accumulation_steps=1)
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10                      # past the zero-lr warm-up steps
    return eng


def raw_batch(geo, seed=5):
    return synthetic_text_batch(geo, 2, seed=seed, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)


@pytest.mark.parametrize("name", GOLDENS)
def test_qwen3_full_ft_step_vs_reference_golden(name):
    z, geo, sd, batch = golden_case(name)
    m = build_ft(geo, sd, Qwen3FullFtFakeOps(), "cpu")
    st = run_text(m, batch)
    check_step_against_golden(m, st, z, show=name)


def test_exchanged_weight_gradients_miss_the_golden():
    """what the fixture is built to see: dwq and dwk exchanged in the double fails the bar of the head norms"""
    z, geo, sd, batch = golden_case(GOLDENS[0])
    ops = Qwen3FullFtFakeOps()
    ops.mutant = "swap"
    m = build_ft(geo, sd, ops, "cpu")
    st = run_text(m, batch)
    with pytest.raises(AssertionError, match="_norm.weight"):
        check_step_against_golden(m, st, z)


def expected_offsets(geo, proj_numel, qwen3):
    """the bucket's layout computed here: [projector | norm | head (untied) | layers, last first | table], every tensor on a
    multiple of 64 elements, a layer in the order the backward completes its tensors"""
    D, I, Q, KV = geo.llm_dim, geo.llm_inter, geo.llm_heads * HD, geo.llm_kv_heads * HD
    sizes = {"wd": D * I, "wgu": 2 * I * D, "ln2": D, "wo": D * Q, "q_norm": HD, "k_norm": HD, "wqkv": (Q + 2 * KV) * D, "bqkv": Q + 2 * KV,
             "ln1": D}
    order = ("wd", "wgu", "ln2", "wo", "q_norm", "k_norm", "wqkv", "ln1") if qwen3 else ("wd", "wgu", "ln2", "wo", "wqkv", "bqkv", "ln1")
    off, out = rup(proj_numel, 64), {}
    out[("norm", None)] = off
    off += rup(D, 64)
    if not geo.tied:
        out[("head", None)] = off
        off += rup(geo.llm_vocab * D, 64)
    for l in range(geo.llm_layers - 1, -1, -1):
        for n in order:
            out[(n, l)] = off
            off += rup(sizes[n], 64)
    return out, off


@pytest.mark.parametrize("tied", [True, False])
def test_bucket_layout_of_a_qwen3_decoder(tied):
    import dataclasses
    geo = dataclasses.replace(R.mid_qwen3_geometry(), tied=tied)
    m = TasuModel(geo, Qwen3FullFtFakeOps(), "cpu")
    m.load_reference_state_dict(qwen3_state_dict(geo, 3))
    numel = m.proj.numel
    m.enable_llm_training()
    ft, pr = m.full_ft, m.proj
    want, end = expected_offsets(geo, numel, True)
    assert {k: v[0] for k, v in ft.offsets.items()} == want and ft.end == end
    assert all(off % 64 == 0 for off in want.values()) and not any(n == "bqkv" for n, _ in ft.offsets)
    for l in range(geo.llm_layers):                                     # after wo, before wqkv; one contiguous range per layer
        assert want[("wo", l)] < want[("q_norm", l)] < want[("k_norm", l)] < want[("wqkv", l)] < want[("ln1", l)]
        assert ft.layer_range[l] == (want[("wd", l)], want[("ln1", l)] + rup(geo.llm_dim, 64))
    assert ft.grad_ranges() == [(ft.lo, ft.layers_lo)] + [ft.layer_range[l] for l in range(geo.llm_layers - 1, -1, -1)]
    cover = sorted(m.grad_ranges(1))
    assert cover[0][0] == 0 and cover[-1][1] == pr.numel and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    # the kernels' tensors are views of the bucket: the head norms of the fp32 masters, the zero bias outside it
    lo_p, hi_p = pr.p.data_ptr(), pr.p.data_ptr() + 4 * pr.numel
    for l, w in enumerate(m.llm.layers):
        assert w["q_norm"].data_ptr() == ft.view(pr.p, "q_norm", l).data_ptr() and w["k_norm"].data_ptr() == ft.view(pr.p, "k_norm", l).data_ptr()
        assert w["q_norm"].dtype == torch.float32 and w["wqkv"].data_ptr() == ft.view(pr.pb, "wqkv", l).data_ptr()
        assert not lo_p <= w["bqkv"].data_ptr() < hi_p and float(w["bqkv"].abs().max()) == 0
        assert not pr.pb.data_ptr() <= w["bqkv"].data_ptr() < pr.pb.data_ptr() + 2 * pr.numel
    names = [k for k, *_ in ft.names()]
    assert len(names) == n_llm_tensors(geo) - 1 and not any(k.endswith(".bias") for k in names)
    assert all(f"llm.model.layers.{l}.self_attn.{n}_norm.weight" in names for l in range(geo.llm_layers) for n in "qk")
    assert ft.num_parameters() == sum(int(np.prod(s)) for _, s in ft.offsets.values())


@pytest.mark.parametrize("tied", [True, False])
def test_a_qwen2_bucket_is_unchanged(tied):
    geo = Geometry.from_dict(dict(MID_GEOMETRY, tied=tied))
    m = TasuModel(geo, Qwen3FullFtFakeOps(), "cpu")
    m.load_reference_state_dict(random_state_dict(geo, 3, with_encoder=False))
    numel = m.proj.numel
    m.enable_llm_training()
    want, end = expected_offsets(geo, numel, False)
    assert {k: v[0] for k, v in m.full_ft.offsets.items()} == want and m.full_ft.end == end
    names = [k for k, *_ in m.full_ft.names()]
    assert len(names) == 12 * geo.llm_layers + 1 + (0 if tied else 1) and not any("_norm.weight" in k and "self_attn" in k for k in names)
    assert sum(k.endswith(".bias") for k in names) == 3 * geo.llm_layers


def test_factory_serves_full_fine_tuning_on_an_operator_set_with_the_weight_gradient():
    assert qk_norm_wgrad_missing(Qwen3FullFtFakeOps()) is None and qk_norm_wgrad_missing(Qwen3FakeOps()) == "qk_norm_wgrad"
    model = factory(Qwen3FullFtFakeOps())
    core = model.core
    assert core.geo.qk_norm and core.full_ft is not None and core.arith_train == "bf16"
    named = dict(model.named_parameters())
    assert len(named) == 6 + n_llm_tensors(core.geo) and sorted(named) == sorted(model.state_dict())
    assert sum(k.endswith(("q_norm.weight", "k_norm.weight")) for k in named) == 2 * core.geo.llm_layers and not any(".bias" in k for k in named if k.startswith("llm."))
    with pytest.raises(NotImplementedError, match="freeze_llm") as exc:
        factory(Qwen3FakeOps())
    assert "qk_norm_wgrad" in str(exc.value)
    with pytest.raises(NotImplementedError, match="use_peft"):
        factory(Qwen3FullFtFakeOps(), freeze_llm=True, use_peft=True, peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0))
    old = TasuModel(core.geo, Qwen3FakeOps(), "cpu")
    old.load_reference_state_dict(qwen3_state_dict(core.geo, 3))
    with pytest.raises(NotImplementedError, match="qk_norm") as exc:
        old.enable_llm_training()
    assert "qk_norm_wgrad" in str(exc.value)


def test_engine_step_moves_every_tensor_and_the_checkpoint_round_trips():
    """one engine step moves every tensor, the head norms among them; state_dict() carries the new keys and no bias; it loads into a
    trainable model and -- load_llm_tensors -- into a FROZEN Qwen3 model, which then computes the stepped model's eval loss"""
    model = factory(Qwen3FullFtFakeOps())
    eng = engine(model)
    geo = model.core.geo
    raw = raw_batch(geo)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    eng.step()
    sd = model.state_dict()
    assert len(sd) == 6 + n_llm_tensors(geo) and all(v.dtype == torch.float32 for v in sd.values())
    assert not any(k.endswith(".bias") for k in sd if k.startswith("llm."))
    for k, v in sd.items():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, before[k]), k
    for l in range(geo.llm_layers):
        for n in "qk":
            assert sd[f"llm.model.layers.{l}.self_attn.{n}_norm.weight"].shape == (HD,)
    w = model.core.llm.layers[0]
    assert torch.equal(w["q_norm"], sd["llm.model.layers.0.self_attn.q_norm.weight"]) and float(w["bqkv"].abs().max()) == 0
    want = float(model.eval()(**to_call(raw))[0].loss.detach())
    for frozen in (False, True):
        m2 = factory(Qwen3FullFtFakeOps() if not frozen else Qwen3FakeOps(), freeze_llm=frozen, seed=99)
        was = float(m2.eval()(**to_call(raw))[0].loss.detach())
        missing, unexpected = m2.load_state_dict(dict(sd, **{HEAD_KEY: sd[EMBED_KEY]}))       # tied: a lm_head key is ignored
        assert not missing and not unexpected
        assert (m2.core.full_ft is None) == frozen
        assert float(m2.eval()(**to_call(raw))[0].loss.detach()) == want != was
    # a frozen model needs the whole decoder: the norm keys are required, bias keys are not
    part = {k: v for k, v in sd.items() if not k.endswith("layers.1.self_attn.k_norm.weight")}
    with pytest.raises(KeyError, match="k_norm"):
        factory(Qwen3FakeOps(), freeze_llm=True).load_state_dict(part)
    assert NORM_KEY in sd and EMBED_KEY in sd


def test_load_llm_tensors_on_a_frozen_core():
    geo = R.mid_qwen3_geometry()
    sd_a, sd_b = qwen3_state_dict(geo, 3), qwen3_state_dict(geo, 4)
    m = TasuModel(geo, Qwen3FakeOps(), "cpu")
    m.load_reference_state_dict(sd_a)
    llm_b = {k: v for k, v in sd_b.items() if k.startswith("llm.")}
    assert not any(k.endswith(".bias") for k in llm_b)
    m.load_llm_tensors(llm_b)
    for l, w in enumerate(m.llm.layers):
        assert torch.equal(w["q_norm"], sd_b[f"llm.model.layers.{l}.self_attn.q_norm.weight"])
        assert torch.equal(w["k_norm"], sd_b[f"llm.model.layers.{l}.self_attn.k_norm.weight"]) and float(w["bqkv"].abs().max()) == 0
    with pytest.raises(KeyError, match="q_norm"):
        m.load_llm_tensors({k: v for k, v in llm_b.items() if not k.endswith("layers.0.self_attn.q_norm.weight")})


# the operator calls of one frozen Qwen3 step on the CPU double (which composes some operators of others), recorded on the commit
# before the head norms' weight gradients existed
FROZEN_FWD = ["posterior_build", "layernorm_fwd", "gemm", "silu_fwd", "gemm", "embed_merge", "rope_table"] + \
    2 * ["rmsnorm_fwd", "gemm", "qk_norm_rope_fwd", "attn_fwd", "gemm", "rmsnorm_fwd", "gemm_gate_up_swiglu", "gemm", "swiglu_fwd", "gemm"] + \
    ["rmsnorm_fwd", "gemm", "ce_fwd_bwd", "ce_reduce"]
FROZEN_BWD = ["gemm", "rmsnorm_bwd"] + \
    2 * ["gemm_dswiglu", "gemm", "swiglu_bwd", "gemm", "rmsnorm_bwd", "gemm", "attn_bwd_fused", "attn_bwd_prep", "attn_bwd_rope", "attn_bwd",
         "attn_bwd_dq", "attn_bwd_dkv", "rope_bwd", "qk_norm_bwd", "gemm", "rmsnorm_bwd"] + \
    ["merge_bwd", "colsum", "transpose", "transpose", "gemm", "gemm", "silu_bwd", "colsum", "transpose", "transpose", "gemm", "gemm",
     "layernorm_bwd_params"]


def recorded_step(m):
    raw = raw_batch(m.geo)
    st = m.prepare_text(raw["input_ids"], raw["attention_mask"], raw["labels"], raw["post_ids"])
    m.ops.calls = []
    m.forward_projector_text(st)
    m.forward_llm(st)
    n = len(m.ops.calls)
    m.backward(st)
    calls, m.ops.calls = m.ops.calls, None
    return calls[:n], calls[n:]


def test_a_frozen_step_issues_the_calls_it_issued_before_and_the_trainable_one_reads_dqkv_first():
    geo = R.mid_qwen3_geometry()
    assert geo.llm_layers == 2
    sd = qwen3_state_dict(geo, 3)
    for ops in (Qwen3FakeOps(), Qwen3FullFtFakeOps()):                   # the new operators' presence changes nothing
        m = TasuModel(geo, ops, "cpu")
        m.load_reference_state_dict(sd)
        fwd, bwd = recorded_step(m)
        assert fwd == FROZEN_FWD and bwd == FROZEN_BWD
    m = build_ft(geo, sd, Qwen3FullFtFakeOps(), "cpu")
    _, bwd = recorded_step(m)
    at = [i for i, n in enumerate(bwd) if n == "qk_norm_wgrad"]
    assert len(at) == geo.llm_layers and all(bwd[i + 1] == "qk_norm_bwd" and bwd[i - 1] == "rope_bwd" for i in at)
    assert "colsum_split" not in bwd and bwd.count("rmsnorm_wgrad") == 2 * geo.llm_layers + 1       # no bias gradient; every norm's
