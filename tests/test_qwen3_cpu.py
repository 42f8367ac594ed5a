"""Qwen3 decoders (per-head q/k RMSNorm, no q|k|v bias) on the CPU: the restatement tests/qwen3_ref.py against the REAL reference's
fixtures (tests/golden/mid_qwen3_step.npz, mid_qwen3_generate.npz; tools/make_golden_qwen3.py), the product through the CPU double
(tests/qwen3_ops.py) against the step fixture and the stable decode cases, the plugin's refusals and the weight loaders."""
import dataclasses
import json

import pytest
import torch

import qwen3_ref as R
from penalty_ref import prompt_embeddings, same
from ps_slm_amd.config import ModelConfig, TrainConfig
from ps_slm_amd.decode import beam_search_generate
from ps_slm_amd.model import Geometry, TasuModel
from ps_slm_amd.ps_slm import geometry_from_config, model_factory
from ps_slm_amd.synthetic import MID_GEOMETRY, qwen3_state_dict, random_state_dict
from qwen3_ops import Qwen3FakeOps

SERVED = dict(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=True)


def factory(llm_path="synthetic:mid-qwen3", ops=None, **flags):
    tc = TrainConfig(**dict(SERVED, **flags))
    mc = ModelConfig(llm_path=llm_path, encoder_projector="linear-silu", llm_dim=256)
    return model_factory(tc, mc, device="cpu", ops=ops or Qwen3FakeOps(), init_seed=1234, with_encoder=True)[0]


@pytest.fixture(scope="module")
def step():
    return R.step_case()


@pytest.fixture(scope="module")
def decode():
    geo, sd, cases = R.generate_cases()
    double = TasuModel(geo, Qwen3FakeOps(), "cpu")
    double.load_reference_state_dict(sd)
    return geo, sd, cases, double


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("tag", ["text", "audio"])
def test_restatement_in_fp32_reproduces_the_reference_step(step, tag):
    """the fp32 bars of tests/test_gpu_model.py: loss 2e-5 relative, projector gradients 2e-4 relative L2"""
    geo, sd, batch, z = step
    out, grads = R.loss_and_projector_grads(sd, batch, dataclasses.asdict(geo), "fp32", audio=tag == "audio")
    ref = float(z[f"{tag}_loss"])
    assert abs(float(out["loss"].detach()) - ref) <= 2e-5 * abs(ref)
    assert abs(float(out["acc"]) - float(z[f"{tag}_acc"])) < 1e-6
    for k, g in grads.items():
        assert R.rel_l2(g, torch.from_numpy(z[f"{tag}_grad." + k[len("encoder_projector."):]])) < 2e-4, k
    lg, want = out["logits"].detach()[:, :, torch.from_numpy(z["cols"])], torch.from_numpy(z[f"{tag}_logits_cols"])
    valid = out["mask"].bool()
    assert float((lg - want)[valid].abs().max() / want[valid].abs().max()) < 2e-5


def test_restatement_without_the_norm_misses_the_reference(step):
    """what the fixture is built to see: ten times the bf16 loss bar"""
    geo, sd, batch, z = step
    with torch.no_grad():
        bare = float(R.forward_text(sd, batch, dataclasses.asdict(geo), "fp32", variant="no-norm")["loss"])
    assert abs(bare - float(z["text_loss"])) > 10 * 2e-2


def test_generate_fixture_covers_what_it_claims(decode):
    _, _, cases, _ = decode
    kws = [c["kw"] for c in cases]
    assert len(cases) >= 24 and {k["num_beams"] for k in kws} == {1, 2, 4, 5, 8, 16}
    assert sum(k["min_length"] > c["ids"].shape[1] + 3 for k, c in zip(kws, cases)) >= 2          # an active EOS ban
    assert sum(k["length_penalty"] != 1.0 for k in kws) >= 2 and any(not bool(c["am"].all()) for c in cases)      # left padding
    stable = [c for c in cases if c["bf16_stable"]]
    assert len(stable) >= 8 and any(c["kw"]["num_beams"] == 1 for c in stable)
    assert 2 * sum(c["swap_differs"] for c in cases) >= len(cases)


def test_restatement_in_fp32_reproduces_the_reference_tokens_on_every_case(decode):
    geo, sd, cases, _ = decode
    gd = dataclasses.asdict(geo)
    bad = []
    with torch.no_grad():
        for n, c in enumerate(cases):
            emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
            t = R.beam_search_generate(sd, emb, mask, gd, mode="fp32", **c["kw"])
            if not same(t, c["tokens"]):
                bad.append((n, t.tolist(), c["tokens"].tolist()))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the product on the double
def run_step(core, batch, audio):
    if audio:
        st = core.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"],
                                batch["input_feature_length"])
    else:
        st = core.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], None, None)
        core.forward_projector_text(st)
    core.forward_llm(st)
    core.backward(st)
    return st


@pytest.mark.parametrize("tag", ["text", "audio"])
def test_factory_model_on_the_double_against_the_reference_step(step, tag):
    """model_factory on synthetic:mid-qwen3 with the fixture's weights, at the bars of
    tests/test_gpu_model.py::test_step_vs_reference_golden on BOTH batches: |loss - ref| < 2e-2, logits within 3e-2 of the logit
    scale; the projector gradients at that test's cosine 0.995 (text) and at the 0.99 of ::test_audio_step_without_merging (audio).
    On the audio branch the bf16 encoder's posterior noise reaches the logits, so a correct bf16 evaluation lies 2e-2 .. 3.8e-2 of
    the logit scale from fp32 depending on the feature draw; the fixture's features are the draw on which the ORACLE's bf16 mode lies
    closest (2.04e-2; tools/make_golden_qwen3.py: step_fixture), chosen without the code under test.  The double measures 1.63e-2
    (text) and 2.42e-2 (audio)."""
    geo, sd, batch, z = step
    model = factory()
    core = model.core
    assert core.geo.qk_norm and not core.geo.qkv_bias and core.arith == "bf16"
    core.load_reference_state_dict(sd)
    st = run_step(core, batch, tag == "audio")
    assert abs(float(st.dev["loss_out"][0]) - float(z[f"{tag}_loss"])) < 2e-2
    valid = torch.from_numpy(st.plan.key_mask[:, :st.S].astype(bool))
    lg = core.logits_view(st).float()[:, :, torch.from_numpy(z["cols"])]
    ref = torch.from_numpy(z[f"{tag}_logits_cols"])
    assert float((lg - ref)[valid].abs().max() / ref[valid].abs().max()) < 3e-2
    for k, g in core.projector_grads().items():
        want = torch.from_numpy(z[f"{tag}_grad." + k[len("encoder_projector."):]])
        assert float(torch.nn.functional.cosine_similarity(g.flatten(), want.flatten(), dim=0)) > (0.995 if tag == "text" else 0.99), k


def test_plugin_forward_and_loss_backward(step):
    """the public interface: model(**batch) in training mode, outputs.loss.backward() -- the same loss and projector gradients as
    the core's hand-scheduled step, and an eval-mode forward (no backward kept) with the same loss"""
    geo, sd, batch, z = step
    model = factory()
    model.core.load_reference_state_dict(sd)
    call = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"], input_features=None,
                input_feature_length=None, GT=[" ".join(map(str, p)) for p in batch["post_ids"]])
    model.train()
    out, _ = model(**call)
    out.loss.backward()
    got = {k: v.clone() for k, v in model.core.projector_grads().items()}
    assert abs(float(out.loss) - float(z["text_loss"])) < 2e-2
    st = run_step(model.core, batch, False)
    assert float(st.dev["loss_out"][0]) == float(out.loss)
    for k, g in model.core.projector_grads().items():
        assert torch.equal(g, got[k]) and float(g.abs().max()) > 0, k
    model.eval()
    with torch.no_grad():
        ev, _ = model(**call)
    assert abs(float(ev.loss) - float(out.loss)) < 1e-5 * float(out.loss)


def test_double_against_the_restatement_in_bf16(step):
    """the bars tests/test_gpu_model.py::test_step_vs_double_and_oracle holds a bf16 step to against the oracle's bf16 mode: loss
    5e-3, projector gradients cosine 0.999"""
    geo, sd, batch, _ = step
    core = TasuModel(geo, Qwen3FakeOps(), "cpu")
    core.load_reference_state_dict(sd)
    st = run_step(core, batch, False)
    out, grads = R.loss_and_projector_grads(sd, batch, dataclasses.asdict(geo), "bf16")
    assert abs(float(st.dev["loss_out"][0]) - float(out["loss"].detach())) < 5e-3
    mine = core.projector_grads()
    for k, g in grads.items():
        assert float(torch.nn.functional.cosine_similarity(mine[k].flatten(), g.flatten(), dim=0)) > 0.999, k


def decode_on(double, geo, c, **over):
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    double.forward_projector_text(st)
    return beam_search_generate(double, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **dict(c["kw"], **over)).numpy()


def test_product_decode_loop_on_the_double_reproduces_the_stable_cases(decode):
    geo, _, cases, double = decode
    bad = [(n, c["kw"]) for n, c in enumerate(cases) if c["bf16_stable"] and not same(decode_on(double, geo, c), c["tokens"])]
    assert not bad, bad


def test_penalty_and_sampled_case_on_the_double(decode):
    """downstream of the logits: one case with repetition_penalty, one with do_sample, at the bf16 restatement's tokens"""
    geo, _, cases, double = decode
    pen, smp = R.knob_cases(cases)
    assert pen["kw"]["num_beams"] > 1 and pen["kw"]["repetition_penalty"] == 1.3 and smp["tokens"].shape[1] >= 4
    assert same(R.decode_case(double, geo, pen), pen["tokens"])
    assert same(R.decode_case(double, geo, smp), smp["tokens"])


def stored_qwen2():
    """tests/golden/qwen2_launches_and_init.json, recorded on the commit BEFORE Qwen3 was served: the operator calls of two Qwen2
    decodes on the CPU double, in order, their tokens, and digests of LLMWeights.init_random's tensors at the mid geometry"""
    import os

    from conftest import GOLDEN
    return json.load(open(os.path.join(GOLDEN, "qwen2_launches_and_init.json")))


def digest(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def test_qwen2_decode_issues_exactly_the_launches_it_did():
    """the whole call sequence of a Qwen2 generate() -- prefill, every decode position, top-k and beam update -- equals the one
    recorded before this route existed, call for call (tests/test_step_trace_cpu.py pins the training layer the same way)"""
    want = stored_qwen2()
    geo2 = Geometry.from_dict(MID_GEOMETRY)
    m = TasuModel(geo2, Qwen3FakeOps(), "cpu")
    m.load_reference_state_dict(random_state_dict(geo2, 5, with_encoder=False))
    ids = torch.tensor([[980, 980, 17, 5, 990, 44, 7], [3, 250, 61, 990, 9, 12, 800]])
    am = torch.tensor([[0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1]]).bool()
    for nb in (4, 1):                                            # (on one model, as recorded: the second call registers no weights)
        st = m.prepare_text(ids, am, None, [[5, 9, 17, 3], [8, 2, 150]], None, None)
        m.forward_projector_text(st)
        m.ops.calls = []
        toks = beam_search_generate(m, st, num_beams=nb, max_new_tokens=5, eos_token_id=-1, pad_token_id=0)
        calls, m.ops.calls = m.ops.calls, None
        assert calls == want[f"decode_calls_nb{nb}"] and toks.tolist() == want[f"decode_tokens_nb{nb}"]
        assert "gemm_skinny_qkv_rope" in calls and "gemm_qkv_rope" in calls and not any(n.startswith("qk_norm") for n in calls)


def test_qwen3_decode_takes_the_plain_projection_and_the_head_norm(decode):
    geo, _, cases, double = decode
    double.ops.calls = []
    decode_on(double, geo, cases[2])
    calls, double.ops.calls = double.ops.calls, None
    names = set(calls)
    assert {"qk_norm_rope_fwd", "qk_norm_rope_append", "gemm_skinny"} <= names and not names & {"gemm_qkv_rope", "gemm_skinny_qkv_rope"}
    # ... one append per layer, chunk and position, right behind the chunk's plain projection (the double's gemm_skinny is a gemm)
    assert all(calls[i - 2:i] == ["gemm_skinny", "gemm"] for i, n in enumerate(calls) if n == "qk_norm_rope_append")


def test_forward_without_backward_keeps_no_projection(step):
    """eval forward / decode prefill: the head norm runs in place on qkv (out == pre, rstd None) -- no per-layer copy of the plain
    projection, no rstd -- and gives the bits of the training forward"""
    geo, sd, batch, _ = step
    a, b = TasuModel(geo, Qwen3FakeOps(), "cpu"), TasuModel(geo, Qwen3FakeOps(), "cpu")
    outs = []
    for m, back in ((a, True), (b, False)):
        m.load_reference_state_dict(sd)
        st = m.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], None, None)
        m.forward_projector_text(st)
        m.forward_llm(st, need_backward=back)
        outs.append((st, m.logits_view(st).clone()))
    assert "qkv_pre" in a._ws and "qk_rstd" in a._ws and "qkv_pre" in outs[0][0].dev
    assert "qkv_pre" not in b._ws and "qk_rstd" not in b._ws and "qkv_pre" not in outs[1][0].dev
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0].dev["qkv"], outs[1][0].dev["qkv"])


def test_core_refuses_what_the_plugin_refuses():
    """a TasuModel built directly on a qk_norm geometry: fp32 copies, adapters and full fine-tuning raise instead of running the
    Qwen2 launches without the head norm"""
    from ps_slm_amd.lora import LoraConfig
    g3 = R.mid_qwen3_geometry()
    m = TasuModel(g3, Qwen3FakeOps(), "cpu")
    m.load_reference_state_dict(qwen3_state_dict(g3, 3))
    with pytest.raises(NotImplementedError, match="qk_norm"):
        m.enable_lora(LoraConfig.from_peft_config(dict(r=8, lora_alpha=16, lora_dropout=0.0)))
    with pytest.raises(NotImplementedError, match="qk_norm"):
        m.enable_llm_training()
    f = TasuModel(g3, Qwen3FakeOps(), "cpu")
    f.llm.keep_f32 = True
    with pytest.raises(NotImplementedError, match="qk_norm"):
        f.load_reference_state_dict(qwen3_state_dict(g3, 3))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("flags,exc,word", [(dict(use_fp16=False), NotImplementedError, "use_fp16"),
                                            (dict(use_peft=True, peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0)), NotImplementedError, "use_peft"),
                                            (dict(freeze_llm=False), NotImplementedError, "freeze_llm")])
def test_unserved_qwen3_recipes_are_refused_before_any_device_work(flags, exc, word):
    class NoOps:
        """any operator call is device work"""
        def __getattr__(self, name):
            raise AssertionError(f"operator {name} was called before the refusal")

    with pytest.raises(exc, match=word):
        factory(ops=NoOps(), **flags)


def write_config(tmp_path, **over):
    c = dict(model_type="qwen3", vocab_size=151936, hidden_size=2048, intermediate_size=6144, num_hidden_layers=28, num_attention_heads=16,
             num_key_value_heads=8, head_dim=128, rope_theta=1000000, rms_norm_eps=1e-6, tie_word_embeddings=True, attention_bias=False)
    c.update(over)
    (tmp_path / "config.json").write_text(json.dumps(c))
    return ModelConfig(llm_path=str(tmp_path), encoder_projector="linear-silu", llm_dim=c["hidden_size"])


def test_config_json_selects_the_decoder_family(tmp_path):
    geo = geometry_from_config(write_config(tmp_path))
    want = geometry_from_config(ModelConfig(llm_path="synthetic:qwen3-1.7b", encoder_projector="linear-silu", llm_dim=2048))
    assert geo.qk_norm and not geo.qkv_bias and dataclasses.asdict(geo) == dataclasses.asdict(want)
    assert (geo.llm_dim, geo.llm_layers, geo.llm_heads, geo.llm_kv_heads, geo.llm_inter, geo.llm_vocab, geo.tied, geo.rope_theta, geo.rms_eps) == \
        (2048, 28, 16, 8, 6144, 151936, True, 1e6, 1e-6)
    mc2 = write_config(tmp_path, model_type="qwen2", hidden_size=1536, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                       attention_bias=True)
    mc2.encoder_dim = 25055
    q2 = geometry_from_config(mc2)
    assert not q2.qk_norm and q2.qkv_bias and dataclasses.asdict(q2) == dataclasses.asdict(Geometry.qwen25_1p5b())
    # a Qwen2 config loads as it did: its use_sliding_window flag and an absent model_type / attention_bias are not looked at
    mc2 = write_config(tmp_path, model_type="qwen2", hidden_size=1536, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960,
                       use_sliding_window=True)
    mc2.encoder_dim = 25055
    assert dataclasses.asdict(geometry_from_config(mc2)) == dataclasses.asdict(q2)
    mid = geometry_from_config(ModelConfig(llm_path="synthetic:mid-qwen3", encoder_projector="linear-silu", llm_dim=256))
    assert dataclasses.asdict(mid) == dataclasses.asdict(R.mid_qwen3_geometry())


@pytest.mark.parametrize("over,exc,word", [(dict(model_type="qwen3_moe"), NotImplementedError, "qwen3_moe"),
                                           (dict(use_sliding_window=True), NotImplementedError, "sliding"),
                                           (dict(hidden_size=1024), ValueError, "hidden"),                  # Qwen3-0.6B: 16 heads x 128 != 1024
                                           (dict(hidden_size=2560, num_attention_heads=32), ValueError, "hidden"),     # Qwen3-4B
                                           (dict(head_dim=64), ValueError, "head_dim")])
def test_unserved_configs_are_refused(tmp_path, over, exc, word):
    mc = write_config(tmp_path, **over)
    with pytest.raises(exc, match=word):
        geometry_from_config(mc)
    with pytest.raises(exc, match=word):                         # ... and by the plugin, before any weight is read (there are none here)
        model_factory(TrainConfig(**SERVED), mc, device="cpu", ops=Qwen3FakeOps())


# ------------------------------------------------------------------------------------------------ weights
def test_state_dict_round_trip_with_and_without_bias_keys():
    """load_reference_state_dict takes a Qwen3 dict (q_norm / k_norm, no bias) and a Qwen2 one (bias, no norm); each geometry
    refuses the other's dict with the missing key's name"""
    g3, g2 = R.mid_qwen3_geometry(), Geometry.from_dict(MID_GEOMETRY)
    sd3, sd2 = qwen3_state_dict(g3, 7), random_state_dict(g2, 7, with_encoder=False)
    assert not any(k.endswith("_proj.bias") for k in sd3) and sum(k.endswith("_norm.weight") for k in sd3) == 2 * g3.llm_layers
    m3 = TasuModel(g3, Qwen3FakeOps(), "cpu")
    m3.load_reference_state_dict(sd3)
    for l, w in enumerate(m3.llm.layers):
        p = f"llm.model.layers.{l}.self_attn."
        assert torch.equal(w["q_norm"], sd3[p + "q_norm.weight"]) and torch.equal(w["k_norm"], sd3[p + "k_norm.weight"])
        assert w["q_norm"].dtype == torch.float32 and not torch.equal(w["q_norm"], w["k_norm"]) and float(w["bqkv"].abs().max()) == 0
        want = torch.cat([sd3[p + f"{m}_proj.weight"] for m in "qkv"]).to(torch.bfloat16)
        assert torch.equal(w["wqkv"], want)
    m2 = TasuModel(g2, Qwen3FakeOps(), "cpu")
    m2.load_reference_state_dict(sd2)
    assert all("q_norm" not in w and float(w["bqkv"].abs().max()) > 0 for w in m2.llm.layers)
    with pytest.raises(KeyError, match="q_norm"):
        TasuModel(g3, Qwen3FakeOps(), "cpu").load_reference_state_dict(sd2)
    with pytest.raises(KeyError, match="bias"):
        TasuModel(g2, Qwen3FakeOps(), "cpu").load_reference_state_dict(sd3)


def test_hf_shards_of_a_qwen3_checkpoint_load(tmp_path):
    """load_hf_llm_state_dict + load_reference_state_dict on a safetensors shard with HF's Qwen3 key names"""
    st = pytest.importorskip("safetensors.torch")
    from ps_slm_amd.ps_slm import load_hf_llm_state_dict
    g3 = R.mid_qwen3_geometry()
    sd = {k: v for k, v in qwen3_state_dict(g3, 9).items() if k.startswith("llm.")}
    st.save_file({k[len("llm."):]: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    back = load_hf_llm_state_dict(str(tmp_path))
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    llm = TasuModel(g3, Qwen3FakeOps(), "cpu").llm
    llm.load_reference_state_dict(back)
    assert torch.equal(llm.layers[1]["k_norm"], sd["llm.model.layers.1.self_attn.k_norm.weight"])


def test_qwen2_synthetic_weights_are_unchanged():
    """random_state_dict / decode_fixture_state_dict must return bit-identical tensors for Qwen2 geometries: every existing token
    fixture regenerates its weights from a seed, so the existing golden tests (tests/test_oracle_golden.py, the generate fixtures)
    enforce this implicitly.  Stated here directly: Qwen3's extra draws come from a generator of their own, so the shared tensors
    of qwen3_state_dict ARE random_state_dict's, and the Qwen2 dict has no new key."""
    g2, g3 = Geometry.from_dict(MID_GEOMETRY), R.mid_qwen3_geometry()
    sd2, sd3 = random_state_dict(g2, 11, with_encoder=False), qwen3_state_dict(g3, 11)
    assert not any("_norm.weight" in k and "self_attn" in k for k in sd2)
    shared = set(sd2) & set(sd3)
    assert len(shared) == len(sd2) - 3 * g2.llm_layers and all(torch.equal(sd2[k], sd3[k]) for k in shared)
    assert list(sd2) == list(random_state_dict(g3, 11, with_encoder=False))       # the new Geometry fields do not reach the draws


def test_qwen2_init_random_is_unchanged():
    """LLMWeights.init_random at a Qwen2 geometry (the benchmark's and the full-size tests' weights): every tensor's bytes equal
    the digests recorded before the bias / head-norm draws became optional in its argument list"""
    from ps_slm_amd.model import LLMWeights
    want = stored_qwen2()["init_random"]
    w = LLMWeights(Geometry.from_dict(MID_GEOMETRY), torch.device("cpu"))
    w.init_random(1234)
    got = {f"{l}.{k}": digest(v) for l, lw in enumerate(w.layers) for k, v in sorted(lw.items()) if k in ("wqkv", "bqkv", "wo", "wgu", "wd", "wqkv_t")}
    got.update(embed=digest(w.embed), head=digest(w.head))
    assert got == want
    w3 = LLMWeights(R.mid_qwen3_geometry(), torch.device("cpu"))
    w3.init_random(1234)
    assert all("q_norm" in lw and not torch.equal(lw["q_norm"], lw["k_norm"]) and float(lw["bqkv"].abs().max()) == 0 for lw in w3.layers)
