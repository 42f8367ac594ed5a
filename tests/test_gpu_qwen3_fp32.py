"""Qwen3 decoders with train_config.use_fp16=false on the GPU: the fp32 path (decode_fp32.py, train_fp32.py) with the per-head q/k
RMSNorm of csrc/qk_norm.hip / csrc/fp32.hip, through model_factory.

At ``synthetic:mid-qwen3``: the eval forward and the training step against the REAL reference's fp32 fixture
(tests/golden/mid_qwen3_step.npz), text and audio batch, at the fp32 bars of tests/test_gpu_fp32_geometry.py -- |loss - ref| <= 2e-5
relative, logits at the stored columns within 2e-5 of the logit scale, every projector gradient within 2e-4 relative L2, the same
accuracy; q_norm and k_norm exchanged in the state dict miss the loss bar by more than 100x.  generate(): all 24 cases of
tests/golden/mid_qwen3_generate.npz token for token against the reference (the fp32 restatement keeps them under +-2e-5 logit
noise: tests/test_qwen3_fp32_cpu.py), decode graphs on and off; the penalty and the sampled case at the fp32 restatement's tokens,
computed here.  The training step is bit-identical run to run (the fp32 step is launched eagerly: there is no replay to compare).
A Qwen2 model on the same path calls none of the three new operators.

At ``synthetic:qwen3-1.7b``, once: each returned hypothesis' beam score equals the log-softmax sum of a plain fp32 forward over
prompt + tokens (the fused finisher on the streaming q|k|v route at K = 2048, the prefill and the append tied together).

Measured on MI355X (8 tests, 2 s for the file; the QWEN3-FP32 lines): eval loss 10.4090214 / 10.4090214 (text), 10.3327131 / 10.3327141
(audio), logits 2.2e-6 / 2.4e-6 of the logit scale, gradients 2.9e-6 / 2.6e-6 relative L2; exchanged norms 96.6 x (text) and 601 x
(audio) the loss bar; 24 of 24 decode cases token-exact; decode scores against the full forward 7.6e-6 nats over 6 tokens."""
import math

import numpy as np
import pytest
import torch

import qwen3_f32_ref as F
import qwen3_ref as R
from penalty_ref import same
from ps_slm_amd.config import ModelConfig, TrainConfig
from ps_slm_amd.synthetic import synthetic_text_batch

pytestmark = pytest.mark.gpu
LOSS_BAR, LOGIT_BAR, GRAD_BAR = 2e-5, 2e-5, 2e-4              # tests/test_gpu_fp32_geometry.py


def factory(llm_path, llm_dim, **kw):
    from ps_slm_amd.ps_slm import model_factory
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=False)
    mc = ModelConfig(llm_path=llm_path, encoder_projector="linear-silu", llm_dim=llm_dim, **({"encoder_dim": 25055} if llm_dim != 256 else {}))
    core = model_factory(tc, mc, init_seed=1234, **kw)[0].core
    assert core.arith == "fp32" and core.arith_train == "fp32" and core.device.type == "cuda"
    return core


@pytest.fixture(scope="module")
def mid():
    gm = factory("synthetic:mid-qwen3", 256, with_encoder=True)
    assert gm.geo.qk_norm and all("q_norm" in f and "k_norm" in f for f in gm.llm.f32["layers"])
    return gm.geo, gm


@pytest.fixture(scope="module")
def step():
    return R.step_case()


def prepare(gm, batch, audio):
    if audio:
        return gm.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"],
                                batch["input_feature_length"], fp32=True)
    return gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], None, None)


def eval_fp32(gm, batch, audio):
    from ps_slm_amd.decode_fp32 import forward_fp32
    st = prepare(gm, batch, audio)
    forward_fp32(gm, st)
    torch.cuda.synchronize()
    return st


def train_fp32(gm, batch, audio):
    from ps_slm_amd.train_fp32 import forward_train_fp32
    st = prepare(gm, batch, audio)
    forward_train_fp32(gm, st)
    gm.run_backward(st)
    torch.cuda.synchronize()
    return st


def loss_error(st, z, tag):
    """|loss - ref| in units of the bar"""
    ref = float(z[f"{tag}_loss"])
    return abs(float(st.dev["loss_out"][0]) - ref) / (LOSS_BAR * abs(ref))


@pytest.mark.parametrize("tag", ["text", "audio"])
def test_eval_forward_and_training_step_against_the_reference(mid, step, tag):
    geo, gm = mid
    _, sd, batch, z = step
    gm.load_reference_state_dict(sd)
    st = eval_fp32(gm, batch, tag == "audio")
    valid = torch.from_numpy(st.plan.key_mask[:, :st.S].astype(bool))
    lg = gm.logits_view(st).cpu()
    assert lg.dtype == torch.float32
    got, ref = lg[:, :, torch.from_numpy(z["cols"])], torch.from_numpy(z[f"{tag}_logits_cols"])
    logit = float((got - ref)[valid].abs().max() / ref[valid].abs().max())
    print(f"QWEN3-FP32 eval {tag}: loss {float(st.dev['loss_out'][0]):.7f} ref {float(z[tag + '_loss']):.7f} ({loss_error(st, z, tag):.3f} of the bar); "
          f"logits {logit:.3g} of the logit scale")
    assert loss_error(st, z, tag) <= 1.0
    assert logit <= LOGIT_BAR
    assert abs(float(st.dev["loss_out"][1]) - float(z[f"{tag}_acc"])) < 1e-6
    st = train_fp32(gm, batch, tag == "audio")
    errs = {k: R.rel_l2(g.cpu(), torch.from_numpy(z[f"{tag}_grad." + k[len("encoder_projector."):]])) for k, g in gm.projector_grads().items()}
    print(f"QWEN3-FP32 step {tag}: loss {float(st.dev['loss_out'][0]):.7f} ({loss_error(st, z, tag):.3f} of the bar); gradients rel L2 "
          f"{max(errs.values()):.3g}")
    assert loss_error(st, z, tag) <= 1.0 and abs(float(st.dev["loss_out"][1]) - float(z[f"{tag}_acc"])) < 1e-6
    assert len(errs) >= 4 and all(v <= GRAD_BAR for v in errs.values()), errs


def test_exchanged_head_norms_miss_the_loss_bar(mid, step):
    """q_norm and k_norm exchanged in the state dict: the fixture sees it.  Asked of the AUDIO batch at more than 100 x the loss
    bar: the reference's own arithmetic (tests/qwen3_ref.py in fp32, variant "swapped", on the CPU) puts the exchanged model
    601 x the bar from the fixture there and 96.6 x on the text batch -- on the text batch no correct implementation can miss by
    more than 100 x.  On BOTH batches the exchanged model's loss is held to that restatement's within the loss bar, so the
    text batch's 96.6 x is asserted as well, as what it is.  Measured on MI355X: 96.6 x (text), 601 x (audio)."""
    import dataclasses
    geo, gm = mid
    _, sd, batch, z = step
    swapped = dict(sd)
    for l in range(geo.llm_layers):
        p = f"llm.model.layers.{l}.self_attn."
        swapped[p + "q_norm.weight"], swapped[p + "k_norm.weight"] = sd[p + "k_norm.weight"], sd[p + "q_norm.weight"]
    gm.load_reference_state_dict(swapped)
    try:                                                         # (the loss buffer is the model's: read before the next forward)
        got = {tag: float(eval_fp32(gm, batch, tag == "audio").dev["loss_out"][0]) for tag in ("text", "audio")}
    finally:
        gm.load_reference_state_dict(sd)
    gd = dataclasses.asdict(geo)
    with torch.no_grad():
        want = {"text": float(R.forward_text(sd, batch, gd, "fp32", variant="swapped")["loss"]),
                "audio": float(R.forward_audio(sd, batch, gd, "fp32", variant="swapped")["loss"])}
    miss = {tag: abs(got[tag] - float(z[f"{tag}_loss"])) / (LOSS_BAR * abs(float(z[f"{tag}_loss"]))) for tag in got}
    for tag in got:
        print(f"QWEN3-FP32 q_norm / k_norm exchanged, {tag}: {miss[tag]:.3g} x the loss bar (loss {got[tag]:.7f}, restatement {want[tag]:.7f})")
        assert abs(got[tag] - want[tag]) <= LOSS_BAR * abs(want[tag]), tag
    assert miss["audio"] > 100.0


def test_training_step_is_bit_identical_run_to_run(mid, step):
    geo, gm = mid
    _, sd, batch, z = step
    gm.load_reference_state_dict(sd)
    runs = []
    for _ in range(3):
        st = train_fp32(gm, batch, False)
        runs.append((st.dev["loss_out"].clone(), gm.proj.g.clone()))
    assert math.isfinite(float(runs[0][0][0])) and float(runs[0][1].abs().max()) > 0
    for l, g in runs[1:]:
        assert torch.equal(l, runs[0][0]) and torch.equal(g, runs[0][1])


@pytest.fixture(scope="module")
def decode(mid):
    geo, gm = mid
    _, sd, cases = R.generate_cases()
    return geo, sd, cases, gm


def test_generate_all_cases_token_for_token(decode):
    geo, sd, cases, gm = decode
    gm.load_reference_state_dict(sd)
    assert gm.decode_graphs and len(cases) == 24
    bad, differ = [], []
    for n, c in enumerate(cases):
        t, e = F.decode_case_fp32(gm, geo, c, graphs=True), F.decode_case_fp32(gm, geo, c, graphs=False)
        if not same(t, c["tokens"]):
            bad.append((n, c["kw"], t.tolist(), c["tokens"].tolist()))
        if not same(t, e):
            differ.append((n, c["kw"]))
    print(f"QWEN3-FP32 generate: {len(cases) - len(bad)} of {len(cases)} cases token-exact")
    assert not bad, bad
    assert not differ, differ


def test_generate_penalty_and_sampled_case(decode):
    geo, sd, cases, gm = decode
    gm.load_reference_state_dict(sd)
    pen, smp, stable = F.knob_cases_fp32(sd, geo, cases)
    assert stable
    for c in (pen, smp):
        t, e = F.decode_case_fp32(gm, geo, c, graphs=True), F.decode_case_fp32(gm, geo, c, graphs=False)
        assert same(t, c["tokens"]), (t.tolist(), c["tokens"].tolist())
        assert same(t, e)


def test_qwen2_on_the_fp32_path_calls_none_of_the_new_operators(monkeypatch):
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    from ps_slm_amd.model import F32_QK_NORM_OPS
    from ps_slm_amd.ops import HipOps
    count = {n: 0 for n in F32_QK_NORM_OPS}
    for n in F32_QK_NORM_OPS:
        def counted(self, *a, _n=n, _f=getattr(HipOps, n), **k):
            count[_n] += 1
            return _f(self, *a, **k)
        monkeypatch.setattr(HipOps, n, counted)
    gm = factory("synthetic:mid", 256, with_encoder=False)
    assert not gm.geo.qk_norm
    batch = synthetic_text_batch(gm.geo, 3, seed=31, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=False, ragged=True)
    st = train_fp32(gm, batch, False)
    assert math.isfinite(float(st.dev["loss_out"][0]))
    ids = batch["input_ids"][:, :9]
    st = gm.prepare_text(ids, torch.ones_like(ids, dtype=torch.bool), None, batch["post_ids"], None, None)
    out = beam_search_generate_fp32(gm, st, num_beams=4, max_new_tokens=5, eos_token_id=-1, pad_token_id=0)
    assert tuple(out.shape) == (3, 5)
    assert count == {n: 0 for n in F32_QK_NORM_OPS}


# ------------------------------------------------------------------------------------------------ synthetic:qwen3-1.7b
def test_full_size_decode_scores_equal_full_forward():
    """2 utterances x 4 beams, 6 new tokens at Qwen3-1.7B in fp32: the beam score of each returned hypothesis against the
    log-softmax sum of a plain fp32 forward over prompt + tokens.  The fp32 suites hold no such comparison for Qwen2.5-1.5B, so the
    tolerance is derived: the fp32 path's logits agree with another fp32 evaluation within LOGIT_BAR = 2e-5 of the logit scale
    per token; a token's log-probability moves by at most twice its logits' error; 10 x the per-token bar x the token count,
    10 * 2e-5 * max |logit| * 6.  Measured on MI355X: 7.63e-6 nats against a bar of 5.41e-3 (logit scale 4.505)."""
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32, forward_fp32
    torch.cuda.empty_cache()
    m = factory("synthetic:qwen3-1.7b", 2048, keep_logits=True)
    geo = m.geo
    assert (geo.llm_dim, geo.llm_layers, geo.llm_heads, geo.llm_kv_heads, geo.llm_inter) == (2048, 28, 16, 8, 6144)
    B, nb, n_new, prompt = 2, 4, 6, 25
    batch = synthetic_text_batch(geo, B, seed=321, prompt_len=prompt, n_audio=104, speech_pos=4, noise=False)
    ids = batch["input_ids"][:, :prompt]
    st = m.prepare_text(ids, torch.ones_like(ids, dtype=torch.bool), None, batch["post_ids"], None, None)
    out = beam_search_generate_fp32(m, st, num_beams=nb, max_new_tokens=n_new, eos_token_id=-1, pad_token_id=0)
    assert tuple(out.shape) == (B, n_new)
    beam_score = m._last_beam.fin_scores[:, 0].float().cpu() * n_new          # length_penalty 1.0: score = sum / length
    S = st.S
    ids2 = torch.cat([ids, out.to(ids.dtype)], dim=1)
    st2 = m.prepare_text(ids2, torch.ones_like(ids2, dtype=torch.bool), None, batch["post_ids"], None, None)
    forward_fp32(m, st2, compute_loss=False)
    torch.cuda.synchronize()
    assert st2.S == S + n_new
    lg = m.logits_view(st2)[:, S - 1:S - 1 + n_new].float()
    tok_lp = torch.log_softmax(lg, dim=-1).gather(2, out.cuda().long()[:, :, None])[:, :, 0].cpu()
    worst, tol = float((tok_lp.sum(1) - beam_score).abs().max()), 10 * LOGIT_BAR * float(lg.abs().max()) * n_new
    print(f"QWEN3-FP32 decode scores vs full forward (B={B}, nb={nb}, D={geo.llm_dim}): worst {worst:.3g} nats of {tol:.3g} "
          f"(logit scale {float(lg.abs().max()):.3f})")
    assert float(tok_lp.min()) > -math.log(geo.llm_vocab) + 1.0             # the beams' tokens stand out of the uniform floor
    assert worst <= tol, (tok_lp.sum(1), beam_score)
    assert np.isfinite(out.numpy()).all()
