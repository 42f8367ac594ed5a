"""Full fine-tuning of a Qwen3 decoder (train_config.freeze_llm=false on synthetic:mid-qwen3) on the HIP kernels: the bf16 step, tied
and untied, against the real reference's fixtures (tools/make_golden_qwen3_full_ft.py) at the bars of tests/test_gpu_full_ft.py and
against the CPU double; the fp32 step at the bars of tests/test_gpu_f32_full_ft.py (loss 2e-5, gradients 2e-4 relative L2 plus the
fixtures' fp16 storage error); eager against graph replay, bit for bit; two engine steps, then generate() and a frozen model loaded
from the checkpoint; save_state / load_state resuming to the uninterrupted run's bits; and the frozen Qwen3 step, which issues
exactly the operator calls it issued before -- no weight-gradient launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDENS = ("mid_qwen3_full_ft", "mid_qwen3_full_ft_untied")


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def double_runs():
    """The CPU double's step on both golden cases, computed once."""
    from full_ft_ops import llm_grads
    from qwen3_full_ft_ops import Qwen3FullFtFakeOps, build_ft, golden_case
    from test_lora_cpu import run_text
    out = {}
    for name in GOLDENS:
        z, geo, sd, batch = golden_case(name)
        cm = build_ft(geo, sd, Qwen3FullFtFakeOps(), "cpu")
        sc = run_text(cm, batch)
        out[name] = (float(sc.dev["loss_out"][0]), llm_grads(cm), cm.projector_grads())
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_bf16_step_vs_reference_golden_and_double(ops, double_runs, name):
    from full_ft_ops import llm_grads
    from qwen3_full_ft_ops import build_ft, check_step_against_golden, golden_case
    from test_lora_cpu import cosine, run_text
    z, geo, sd, batch = golden_case(name)
    gm = build_ft(geo, sd, ops, "cuda")
    sg = run_text(gm, batch)
    torch.cuda.synchronize()
    check_step_against_golden(gm, sg, z, show=f"{name} (HIP)")
    loss_c, lg_c, pg_c = double_runs[name]
    assert abs(float(sg.dev["loss_out"][0]) - loss_c) < 2e-3
    mine = llm_grads(gm)
    worst = (2.0, 0.0, None)
    for k, g2 in lg_c.items():
        g1 = mine[k].cpu()
        c, rel = cosine(g1, g2), float((g1 - g2).norm() / g2.norm())
        worst = min(worst, (c, rel, k))
        assert c > 0.9995 and rel < 3e-2, (k, c, rel)
    print(f"{name}: HIP vs double: lowest cosine {worst[0]:.6f} (relative error {worst[1]:.2e}) at {worst[2]}")
    for k, g2 in pg_c.items():
        assert cosine(gm.projector_grads()[k], g2) > 0.9995, k


@pytest.mark.parametrize("name", GOLDENS)
def test_fp32_step_equals_the_reference(ops, name):
    from full_ft_ops import llm_grads, stored
    from qwen3_full_ft_ops import build_ft, golden_case, n_llm_tensors
    from test_gpu_fp32_train_recipes import check_golden_grads, fp16_storage_error, step_fp32
    z, geo, sd, batch = golden_case(name)
    gm = build_ft(geo, sd, ops, "cuda", fp32=True)
    ft = gm.full_ft
    # the forward reads the masters themselves: the head norms of the fp32 layer set are the bucket's
    f = gm.llm.f32["layers"][1]
    assert f["q_norm"].data_ptr() == ft.view(gm.proj.p, "q_norm", 1).data_ptr() and f["k_norm"].data_ptr() == ft.view(gm.proj.p, "k_norm", 1).data_ptr()
    assert f["wqkv"].data_ptr() == ft.view(gm.proj.p, "wqkv", 1).data_ptr()
    st = step_fp32(gm, batch)
    assert st.fp32
    res = st.dev["loss_out"].cpu()
    print(f"{name}: loss {float(res[0]):.7f} reference {float(z['loss']):.7f}")
    assert abs(float(res[0]) - float(z["loss"])) <= 2e-5
    assert abs(float(res[1]) - float(z["acc"])) < 1e-6
    assert check_golden_grads(gm, z) == 5
    gs = llm_grads(gm)
    want = sorted(k[len("g."):] for k in z if k.startswith("g."))
    assert sorted(gs) == want and len(want) == n_llm_tensors(geo)
    worst = (0.0, None)
    for k, g in gs.items():
        sub, ref = stored(g, z, k)
        bar = 2e-4 + fp16_storage_error(z["g." + k])
        err = float((sub.double() - ref.double()).norm() / ref.double().norm())
        rn = float(g.double().norm()) / float(z["gnorm." + k])
        if "_norm.weight" in k and "self_attn" in k:
            print(f"  {k}: relative L2 {err:.3e} (bar {bar:.3e}), norm ratio - 1 = {rn - 1.0:+.2e}")
        worst = max(worst, (err / bar, k))
        assert err < bar and abs(rn - 1.0) < 2e-4, (k, err, bar, rn)
    print(f"{name}: worst error / bar {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("name", GOLDENS)
def test_graph_replay_equals_eager_on_another_batch(ops, name):
    """Eager launches against hipGraph replay on a DIFFERENT batch of the same shape (first call eager, second captured, third
    replayed) on the bf16 step (the fp32 step is launched eagerly): the loss and the whole gradient bucket, bit for bit -- the head
    norms' ranges not zero."""
    from ps_slm_amd.synthetic import synthetic_text_batch
    from qwen3_full_ft_ops import build_ft, golden_case
    z, geo, sd, _ = golden_case(name)
    gm = build_ft(geo, sd, ops, "cuda")
    gm.keep_logits = False
    mk = lambda seed: synthetic_text_batch(geo, 3, seed=seed, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=False)  # noqa: E731
    b1, b2 = mk(41), mk(42)

    def step(batch, graphs):
        gm.use_graphs = graphs
        st = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"])
        gm.run_forward_text(st)
        gm.run_backward(st)
        torch.cuda.synchronize()
        gm.use_graphs = False
        return st, st.dev["loss_out"].clone(), gm.proj.g.clone()

    _, loss_e, g_e = step(b2, False)
    step(b1, True), step(b1, True)
    st2, loss_g, g_g = step(b2, True)
    assert gm._shape_key(st2, "bwd") in gm._graphs
    assert torch.equal(loss_e, loss_g) and torch.equal(g_e, g_g)
    for l in range(geo.llm_layers):
        for n in ("q_norm", "k_norm"):
            assert float(gm.full_ft.view(g_g, n, l).abs().min()) > 0


def _factory(freeze_llm=False, fp16=True, seed=77, lr=2e-2, ops=None):
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    tc = TrainConfig(freeze_llm=freeze_llm, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=fp16)
    mc = ModelConfig(llm_path="synthetic:mid-qwen3", encoder_projector="linear-silu", llm_dim=256)
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=seed, **({} if ops is None else dict(ops=ops)))
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg["lr"] = lr                                                      # 2e-2: two steps have to move the argmax of some position
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10
    return model, eng


@pytest.mark.parametrize("fp16", [True, False], ids=["bf16", "fp32"])
def test_two_engine_steps_then_decode_and_a_frozen_model_from_the_checkpoint(fp16):
    """generate() after two engine steps differs from the frozen model's (the same init seed) and equals, token for token,
    generate() of a fresh FROZEN model loaded from the stepped model's state_dict(); every tensor moved, the head norms among them"""
    from ps_slm_amd.synthetic import synthetic_text_batch
    from qwen3_full_ft_ops import n_llm_tensors
    from test_lora_cpu import to_call
    model, eng = _factory(fp16=fp16)
    core = model.core
    assert core.full_ft is not None and core.arith_train == ("bf16" if fp16 else "fp32")
    raws = [synthetic_text_batch(core.geo, 2, seed=s, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False) for s in (5, 6)]
    ids = raws[0]["input_ids"][:, :10]
    am = torch.ones_like(ids, dtype=torch.bool)
    targets = ["ab cde f ghij kl m", "no pq rst uvw"]
    gen = lambda m: m.generate(input_ids=ids, attention_mask=am, targets=targets, num_beams=4, max_new_tokens=12).cpu().numpy()  # noqa: E731
    frozen, _ = _factory(freeze_llm=True, fp16=fp16)
    t0 = gen(frozen.eval())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    for raw in raws:
        out, _ = eng(**to_call(raw))
        eng.backward(out.loss)
        eng.step()
    torch.cuda.synchronize()
    after = model.state_dict()
    assert len(after) == 6 + n_llm_tensors(core.geo) and not any(k.endswith(".bias") for k in after if k.startswith("llm."))
    for k, v in after.items():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, before[k]), k
    t1 = gen(model.eval())
    ckpt = {k: v.cpu() for k, v in after.items()}
    missing, unexpected = frozen.load_state_dict(ckpt)
    assert not missing and not unexpected and frozen.core.full_ft is None
    t2 = gen(frozen.eval())
    torch.cuda.synchronize()
    assert np.array_equal(t1, t2), (t1, t2)
    assert not np.array_equal(t0, t1)


RESUME = {"qwen3_full_ft_bf16": dict(freeze_llm=False, use_fp16=True), "qwen3_full_ft_fp32": dict(freeze_llm=False, use_fp16=False)}


@pytest.mark.parametrize("recipe", list(RESUME))
def test_three_steps_are_deterministic_and_resume_after_the_second(tmp_path, recipe):
    """Two uninterrupted runs of three steps give equal bits in p, m, v (and the bf16 image and the losses); save_state after step 2,
    load_state into a model built from another init_seed, then step 3: the uninterrupted run's bits."""
    import resume_cases as rc
    from test_gpu_f32_full_ft import _resume_make
    a, c, control = rc.resume_pattern(_resume_make(RESUME[recipe], "synthetic:mid-qwen3", True), tmp_path, N=3, k=2, what=recipe)
    assert control == 0.0                                                # the control: A and A' are bit-equal
    want = "fp32" if recipe.endswith("fp32") else "bf16"
    assert a.core.arith_train == want and c.core.arith_train == want and a.core.geo.qk_norm and a.core.full_ft is not None


def _recording_ops():
    from ps_slm_amd.ops import HipOps

    class Recording(HipOps):
        """HipOps with ``calls`` (a list, or None) receiving the name of every operator called"""

        def __init__(self):
            super().__init__()
            self.calls = None

        def __getattribute__(self, name):
            attr = object.__getattribute__(self, name)
            if name.startswith("_") or not callable(attr):
                return attr
            calls = object.__getattribute__(self, "__dict__").get("calls")
            if calls is None:
                return attr

            def recorded(*a, **k):
                calls.append(name)
                return attr(*a, **k)
            return recorded

    return Recording()


def _recorded_step(m, batch):
    st = m.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"])
    m.ops.calls = []
    m.forward_projector_text(st)
    m.forward_llm(st)
    m.backward(st)
    torch.cuda.synchronize()
    calls, m.ops.calls = m.ops.calls, None
    return calls


def test_a_frozen_step_issues_no_weight_gradient_launch():
    """The frozen Qwen3 step on an operator set that HAS the new operators: its decoder backward is the dgrad chain it was -- per
    layer the fused SwiGLU dgrad, two GEMMs, two norm backwards, the attention backward and ONE head-norm backward -- with no
    weight-gradient call anywhere in the decoder; the trainable step reads dqkv right before the head norm's backward."""
    from ps_slm_amd.model import TasuModel
    from qwen3_full_ft_ops import build_ft, golden_case
    z, geo, sd, batch = golden_case(GOLDENS[0])
    L = geo.llm_layers
    ops = _recording_ops()
    fm = TasuModel(geo, ops, "cuda")
    fm.load_reference_state_dict(sd)
    calls = _recorded_step(fm, batch)
    assert not any("wgrad" in n or n in ("gemm_tn", "colsum_split") for n in calls), calls
    layer = ["gemm_dswiglu", "gemm", "rmsnorm_bwd", "gemm", "attn_bwd_fused", "qk_norm_bwd", "gemm", "rmsnorm_bwd"]
    first = calls.index("gemm_dswiglu")
    assert calls[first:first + L * len(layer)] == L * layer, calls[first:]
    assert calls.count("qk_norm_rope_fwd") == L and calls.count("qk_norm_bwd") == L
    tm = build_ft(geo, sd, _recording_ops(), "cuda")
    calls = _recorded_step(tm, batch)
    at = [i for i, n in enumerate(calls) if n == "qk_norm_wgrad"]
    assert len(at) == L and all(calls[i - 1] == "attn_bwd_fused" and calls[i + 1] == "qk_norm_bwd" for i in at), calls
    assert "colsum_split" not in calls and calls.count("rmsnorm_wgrad") == 2 * L + 1
