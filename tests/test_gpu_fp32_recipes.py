"""use_fp16 = false for LoRA models and the alternate projectors: the reference decodes and evaluates them in fp32
(Multitask/inference_batch.py:113-117,146; Multitask/scripts/decode_sensevoice.sh passes use_peft / encoder_projector through).
The fused fp32 cross-attention kernel (csrc/f32_ca.hip) against a float64 restatement of projector.py:111-126, the eval forward of
every served projector and of the adapted decoder at the fp32 bars of the shipped model against the REAL reference's goldens, the
adapted fp32 decode token-exact, adapter updates, and the selection through model_factory."""
import numpy as np
import pytest
import torch


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def f32_model(geo, sd, ops, cfg=None, lsd=None):
    """What model_factory builds for train_config.use_fp16 = false (fp32 copies of the frozen weights, arith = fp32)."""
    from ps_slm_amd.model import TasuModel
    gm = TasuModel(geo, ops, "cuda")
    gm.llm.keep_f32 = True
    gm.arith = "fp32"
    gm.load_reference_state_dict(sd)
    if cfg is not None:
        gm.enable_lora(cfg)
        gm.lora.load_state_dict(lsd)
        gm.sync_projector_copies()
    return gm


# ------------------------------------------------------------------------------------------ 1. the kernel
def ca_double(q, table, H):
    """projector.py:111-126 in float64: q [R, D], table [V, D] -> [R, D]."""
    R, D = q.shape
    d = D // H
    qh, kh = q.double().view(R, H, d), table.double().view(-1, H, d)
    scores = torch.einsum("rhd,vhd->rhv", qh, kh) / d ** 0.5
    return torch.einsum("rhv,vhd->rhd", scores.softmax(-1), kh).reshape(R, D)


@pytest.mark.parametrize("dh", [64, 192, 448])
@pytest.mark.parametrize("V", [1000, 151936])
def test_ca_attn_kernel_vs_double(ops, dh, V):
    H = 8
    D = H * dh
    g = torch.Generator(device="cuda").manual_seed(dh * 7 + V)
    table = torch.randn(V, D, generator=g, device="cuda")
    for R in (1, 37, 300):
        q = torch.randn(R, D, generator=g, device="cuda") * 0.15
        # near-one-hot rows: a query along one key of its head gives that key a score of ~40 against N(0, 40^2 / dh) for the
        # others -- the running max, the rescale and the split merge see a wide dynamic range
        for r in range(0, R, 3):
            v = int(torch.randint(0, V, (1,), generator=g, device="cuda"))
            q[r] = table[v] * (40.0 / dh ** 0.5)
        out = torch.full((R, D), 7.0, device="cuda")
        ops.f32_ca_attn(q, table, out, R, H)
        torch.cuda.synchronize()
        ref = ca_double(q, table, H)
        err = (out.double() - ref).abs().view(R, H, dh).amax(dim=(0, 2))
        scale = ref.abs().view(R, H, dh).amax(dim=(0, 2))
        assert bool((err <= 1e-5 * scale).all()), (dh, V, R, (err / scale).max().item())
        again = torch.empty_like(out)
        ops.f32_ca_attn(q, table, again, R, H)
        torch.cuda.synchronize()
        assert torch.equal(out, again)


def test_ca_attn_rejects_bad_arguments_and_leaves_out_untouched(ops):
    from ps_slm_amd._lib import load
    lib = load()
    V, H, dh, R = 1000, 8, 64, 5
    D = H * dh
    q, table = torch.randn(R, D, device="cuda"), torch.randn(V, D, device="cuda")
    out = torch.full((R, D), 3.0, device="cuda")
    n = lib.tasu_f32_ca_workspace_floats(R, V, D, H)
    assert n > 0 and lib.tasu_f32_ca_workspace_floats(R, V, D + 1, H) == -1
    ws = torch.empty(n, device="cuda")
    good = [q.data_ptr(), D, table.data_ptr(), V, D, H, float(dh) ** 0.5, out.data_ptr(), D, R, ws.data_ptr(), n, None]
    bad = [{0: None}, {2: None}, {7: None}, {10: None},            # null operands
           {1: D - 4}, {8: D - 1}, {1: D + 2},                     # ldq / ldo < D, ldq not a multiple of 4
           {11: n - 1},                                            # workspace too small
           {4: 8 * 20, 1: 160, 8: 160},                            # dh = 20: not a multiple of 16
           {4: 8 * 528, 1: 8 * 528, 8: 8 * 528},                   # dh = 528 > 512
           {5: 7}, {9: 0}, {3: 0}, {6: 0.0}]                       # D % H, R, V, denom
    for over in bad:
        args = list(good)
        for k, v in over.items():
            args[k] = v
        assert lib.tasu_f32_ca_attn(*args) == 1, over
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert lib.tasu_f32_ca_attn(*good) == 0
    torch.cuda.synchronize()
    assert not bool((out == 3.0).any())


# ------------------------------------------------------------------------------------------ 2. eval forward vs the goldens
def check_fp32(gm, st, z):
    """The fp32 bars of test_gpu_model.py::test_eval_forward_in_fp32_equals_the_reference_to_fp32_rounding."""
    res = st.dev["loss_out"].cpu()
    assert abs(float(res[0]) - float(z["loss"])) <= 2e-5 * max(1.0, abs(float(z["loss"]))), (float(res[0]), float(z["loss"]))
    assert abs(float(res[1]) - float(z["acc"])) < 1e-6
    valid = torch.from_numpy(st.plan.key_mask[:, : st.S].astype(bool))
    lg = gm.logits_view(st).cpu()
    assert lg.dtype == torch.float32
    ref = torch.from_numpy(z["logits_cols"])
    assert float((lg[:, :, torch.from_numpy(z["cols"])] - ref)[valid].abs().max() / ref[valid].abs().max()) < 2e-5
    lse = st.dev["row_lse"].cpu().view(st.B, st.S)
    assert float((lse - torch.from_numpy(z["lse"]))[valid].abs().max()) < 2e-5 * float(np.abs(z["lse"]).max())


def _projector_case(name):
    from conftest import ca_projector_case, cov1d_projector_case, linear_projector_case
    if name == "ca":
        return ca_projector_case()
    kind, k = name.split("_k")
    return (linear_projector_case if kind == "linear" else cov1d_projector_case)(int(k))


@pytest.mark.parametrize("name", ["linear_k1", "linear_k2", "cov1d_k1", "cov1d_k2", "ca"])
def test_eval_forward_alternate_projectors_at_fp32_bars(ops, name):
    from ps_slm_amd.decode_fp32 import forward_fp32
    geo, sd, batch, z = _projector_case(name)
    gm = f32_model(geo, sd, ops)
    st = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], batch.get("alphas"),
                         batch.get("keeps"))
    forward_fp32(gm, st)
    torch.cuda.synchronize()
    check_fp32(gm, st, z)


@pytest.mark.parametrize("name", ["mid_text_lora", "mid_text_lora_qv"])
def test_eval_forward_lora_at_fp32_bars(ops, name):
    """Dropout p = 0 in these fixtures: their training-mode goldens are the eval forward."""
    from ps_slm_amd.decode_fp32 import forward_fp32
    from test_lora_cpu import golden_case
    z, geo, cfg, sd, lsd, batch = golden_case(name)
    assert cfg.lora_dropout == 0.0
    gm = f32_model(geo, sd, ops, cfg, lsd)
    st = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"])
    forward_fp32(gm, st)
    torch.cuda.synchronize()
    check_fp32(gm, st, z)


# ------------------------------------------------------------------------------------------ 3. LoRA decode, token-exact
def gen_fp32(gm, ids, am, post_ids, **kw):
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    st = gm.prepare_text(ids, am, None, post_ids, None, None)
    return beam_search_generate_fp32(gm, st, **kw).numpy()


def test_lora_fp32_decode_equals_the_reference_tokens(ops):
    from conftest import decode_lora_margin_cases
    from test_lora_cpu import gen_inputs
    geo, cfg, sd, lsd, cases = decode_lora_margin_cases()
    gm = f32_model(geo, sd, ops, cfg, lsd)
    bad = []
    for n, c in enumerate(cases):
        toks = gen_fp32(gm, c["ids"], c["am"], c["post_ids"], eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **c["kw"])
        if toks.shape != c["tokens"].shape or not np.array_equal(toks, c["tokens"]):
            bad.append((n, toks.tolist(), c["tokens"].tolist()))
    assert not bad, bad
    geo, cfg, sd, lsd, ids, am, word_ids, ref, _ = gen_inputs()
    gm = f32_model(geo, sd, ops, cfg, lsd)
    toks = gen_fp32(gm, ids, am, word_ids, max_new_tokens=16)
    assert np.array_equal(toks, ref), (toks, ref)


# ------------------------------------------------------------------------------------------ 4. adapter updates
def test_adapter_update_rebuilds_the_fp32_weights(ops):
    from conftest import decode_lora_margin_cases
    from ps_slm_amd.synthetic import random_lora_state_dict
    geo, cfg, sd, lsd, cases = decode_lora_margin_cases()
    c = cases[0]
    kw = dict(eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **c["kw"])
    gm = f32_model(geo, sd, ops, cfg, lsd)
    base = [{k: v.clone() for k, v in f.items() if torch.is_tensor(v)} for f in gm.llm.f32["layers"]]
    gen_fp32(gm, c["ids"], c["am"], c["post_ids"], **kw)
    gen_fp32(gm, c["ids"], c["am"], c["post_ids"], **kw)            # a captured decode graph exists now
    lsd2 = random_lora_state_dict(geo, cfg, 977, b_scale=0.05)
    gm.lora.load_state_dict(lsd2)
    gm.sync_projector_copies()
    got = gen_fp32(gm, c["ids"], c["am"], c["post_ids"], **kw)
    fresh = f32_model(geo, sd, ops, cfg, lsd2)
    want = gen_fp32(fresh, c["ids"], c["am"], c["post_ids"], **kw)
    assert np.array_equal(got, want), (got, want)
    for l, f in enumerate(gm.llm.f32["layers"]):
        for k, v in base[l].items():
            assert torch.equal(f[k], v), (l, k)
    m1, m2 = gm.lora._merged32["layers"], fresh.lora._merged32["layers"]
    for a, b in zip(m1, m2):
        for k in ("wqkv", "wo", "wgu", "wd"):
            assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ 5. selection through the plugin
def _factory(projector, use_peft, fp16):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    kw = dict(peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0)) if use_peft else {}
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True,
                     use_fp16=fp16, use_peft=use_peft, **kw)
    extra = dict(encoder_projector_ds_rate=2) if projector in ("linear", "cov1d-linear") else {}
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector=projector, llm_dim=256, **extra)
    model, tok = model_factory(tc, mc, device="cuda:0", init_seed=77)
    return model, tok


@pytest.mark.parametrize("projector,use_peft", [("linear-silu", True), ("linear", False), ("cov1d-linear", False),
                                                ("cross-attention", False)])
def test_use_fp16_false_selects_fp32_eval_and_keeps_the_bf16_training_step(projector, use_peft):
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    from ps_slm_amd.synthetic import random_lora_state_dict, synthetic_text_batch
    model, tok = _factory(projector, use_peft, False)
    core = model.core
    assert core.arith == "fp32" and core.arith_train == "bf16" and core.llm.f32 is not None
    if use_peft:                                                    # non-zero adapters: the decode has to see them
        core.lora.load_state_dict(random_lora_state_dict(core.geo, core.lora.cfg, 5, b_scale=0.05))
        core.sync_projector_copies()
    raw = synthetic_text_batch(core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    ids = raw["input_ids"][:, :10]
    am = torch.ones_like(ids, dtype=torch.bool)
    targets = ["ab cde f ghij kl m", "no pq rst uvw"]
    model.eval()
    toks = model.generate(input_ids=ids, attention_mask=am, targets=targets, num_beams=4, max_new_tokens=12).numpy()
    st = core.prepare_text(ids, am, None, [model.encoder_tokenizer.encode(t) for t in targets], None, None)
    direct = beam_search_generate_fp32(core, st, num_beams=4, max_new_tokens=12, eos_token_id=tok.eos_token_id,
                                       pad_token_id=tok.pad_token_id).numpy()
    assert np.array_equal(toks, direct)
    # the training step is the use_fp16 = true model's, bit for bit
    m16, _ = _factory(projector, use_peft, True)
    assert m16.core.arith == "bf16"
    if use_peft:
        m16.core.lora.load_state_dict(core.lora.state_dict())
        m16.core.sync_projector_copies()
    if projector == "cross-attention":
        # the bf16 cross-attention step needs a head width that is a multiple of 64 (synthetic:mid: 256 / 8 heads = 32): the same
        # selection on the mid512 fixture's geometry (8 heads of 64), wrapped the way model_factory wraps its core
        model, m16, raw = _ca_pair(core), _ca_pair(m16.core), _ca_batch()
    call = dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], labels=raw["labels"], input_features=None,
                input_feature_length=None, GT=[" ".join(map(str, p)) for p in raw["post_ids"]])
    res = []
    for m in (model, m16):
        m.train()
        out, _ = m(**call)
        out.loss.backward()
        torch.cuda.synchronize()
        assert not getattr(m.last_state, "fp32", False)
        if use_peft:                                # the adapters' gradients live in the bucket's tail, behind the projector's
            assert m.core.proj.g.numel() == m.core.lora.base + m.core.lora.numel
        res.append((out.loss.detach().cpu().clone(), m.core.proj.g.detach().cpu().clone(), m.core.lora_grads()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    assert res[0][2].keys() == res[1][2].keys() and all(torch.equal(v.cpu(), res[1][2][k].cpu()) for k, v in res[0][2].items())


def _ca_batch():
    from conftest import ca_projector_case
    return ca_projector_case()[2]


def _ca_pair(selected):
    """A cross-attention model at the mid512 geometry with the arithmetic selection of ``selected`` (a model_factory core)."""
    from conftest import ca_projector_case
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.model import TasuModel
    from ps_slm_amd.ps_slm import SyntheticLLMTokenizer, setup_encoder_tokenizer, slam_model_asr
    geo, sd, _, _ = ca_projector_case()
    core = TasuModel(geo, selected.ops, "cuda")
    core.arith, core.arith_train, core.llm.keep_f32 = selected.arith, selected.arith_train, selected.llm.keep_f32
    core.load_reference_state_dict(sd)
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True,
                     use_fp16=selected.arith != "fp32")
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector="cross-attention")
    return slam_model_asr(core, SyntheticLLMTokenizer(geo), setup_encoder_tokenizer(mc, geo), tc, mc)


# ------------------------------------------------------------------------------------------ 3b. unfiltered cases vs the oracle
def test_lora_fp32_decode_equals_the_double_oracle_on_unfiltered_cases(ops):
    """20 seeded cases, none filtered: the GPU must equal the float64 oracle (W + s B A merged in float64) wherever the oracle's
    fp32 and float64 runs agree, and at least 12 cases must qualify."""
    from conftest import decode_lora_margin_cases
    from fp32_oracle_cases import compare, lora_merged_double
    geo, cfg, sd, lsd, _ = decode_lora_margin_cases()
    gm = f32_model(geo, sd, ops, cfg, lsd)
    n_ok, bad = compare(lambda ids, am, p, kw: gen_fp32(gm, ids, am, p, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw),
                        lora_merged_double(sd, lsd, cfg), geo, range(5100, 5120))
    assert n_ok >= 12, n_ok
    assert not bad, bad


@pytest.mark.parametrize("kind", ["linear", "cov1d-linear", "cross-attention"])
def test_alternate_projector_fp32_decode_equals_the_double_oracle_on_unfiltered_cases(ops, kind):
    """10 seeded cases per projector (k = 2 frames per row for linear / cov1d-linear, 8 heads of 64 for cross-attention), none
    filtered: the GPU equals the float64 oracle on every case where its fp32 and float64 runs agree; at least 8 qualify."""
    from fp32_oracle_cases import compare
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, decode_fixture_state_dict
    extra = dict(llm_dim=512, llm_heads=4, llm_kv_heads=2, llm_inter=1024) if kind == "cross-attention" else \
        dict(projector_ds_rate=2, bottleneck=2048)
    geo = Geometry.from_dict(dict(MID_GEOMETRY, projector=kind, **extra))
    sd = decode_fixture_state_dict(geo, 4242)
    gm = f32_model(geo, sd, ops)
    n_ok, bad = compare(lambda ids, am, p, kw: gen_fp32(gm, ids, am, p, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw),
                        {k: v.double() for k, v in sd.items()}, geo, range(6100, 6110), min_post=4)
    assert n_ok >= 8, n_ok
    assert not bad, bad


# ------------------------------------------------------------------------------------------ audio branch
@pytest.mark.parametrize("kind", ["lora", "cov1d-linear"])
def test_audio_branch_eval_forward_in_fp32_vs_the_double_oracle(ops, kind):
    """The audio branch (fp32 encoder -> CTC softmax -> PSD -> fp32 projector -> decoder) of an adapted model and of a
    k = 2 cov1d-linear projector: the eval-mode loss within 2e-5 and the logits within 2e-5 of their scale of the float64 oracle
    on the mid_audio_psd inputs (PSD decisions stable under rounding), the same PSD lengths."""
    import dataclasses

    from conftest import mid_audio_psd_case
    from fp32_oracle_cases import lora_merged_double
    from oracle import tasu_oracle as O
    from ps_slm_amd.decode_fp32 import forward_fp32
    from ps_slm_amd.lora import LoraConfig
    from ps_slm_amd.synthetic import random_lora_state_dict, random_state_dict
    geo, sd, batch, z = mid_audio_psd_case()
    cfg = lsd = None
    if kind == "lora":
        cfg = LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0)
        lsd = random_lora_state_dict(geo, cfg, 31, b_scale=0.05)
        W = lora_merged_double(sd, lsd, cfg)
    else:
        geo = dataclasses.replace(geo, projector=kind, projector_ds_rate=2, bottleneck=2048)
        sd = {n: v for n, v in sd.items() if not n.startswith("encoder_projector.")}
        sd.update({n: v for n, v in random_state_dict(geo, 91, with_encoder=False).items() if n.startswith("encoder_projector.")})
        W = {k: v.double() for k, v in sd.items()}
    gm = f32_model(geo, sd, ops, cfg, lsd)
    st = gm.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"],
                          batch["input_feature_length"], fp32=True)
    assert np.array_equal(st.dev["psd_lens"], z["psd_lens"])
    assert "y2" not in st.dev                                       # no bf16 projector pass behind the fp32 one
    forward_fp32(gm, st)
    torch.cuda.synchronize()
    b64 = dict(batch, input_features=batch["input_features"].double())
    ref = O.forward_audio(W, b64, dataclasses.asdict(geo), mode="fp32")
    loss = float(st.dev["loss_out"][0])
    assert abs(loss - float(ref["loss"])) <= 2e-5 * max(1.0, abs(float(ref["loss"]))), (loss, float(ref["loss"]))
    valid = torch.from_numpy(st.plan.key_mask[:, : st.S].astype(bool))
    lg, rl = gm.logits_view(st).cpu().double(), ref["logits"].detach()
    assert lg.shape == rl.shape
    assert float((lg - rl)[valid].abs().max() / rl[valid].abs().max()) < 2e-5
