"""Full fine-tuning of the decoder and use_emb on the fp32 training step (train_config.freeze_llm = false / use_emb with
use_fp16 = false), on the GPU: the weight-gradient kernels of csrc/wgrad_f32.hip (tasu_f32_gemm_tn, tasu_f32_rmsnorm_wgrad,
tasu_f32_colsum_split) against float64 with bounds derived from the arithmetic, the step against the REAL reference's fp32
gradients of every Qwen2 tensor at the project's fp32 bars (loss 2e-5, gradients 2e-4 relative L2 + what the fixtures' fp16 storage
may have moved), the audio branch against float64 autograd, the factory / engine / checkpoint plumbing, determinism and resume.
Everything at the mid geometry (256 wide, 2 layers, V = 1000) unless a shape says otherwise."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                                                          # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def _ulp(t):
    """One unit in the last place of every fp32 element of t (float64 tensor out)."""
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# ------------------------------------------------------------------------------------------ 1. tasu_f32_gemm_tn
# (R, N, K, lda, ldb, ldc): one row and one quad; odd sizes inside one tile with a last stage of 15 rows; one row past four stages;
# several tiles, every width ending inside a tile, all three matrices column slices of wider ones; more than one block both ways
# with one row past 16 stages; the down projection of Qwen2.5-1.5B (12 x 70 tiles)
TN_SHAPES = [(1, 4, 4, None, None, None), (63, 60, 68, None, None, None), (65, 64, 64, None, None, None),
             (200, 132, 260, 140, 272, 268), (257, 384, 256, None, None, None), (320, 1536, 8960, None, None, None)]


def _tn_case(R, N, K, lda, ldb):
    """Operands on the GPU with NaN in the three rows behind R and in the columns past the widths; float64 reference and magnitude."""
    g = torch.Generator().manual_seed(R * 7 + N * 3 + K)
    a = torch.full((R + 3, lda), float("nan"))
    b = torch.full((R + 3, ldb), float("nan"))
    a[:R, :N] = torch.randn(R, N, generator=g)
    b[:R, :K] = torch.randn(R, K, generator=g)
    a, b = a.cuda(), b.cuda()
    ad, bd = a[:R, :N].double(), b[:R, :K].double()
    return a, b, ad.t() @ bd, ad.abs().t() @ bd.abs()


@pytest.mark.parametrize("R,N,K,lda,ldb,ldc", TN_SHAPES)
def test_f32_gemm_tn_against_float64(ops, R, N, K, lda, ldb, ldc):
    lda, ldb, ldc = lda or N, ldb or K, ldc or K + 8
    a, b, ref, mag = _tn_case(R, N, K, lda, ldb)
    c0 = torch.randn(N + 3, ldc, generator=torch.Generator().manual_seed(R + N + K)).cuda()   # C sits inside a larger pre-filled buffer
    top = min(16, (R + 15) // 16)                                        # TASU_F32_GEMM_TN_MAX_SPLIT, whole 16-row stages
    policy = ops.f32_gemm_tn_split(R, N, K)
    assert 1 <= policy <= top
    worst = 0.0
    for accumulate in (False, True):
        for nsplit in sorted({1, min(2, top), top, policy}):
            ws = torch.full((nsplit * N * K,), float("nan"), device="cuda") if nsplit > 1 else None
            outs = []
            for _ in range(2):
                c = c0.clone()
                ops.f32_gemm_tn(a, b, c, R, N, K, accumulate=accumulate, nsplit=nsplit, ws=ws)
                torch.cuda.synchronize()
                outs.append(c)
            assert torch.equal(outs[0], outs[1]), (accumulate, nsplit)   # no atomics: the same bits on every run
            got = outs[0][:N, :K].double()
            assert bool(torch.isfinite(got).all()), (accumulate, nsplit)  # the NaN rows behind R never reach C
            want = ref + c0[:N, :K].double() if accumulate else ref
            # one rounding per product and at most R - 1 additions in any order (inside an MFMA, over the stages, over the slabs):
            # the any-order summation bound; one ulp of the initial and of the final value when accumulating
            bound = (R + 2) * EPS * mag + (_ulp(c0[:N, :K]) + _ulp(want) if accumulate else 0)
            err = (got - want).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), (accumulate, nsplit, ratio)
            assert torch.equal(outs[0][N:], c0[N:]) and torch.equal(outs[0][:, K:], c0[:, K:]), (accumulate, nsplit)   # bitwise
            assert not torch.equal(outs[0][:N, :K], c0[:N, :K])
    print(f"f32_gemm_tn ({R}, {N}, {K}): policy split {policy}, worst error / bound {worst:.3f}")


def test_composed_route_meets_the_same_bound(ops):
    """Two tasu_f32_transpose + tasu_f32_gemm_nt (the projector's route) on (257, 384, 256): the same sums in another order."""
    R, N, K = 257, 384, 256
    a, b, ref, mag = _tn_case(R, N, K, N, K)
    Rp = (R + 31) // 32 * 32
    a_t, b_t = torch.full((N, Rp), float("nan"), device="cuda"), torch.full((K, Rp), float("nan"), device="cuda")
    ops.f32_transpose(a, a_t, R, N, Rp)
    ops.f32_transpose(b, b_t, R, K, Rp)
    c_old, c_new = torch.zeros(N, K, device="cuda"), torch.zeros(N, K, device="cuda")
    ops.f32_gemm(a_t, b_t, c_old, N, K, Rp)
    ops.f32_gemm_tn(a, b, c_new, R, N, K)
    torch.cuda.synchronize()
    bound = (R + 2) * EPS * mag
    assert bool(((c_old.double() - ref).abs() <= bound).all()) and bool(((c_new.double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------ 2. tasu_f32_rmsnorm_wgrad, colsum
@pytest.mark.parametrize("R,D", [(1, 256), (77, 512), (1024, 1536), (5, 4), (130, 4), (5, 260), (130, 260)])   # D = 4: one lane of one
@pytest.mark.parametrize("given", [False, True])                                                               # block; 260: a second block, one live lane
def test_f32_rmsnorm_wgrad_against_float64(ops, R, D, given):
    """rstd recomputed from x and eps (what the step does) or passed in; the reference is float64 on the very inputs."""
    from ps_slm_amd.ops import RMS_WGRAD_SPLIT
    g = torch.Generator().manual_seed(R * 13 + D)
    dy, x, eps = torch.randn(R, D, generator=g).cuda(), (torch.randn(R, D, generator=g) * 3).cuda(), 1e-6
    rstd = (torch.rand(R, generator=g) + 0.2).cuda() if given else None
    rs64 = rstd.double() if given else 1.0 / torch.sqrt(x.double().pow(2).mean(1) + eps)
    terms = dy.double() * x.double() * rs64[:, None]
    ref, mag = terms.sum(0), terms.abs().sum(0)
    dw0 = torch.randn(D + 4, generator=g).cuda()
    ws = torch.full((RMS_WGRAD_SPLIT * D + R + 3,), float("nan"), device="cuda")
    for accumulate in (False, True):
        outs = []
        for _ in range(2):
            dw = dw0.clone()
            ops.f32_rmsnorm_wgrad(dy, x, dw[:D], ws, eps, rstd=rstd, accumulate=accumulate)
            torch.cuda.synchronize()
            outs.append(dw)
        assert torch.equal(outs[0], outs[1])
        want = ref + dw0[:D].double() if accumulate else ref
        # three factors per term: two product roundings and rstd's own (the bf16 kernel's term has exact inputs and two), at most
        # R - 1 additions over the two stages
        bound = (R + 4) * EPS * mag + (_ulp(dw0[:D]) + _ulp(want) if accumulate else 0)
        err = (outs[0][:D].double() - want).abs()
        assert bool((err <= bound).all()), (accumulate, float((err / bound.clamp_min(1e-300)).max()))
        assert torch.equal(outs[0][D:], dw0[D:])


@pytest.mark.parametrize("R,C,ld", [(1, 256, 256), (77, 512, 520), (1024, 2048, 2048), (300, 100, 104)])
def test_f32_colsum_split_against_float64(ops, R, C, ld):
    """The q|k|v bias gradient's reduction: R - 1 fp32 additions in any order; columns past C and the rest of `out` untouched."""
    from ps_slm_amd.ops import RMS_WGRAD_SPLIT
    g = torch.Generator().manual_seed(R + C)
    x = torch.randn(R, ld, generator=g).cuda()
    out0 = torch.randn(C + 4, generator=g).cuda()
    ws = torch.full((RMS_WGRAD_SPLIT * C,), float("nan"), device="cuda")
    ref, mag = x[:, :C].double().sum(0), x[:, :C].double().abs().sum(0)
    for accumulate in (False, True):
        outs = []
        for _ in range(2):
            out = out0.clone()
            ops.f32_colsum_split(x, out, ws, R, C, accumulate=accumulate)
            torch.cuda.synchronize()
            outs.append(out)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0][C:], out0[C:])
        want = ref + out0[:C].double() if accumulate else ref
        bound = R * EPS * mag + (_ulp(out0[:C]) + _ulp(want) if accumulate else 0)
        assert bool(((outs[0][:C].double() - want).abs() <= bound).all())


# ------------------------------------------------------------------------------------------ 3. the step against the reference
def build_ft32(geo, sd, ops):
    """What model_factory builds for freeze_llm = false with use_fp16 = false: fp32 everywhere, the decoder in the bucket."""
    from ps_slm_amd.model import TasuModel
    gm = TasuModel(geo, ops, "cuda")
    gm.llm.keep_f32 = True
    gm.arith = gm.arith_train = "fp32"
    gm.load_reference_state_dict(sd)
    gm.enable_llm_training(sd)
    return gm


def rel(g, ref):
    return float((g.double().cpu() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("route", ["policy", "tn", "composed"])
@pytest.mark.parametrize("name", ["mid_text_full_ft", "mid_text_full_ft_untied"])
def test_fp32_full_ft_step_equals_the_reference(ops, name, route):
    """Loss, accuracy, sampled logits and lse, the projector's gradients and EVERY tensor of the decoder (the fixture's sub-grid and
    the full tensor's norm) against the real reference's fp32 step; with the weight gradients on the routes the policy picks, all on
    tasu_f32_gemm_tn, and all on the composed route."""
    from full_ft_ops import golden_case, llm_grads, stored
    from ps_slm_amd.decode_fp32 import forward_fp32
    from test_gpu_fp32_train_recipes import check_golden_grads, fp16_storage_error, step_fp32
    z, geo, sd, batch = golden_case(name)
    gm = build_ft32(geo, sd, ops)
    ft = gm.full_ft
    assert ft.f32_route is None and set(ft.f32_routes) == {"wqkv", "wo", "wgu", "wd", "head"} and set(ft.f32_routes.values()) == {"tn", "composed"}
    ft.f32_route = {"policy": None, "tn": "tn", "composed": "composed"}[route]
    # the forward reads the masters themselves: no separately allocated fp32 copies are left
    assert gm.llm.f32["layers"][1]["wd"].data_ptr() == ft.view(gm.proj.p, "wd", 1).data_ptr()
    assert gm.llm.f32["head"].data_ptr() == (gm.llm.embed if geo.tied else ft.view(gm.proj.p, "head")).data_ptr()
    st = step_fp32(gm, batch)
    assert st.fp32
    res = st.dev["loss_out"].cpu()
    print(f"{name} ({route}): loss {float(res[0]):.7f} reference {float(z['loss']):.7f} acc {float(res[1]):.7f} reference {float(z['acc']):.7f}")
    assert abs(float(res[0]) - float(z["loss"])) <= 2e-5
    assert abs(float(res[1]) - float(z["acc"])) < 1e-6
    assert check_golden_grads(gm, z) == 5
    gs = llm_grads(gm)
    want = sorted(k[len("g."):] for k in z if k.startswith("g."))
    assert sorted(gs) == want and len(want) == 12 * geo.llm_layers + 2 + (0 if geo.tied else 1)
    worst = (0.0, None)
    for k, g in gs.items():
        sub, ref = stored(g, z, k)
        bar = 2e-4 + fp16_storage_error(z["g." + k])
        err, rn = rel(sub, ref), float(g.double().norm()) / float(z["gnorm." + k])
        print(f"  {k}: relative L2 {err:.3e} (bar {bar:.3e}), norm ratio - 1 = {rn - 1.0:+.2e}")
        worst = max(worst, (err / bar, k))
        assert err < bar and abs(rn - 1.0) < 2e-4, (k, err, bar, rn)
    print(f"{name} ({route}): worst error / bar {worst[0]:.3f} at {worst[1]}")
    # the eval forward of the same model (the same masters): sampled logit columns and lse
    se = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"])
    forward_fp32(gm, se)
    torch.cuda.synchronize()
    valid = torch.from_numpy(se.plan.key_mask[:, : se.S].astype(bool))
    lg = se.dev["logits"].view(se.B, se.S, -1).cpu()
    refl = torch.from_numpy(z["logits_cols"])
    assert float((lg[:, :, torch.from_numpy(z["cols"])] - refl)[valid].abs().max() / refl[valid].abs().max()) < 2e-5
    lse = se.dev["row_lse"].cpu().view(se.B, se.S)
    assert float((lse - torch.from_numpy(z["lse"]))[valid].abs().max()) < 2e-5 * float(np.abs(z["lse"]).max())


# ------------------------------------------------------------------------------------------ 4. use_emb in fp32
@pytest.mark.parametrize("name", ["mid_text_lora_emb", "mid_text_lora_emb_untied"])
def test_fp32_use_emb_step_equals_the_reference(ops, name):
    from test_gpu_fp32_train_recipes import fp16_storage_error, lora_model, step_fp32
    from test_use_emb_cpu import golden_case
    z, geo, cfg, sd, lsd, batch = golden_case(name)
    gm = lora_model(geo, cfg, sd, lsd, ops, z["rng"] if cfg.lora_dropout > 0 else None)
    gm.enable_embedding_training()
    assert gm.arith_train == "fp32" and gm.llm.embed.data_ptr() == gm.embed_view(gm.proj.p).data_ptr()
    st = step_fp32(gm, batch)
    res = st.dev["loss_out"].cpu()
    print(f"{name}: loss {float(res[0]):.7f} reference {float(z['loss']):.7f}")
    assert st.fp32 and abs(float(res[0]) - float(z["loss"])) <= 2e-5
    n = 0
    for k, g in gm.lora_grads().items():
        ref16 = z["lgrad." + k]
        ref = torch.from_numpy(ref16.astype(np.float64))
        if g.shape != ref.shape:
            g = g[::2, ::2]
        bar = 2e-4 + fp16_storage_error(ref16)
        assert rel(g, ref) < bar, (k, rel(g, ref), bar)
        n += 1
    assert n == 2 * len(cfg.target_modules) * geo.llm_layers
    g = gm.embed_grad().cpu()
    rows = torch.from_numpy(z["egrad_rows"].astype(np.int64))
    ref = torch.from_numpy(z["egrad"].astype(np.float64)) / float(z["egrad_scale"])
    bar = 2e-4 + fp16_storage_error(z["egrad"])
    err = rel(g[rows], ref)
    norms = torch.from_numpy(z["egrad_norms"].astype(np.float64))
    dn = float((g.double().norm(dim=1) - norms).abs().max() / norms.max())
    print(f"{name}: table rows relative L2 {err:.3e} (bar {bar:.3e}), worst row norm error / scale {dn:.3e}")
    assert err < bar and dn < 2e-4
    assert torch.equal(g.norm(dim=1) == 0, norms == 0)                    # rows the reference leaves zero are exactly zero
    assert int((norms == 0).sum()) == (0 if geo.tied else 940)


# ------------------------------------------------------------------------------------------ 5. the audio branch
@pytest.mark.parametrize("tied", [True, False])
def test_audio_branch_fp32_full_ft_step_vs_double_autograd(ops, tied):
    """Encoder, PSD, projector and a fully trainable decoder: one step against float64 autograd through the oracle, on a sample
    of tensors."""
    from conftest import mid_audio_psd_case
    from oracle import tasu_oracle as O
    from ps_slm_amd.full_ft import EMBED_KEY
    from ps_slm_amd.train_fp32 import forward_train_fp32
    geo, sd, batch, z = mid_audio_psd_case()
    geo = dataclasses.replace(geo, tied=tied)
    sd = dict(sd)
    sd.pop("llm.lm_head.weight", None)
    if not tied:
        sd["llm.lm_head.weight"] = torch.randn(geo.llm_vocab, geo.llm_dim, generator=torch.Generator().manual_seed(77)) * 0.05
    keys = ["llm.model.layers.1.mlp.down_proj.weight", "llm.model.layers.0.self_attn.k_proj.weight", "llm.model.layers.0.self_attn.q_proj.bias",
            "llm.model.layers.1.post_attention_layernorm.weight", "llm.model.norm.weight", EMBED_KEY] + ([] if tied else ["llm.lm_head.weight"])
    W = {k: v.double() for k, v in sd.items()}
    for k in keys:
        W[k] = W[k].clone().requires_grad_(True)
    out = O.forward_audio(W, dict(batch, input_features=batch["input_features"].double()), dataclasses.asdict(geo), mode="fp32")
    ref = dict(zip(keys, torch.autograd.grad(out["loss"], [W[k] for k in keys])))
    gm = build_ft32(geo, sd, ops)
    st = gm.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"],
                          batch["input_feature_length"], fp32=True)
    forward_train_fp32(gm, st)
    gm.run_backward(st)
    torch.cuda.synchronize()
    got, loss = float(st.dev["loss_out"][0]), float(out["loss"].detach())
    assert st.path == "audio" and abs(got - loss) <= 2e-5 * max(1.0, abs(loss)), (got, loss)
    gs = gm.full_ft.grads()
    gs[EMBED_KEY] = gm.embed_grad()
    for k in keys:
        err = rel(gs[k], ref[k])
        print(f"audio full FT (tied {tied}) {k}: relative L2 {err:.3e}")
        assert err < 2e-4, (k, err)


# ------------------------------------------------------------------------------------------ 6. factory and engine
def _factory(tied=True, freeze_llm=False, ga=1, lr=2e-2, seed=77, **kw):
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    projector = kw.pop("projector", "linear-silu")
    peft = kw.pop("peft_config", None)
    use_emb = kw.pop("use_emb", False)
    tc = TrainConfig(freeze_llm=freeze_llm, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, **kw)
    if peft:
        tc.peft_config.r, tc.peft_config.lora_alpha, tc.peft_config.lora_dropout = peft["r"], peft["lora_alpha"], peft["lora_dropout"]
    tc.use_emb = use_emb
    extra = dict(encoder_projector_ds_rate=2) if projector in ("linear", "cov1d-linear") else {}
    mc = ModelConfig(llm_path="synthetic:mid" if tied else "synthetic:mid-untied", encoder_projector=projector, llm_dim=256, **extra)
    model, _ = model_factory(tc, mc, device="cuda:0", init_seed=seed)
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg.update(lr=lr, gradient_accumulation_steps=ga)                    # lr 2e-2: one step has to move the argmax of some position
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10
    return model, eng


def _raw(geo, seed=5):
    from ps_slm_amd.synthetic import synthetic_text_batch
    return synthetic_text_batch(geo, 2, seed=seed, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)


def test_factory_builds_a_fully_trainable_llm_on_the_reference_defaults():
    """freeze_llm = false with the dataclass defaults of use_fp16 (false) and mixed_precision (true): the reference run that sets
    neither flag.  On the parent commit the factory raised NotImplementedError.  One engine step moves every tensor."""
    from ps_slm_amd.config import TrainConfig
    from test_lora_cpu import to_call
    assert TrainConfig().use_fp16 is False and TrainConfig().mixed_precision is True
    model, eng = _factory()
    core = model.core
    assert core.full_ft is not None and core.arith == "fp32" and core.arith_train == "fp32"
    before = {k: v.clone() for k, v in model.state_dict().items()}
    for k in ("llm.model.layers.0.mlp.down_proj.weight", "llm.model.norm.weight", "llm.model.embed_tokens.weight"):
        assert k in before
    out, _ = eng(**to_call(_raw(core.geo)))
    eng.backward(out.loss)
    eng.step()
    torch.cuda.synchronize()
    assert model.last_state.fp32
    after = model.state_dict()
    assert len(after) == 6 + 12 * core.geo.llm_layers + 2
    for k, v in after.items():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, before[k]), k


def test_factory_rules_for_the_fp32_recipes():
    # use_peft + use_emb with fp32 everywhere builds: [projector | adapters | table]
    model, _ = _factory(use_peft=True, use_emb=True, use_fp16=False, mixed_precision=False, freeze_llm=True,
                        peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0))
    core = model.core
    assert core.arith_train == "fp32" and core.lora is not None and core.embed_base is not None and core.full_ft is None
    assert "llm.base_model.model.model.embed_tokens.weight" in model.state_dict()
    # an alternate projector trains in fp32 with mixed_precision = false ...
    model, _ = _factory(projector="linear", use_fp16=False, mixed_precision=False)
    assert model.core.full_ft is not None and model.core.arith_train == "fp32"
    # ... and with mixed_precision = true it would train in bf16 and evaluate in fp32: refused by name
    with pytest.raises(NotImplementedError, match="freeze_llm") as e:
        _factory(projector="linear", use_fp16=False, mixed_precision=True)
    assert "mixed_precision=false" in str(e.value)


@pytest.mark.parametrize("tied", [True, False])
def test_fp32_decode_and_eval_follow_the_stepped_llm(tied):
    """generate() before the step fills every cache (fragment-order copies, transposes, decode graphs); after one engine step it
    equals, token for token, generate() of a fresh model loaded from the stepped model's state_dict(), the eval loss bit for bit,
    and both differ from before the step."""
    from test_lora_cpu import to_call
    model, eng = _factory(tied)
    core = model.core
    raw = _raw(core.geo)
    ids = raw["input_ids"][:, :10]
    am = torch.ones_like(ids, dtype=torch.bool)
    targets = ["ab cde f ghij kl m", "no pq rst uvw"]
    gen = lambda m: m.generate(input_ids=ids, attention_mask=am, targets=targets, num_beams=4, max_new_tokens=12).cpu().numpy()
    ev = lambda m: m.eval()(**to_call(raw))[0].loss.detach().cpu().clone()
    model.eval()
    t0, l0 = gen(model), ev(model)
    model.train()
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    eng.step()
    out, _ = eng(**to_call(raw))                                         # a second step: the dgrads' transposed copies were redone
    eng.backward(out.loss)
    eng.step()
    model.eval()
    t1, l1 = gen(model), ev(model)
    ckpt = {k: v.cpu() for k, v in model.state_dict().items()}
    assert "llm.model.layers.1.self_attn.q_proj.bias" in ckpt and ("llm.lm_head.weight" in ckpt) == (not tied)
    fresh, eng_f = _factory(tied, seed=78)
    missing, unexpected = fresh.load_state_dict(ckpt)
    assert not missing and not unexpected
    t2, l2 = gen(fresh), ev(fresh)
    torch.cuda.synchronize()
    assert core.arith == "fp32" and np.array_equal(t1, t2), (t1, t2)
    assert torch.equal(l1, l2) and not torch.equal(l1, l0)
    assert not np.array_equal(t0, t1)
    # the stepped model's next training loss equals the fresh model's: the dgrad copies and the masters agree in both
    model.train(), fresh.train()
    la, _ = eng(**to_call(raw))
    lb, _ = eng_f(**to_call(raw))
    eng.backward(la.loss), eng_f.backward(lb.loss)
    torch.cuda.synchronize()
    assert torch.equal(la.loss.detach(), lb.loss.detach()) and torch.equal(core.proj.g, fresh.core.proj.g)


def test_gradient_accumulation_and_the_autograd_route():
    """gradient_accumulation_steps = k = 2: the update equals one AdamW step on g1 / 4 + g2 / 4 (TasuEngine adds every micro-step's
    bucket with weight 1 / k^2: the weighting its other recipes are tested for), and no optimizer step happens in between.
    outputs.loss.backward() through _HipStep hands the leaves the gradients engine.backward() leaves in the bucket."""
    from test_lora_cpu import to_call
    model, eng = _factory(ga=2, lr=1e-3)
    core = model.core
    grads, p0 = [], core.proj.p.clone()
    for s in (5, 6):
        out, _ = eng(**to_call(_raw(core.geo, s)))
        eng.backward(out.loss)
        grads.append(core.proj.g.clone())
        eng.step()
        if len(grads) == 1:
            assert torch.equal(core.proj.p, p0)
    m2, e2 = _factory(ga=1, lr=1e-3)
    m2.core.proj.g.copy_(grads[0] / 4 + grads[1] / 4)
    e2.step()
    torch.cuda.synchronize()
    assert torch.equal(m2.core.proj.p, core.proj.p) and not torch.equal(core.proj.p, p0)
    # the autograd route on a third model of the same seed: the first micro-batch's gradients, bit for bit
    m3, _ = _factory(ga=1, lr=1e-3)
    m3.train()
    out, _ = m3(**to_call(_raw(core.geo, 5)))
    out.loss.backward()
    torch.cuda.synchronize()
    assert m3.last_state.fp32
    n = 0
    for (name, p), (_, gv) in zip(m3.named_parameters(), m3._trainable_views(grads[0])):
        assert p.grad is not None and torch.equal(p.grad, gv), name
        n += 1
    assert n == 6 + 12 * core.geo.llm_layers + 2


# ------------------------------------------------------------------------------------------ 7. determinism and resume
def _resume_make(kw, llm_path, reseed):
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory

    def make(other):
        k = dict(kw)
        peft, use_emb = k.pop("peft_config", None), k.pop("use_emb", False)
        tc = TrainConfig(freeze_encoder=True, gt_emb=True, ctc_posterior=True, do_psd=True, gt_emb_noise=True, **k)
        if peft:
            tc.peft_config.r, tc.peft_config.lora_alpha, tc.peft_config.lora_dropout = peft["r"], peft["lora_alpha"], peft["lora_dropout"]
        tc.use_emb = use_emb
        mc = ModelConfig(llm_path=llm_path, encoder_projector="linear-silu", llm_dim=256)
        model, _ = model_factory(tc, mc, device="cuda:0", init_seed=4321 if (other and reseed) else 1234, keep_logits=False)
        cfg = load_ds_config(DEFAULT_DS_CONFIG)
        cfg.update(lr=1e-3, gradient_accumulation_steps=1)
        eng = TasuEngine(model, cfg)
        eng.sched_iter = 10
        return model, eng
    return make


RESUME = {
    "full_ft_fp32": (dict(freeze_llm=False, use_fp16=False), "synthetic:mid", True),
    "full_ft_fp32_untied": (dict(freeze_llm=False, use_fp16=False), "synthetic:mid-untied", True),
    "lora_emb_fp32": (dict(freeze_llm=True, use_fp16=False, mixed_precision=False, use_peft=True, use_emb=True,
                           peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.05)), "synthetic:mid", False),
}


@pytest.mark.parametrize("recipe", list(RESUME))
def test_three_steps_are_deterministic_and_resume_after_the_second(tmp_path, recipe):
    """Two uninterrupted runs of three steps give equal bits in p, m, v (and the bf16 image and the losses); save_state after step 2,
    load_state into a model built from another init_seed (where the decoder trains; else spoiled in every element), then step 3:
    the uninterrupted run's bits."""
    import resume_cases as rc
    a, c, control = rc.resume_pattern(_resume_make(*RESUME[recipe]), tmp_path, N=3, k=2, what=recipe)
    assert control == 0.0                                                # the control: A and A' are bit-equal
    assert a.core.arith_train == "fp32" and c.core.arith_train == "fp32"
    assert (a.core.full_ft is not None) == recipe.startswith("full_ft") and (a.core.lora is not None) == recipe.startswith("lora")
