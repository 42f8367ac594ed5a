"""The weight-gradient kernels of the decoder's own tensors (csrc/wgrad.hip, full fine-tuning of the LLM) on the GPU:
tasu_gemm_tn_bf16 (dW = dY^T X from the row-major bf16 operands, no transposed copies) and tasu_rmsnorm_wgrad against float64 on
the very inputs the kernels read, with bounds derived from the arithmetic (not measured), run-to-run bit equality, untouched
surroundings and the argument rules of include/tasu_hip.h."""
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


# (N, lda or None = N, K): 64 x 64 = a quarter of one tile; several tiles; N that ends inside a tile and inside A's row (columns past
# N hold NaN: they must never be read into a stored element); K = the 1.5B hidden size with N = one and a half tiles
TN_SHAPES = [(64, None, 64), (512, None, 256), (256, None, 512), (1000, 1024, 256), (192, None, 1536)]


@pytest.mark.parametrize("N,lda,K", TN_SHAPES)
@pytest.mark.parametrize("R", [64, 100, 192, 1024])                      # 100: a last stage of 36 rows (zeroed in LDS past R)
def test_gemm_tn_against_float64(ops, R, N, lda, K):
    g = torch.Generator().manual_seed(R * 7 + N * 3 + K)
    lda = lda or N
    a = torch.full((R, lda), float("nan"), dtype=torch.bfloat16)
    a[:, :N] = torch.randn(R, N, generator=g).to(torch.bfloat16)
    b = torch.randn(R, K, generator=g).to(torch.bfloat16)
    ad, bd = a[:, :N].double(), b.double()
    ref, mag = ad.t() @ bd, ad.abs().t() @ bd.abs()                      # exact products, float64 sums
    ldc, rows_c = K + 8, N + 3                                            # C sits inside a larger pre-filled buffer
    c0 = torch.randn(rows_c, ldc, generator=g)
    nstages = (R + 63) // 64
    splits = sorted({1, min(3, nstages), min(ops.gemm_tn_split(R, N, K), nstages)})
    ag, bg = a.cuda(), b.cuda()
    for accumulate in (False, True):
        for nsplit in splits:
            ws = torch.full((nsplit * N * K,), float("nan"), device="cuda") if nsplit > 1 else None
            outs = []
            for _ in range(2):
                c = c0.cuda()
                ops.gemm_tn(ag, bg, c, R, N, K, accumulate=accumulate, nsplit=nsplit, ws=ws)
                torch.cuda.synchronize()
                outs.append(c.cpu())
            assert torch.equal(outs[0], outs[1]), (accumulate, nsplit)   # no atomics: the same bits on every run
            got = outs[0][:N, :K].double()
            want = ref + c0[:N, :K].double() if accumulate else ref
            # bf16 products are exact in fp32; R additions, the factor 2 for the order inside an MFMA (and the slab sums); one ulp
            # of the pre-filled value when accumulating
            bound = 2 * R * EPS * mag + (_ulp(c0[:N, :K]) if accumulate else 0)
            err = (got - want).abs()
            assert bool((err <= bound).all()), (accumulate, nsplit, float((err / bound.clamp_min(1e-300)).max()))
            assert torch.equal(outs[0][N:], c0[N:]) and torch.equal(outs[0][:, K:], c0[:, K:]), (accumulate, nsplit)   # bitwise
            assert not torch.equal(outs[0][:N, :K], c0[:N, :K])


def test_gemm_tn_split_plan_fills_the_chip_for_small_outputs(ops):
    """Host code: the number of row ranges for the training-step shapes -- outputs of a few hundred 128 x 128 tiles run whole,
    o_proj at Qwen2.5-1.5B (144 tiles) is cut, and never into more ranges than there are 64-row stages."""
    assert ops.gemm_tn_split(4096, 1536, 1536) == 3
    assert ops.gemm_tn_split(4096, 2048, 1536) == 2
    assert ops.gemm_tn_split(4096, 17920, 1536) == 1 and ops.gemm_tn_split(4096, 1536, 8960) == 1
    assert ops.gemm_tn_split(2048, 151936, 1536) == 1
    assert ops.gemm_tn_split(4096, 3584, 3584) == 1 and ops.gemm_tn_split(4096, 4608, 3584) == 1
    assert ops.gemm_tn_split(64, 64, 64) == 1 and ops.gemm_tn_split(192, 64, 64) == 3 and ops.gemm_tn_split(4096, 64, 64) == 16
    assert ops.gemm_tn_split(0, 64, 64) == -1


def test_gemm_tn_rejects_bad_arguments(ops):
    lib = ops.lib
    a = torch.zeros(128, 136, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(128, 72, dtype=torch.bfloat16, device="cuda")
    c = torch.zeros(128, 72, device="cuda")
    ws = torch.zeros(2 * 128 * 64, device="cuda")
    p = lambda t: t.data_ptr()

    def call(A=p(a), lda=136, B=p(b), ldb=72, C=p(c), ldc=72, R=128, N=128, K=64, acc=0, nsplit=1, W=None, wf=0):
        return lib.tasu_gemm_tn_bf16(A, lda, B, ldb, C, ldc, R, N, K, acc, nsplit, W, wf, None)

    assert call(A=None) == 1 and call(B=None) == 1 and call(C=None) == 1
    assert call(R=0) == 1 and call(N=0) == 1 and call(K=0) == 1
    assert call(N=124) == 1 and call(K=60) == 1                           # multiples of 8
    assert call(lda=120) == 1 and call(ldb=56) == 1 and call(ldc=56) == 1   # shorter than the operand
    assert call(lda=140) == 1 and call(ldb=76) == 1 and call(ldc=74) == 1   # % 8, % 8, % 4
    assert call(A=p(a) + 2) == 1 and call(B=p(b) + 8) == 1 and call(C=p(c) + 4) == 1   # 16-byte alignment
    assert call(nsplit=0) == 1 and call(nsplit=3) == 1 and call(nsplit=17, R=4096) == 1   # 128 rows = 2 stages; the cap
    assert call(nsplit=2) == 1 and call(nsplit=2, W=p(ws), wf=2 * 128 * 64 - 1) == 1   # no / too small a workspace
    assert call(nsplit=2, W=p(ws) + 4, wf=2 * 128 * 64) == 1
    assert call() == 0 and call(nsplit=2, W=p(ws), wf=2 * 128 * 64) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [256, 1536, 3584])
@pytest.mark.parametrize("R", [1, 77, 300, 1024])
def test_rmsnorm_wgrad_against_float64(ops, R, D):
    from ps_slm_amd.ops import RMS_WGRAD_SPLIT
    g = torch.Generator().manual_seed(R * 13 + D)
    dy = torch.randn(R, D, generator=g).to(torch.bfloat16)
    x = torch.randn(R, D, generator=g) * 3
    rstd = torch.rand(R, generator=g) + 0.2
    terms = dy.double() * x.double() * rstd.double()[:, None]
    ref, mag = terms.sum(0), terms.abs().sum(0)
    dw0 = torch.randn(D + 4, generator=g)
    ws = torch.full((RMS_WGRAD_SPLIT * D,), float("nan"), device="cuda")
    for accumulate in (False, True):
        outs = []
        for _ in range(2):
            dw = dw0.cuda()
            ops.rmsnorm_wgrad(dy.cuda(), x.cuda(), rstd.cuda(), dw[:D], ws, accumulate=accumulate)
            torch.cuda.synchronize()
            outs.append(dw.cpu())
        assert torch.equal(outs[0], outs[1])
        want = ref + dw0[:D].double() if accumulate else ref
        # two roundings per term, at most R - 1 additions over the two stages
        bound = (R + 2) * EPS * mag + (_ulp(dw0[:D]) + _ulp(want) if accumulate else 0)
        err = (outs[0][:D].double() - want).abs()
        assert bool((err <= bound).all()), (accumulate, float((err / bound.clamp_min(1e-300)).max()))
        assert torch.equal(outs[0][D:], dw0[D:])


@pytest.mark.parametrize("n,M,D", [(64, 150, 256), (192, 301, 1536)])
def test_rmsnorm_wgrad_row_compacted_form(ops, n, M, D):
    """dy / rstd compact [n], x indexed by src_rows (the labelled-rows form of tasu_rmsnorm_bwd_rows); src_rows < 0: padding."""
    from ps_slm_amd.ops import RMS_WGRAD_SPLIT
    g = torch.Generator().manual_seed(n + M + D)
    n_real = n - 9
    rows = torch.full((n,), -1, dtype=torch.int32)
    rows[:n_real] = torch.randperm(M, generator=g)[:n_real].sort().values.to(torch.int32)
    dy = torch.randn(n, D, generator=g).to(torch.bfloat16)
    x = torch.randn(M, D, generator=g)
    rstd = torch.rand(n, generator=g) + 0.2
    terms = dy[:n_real].double() * x[rows[:n_real].long()].double() * rstd[:n_real].double()[:, None]
    ws = torch.zeros(RMS_WGRAD_SPLIT * D, device="cuda")
    outs = []
    for _ in range(2):
        dw = torch.full((D,), float("nan"), device="cuda")
        ops.rmsnorm_wgrad(dy.cuda(), x.cuda(), rstd.cuda(), dw, ws, src_rows=rows.cuda())
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])
    err = (outs[0].double() - terms.sum(0)).abs()
    assert bool((err <= (n + 2) * EPS * terms.abs().sum(0)).all())


@pytest.mark.parametrize("R,C,ld", [(1, 256, 256), (77, 512, 520), (1024, 2048, 2048), (300, 100, 104)])
def test_colsum_split_against_float64(ops, R, C, ld):
    """tasu_colsum_bf16_split: R - 1 fp32 additions of exact bf16 values, any order; columns past C and the rest of `out` untouched."""
    from ps_slm_amd.ops import RMS_WGRAD_SPLIT
    g = torch.Generator().manual_seed(R + C)
    x = torch.randn(R, ld, generator=g).to(torch.bfloat16)
    out0 = torch.randn(C + 4, generator=g)
    ws = torch.full((RMS_WGRAD_SPLIT * C,), float("nan"), device="cuda")
    ref, mag = x[:, :C].double().sum(0), x[:, :C].double().abs().sum(0)
    for accumulate in (False, True):
        outs = []
        for _ in range(2):
            out = out0.cuda()
            ops.colsum_split(x.cuda(), out, ws, R, C, accumulate=accumulate)
            torch.cuda.synchronize()
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0][C:], out0[C:])
        want = ref + out0[:C].double() if accumulate else ref
        bound = R * EPS * mag + (_ulp(out0[:C]) + _ulp(want) if accumulate else 0)
        assert bool(((outs[0][:C].double() - want).abs() <= bound).all())
    lib, p = ops.lib, lambda v: v.data_ptr()
    xg = x.cuda()
    assert lib.tasu_colsum_bf16_split(p(xg), ld, p(ws), None, R, C, 0, None) == 1 and lib.tasu_colsum_bf16_split(p(xg), C - 4, p(ws), p(ws), R, C, 0, None) == 1
    assert lib.tasu_colsum_bf16_split(p(xg), ld, p(ws), p(ws), R, C - 2, 0, None) == 1


def test_rmsnorm_wgrad_rejects_bad_arguments(ops):
    lib = ops.lib
    t = torch.zeros(64 * 256, device="cuda")
    d = torch.zeros(8, 256, dtype=torch.bfloat16, device="cuda")
    p = lambda v: v.data_ptr()
    assert lib.tasu_rmsnorm_wgrad(None, p(t), p(t), None, p(t), p(t), 8, 256, 0, None) == 1
    assert lib.tasu_rmsnorm_wgrad(p(d), p(t), p(t), None, p(t), None, 8, 256, 0, None) == 1      # no workspace
    assert lib.tasu_rmsnorm_wgrad(p(d), p(t), p(t), None, p(t), p(t), 8, 254, 0, None) == 1      # D % 4
    assert lib.tasu_rmsnorm_wgrad(p(d), p(t), p(t), None, p(t), p(t), 0, 256, 0, None) == 1
    assert lib.tasu_rmsnorm_wgrad(p(d), p(t) + 4, p(t), None, p(t), p(t), 8, 256, 0, None) == 1  # x: 16-byte alignment


def test_gemm_tn_equals_the_composed_route_to_rounding(ops):
    """The route the projector's weight gradients take (two tasu_transpose_bf16 + the NT GEMM in fp32 mode) and tasu_gemm_tn_bf16
    compute the same sums of exact products in different orders: both within the derived bound of the float64 result."""
    from ps_slm_amd.ops import GEMM_F32
    R, N, K = 256, 384, 256
    g = torch.Generator().manual_seed(5)
    a = torch.randn(R, N, generator=g).to(torch.bfloat16).cuda()
    b = torch.randn(R, K, generator=g).to(torch.bfloat16).cuda()
    a_t = torch.zeros(N, R, dtype=torch.bfloat16, device="cuda")
    b_t = torch.zeros(K, R, dtype=torch.bfloat16, device="cuda")
    ops.transpose(a, a_t, R, N, R, N)
    ops.transpose(b, b_t, R, K, R, K)
    c_old = torch.zeros(N, K, device="cuda")
    ops.gemm(a_t, b_t, c_old, N, K, R, mode=GEMM_F32)
    c_new = torch.zeros(N, K, device="cuda")
    ops.gemm_tn(a, b, c_new, R, N, K)
    torch.cuda.synchronize()
    ref = a.double().t() @ b.double()
    bound = 2 * R * EPS * (a.double().abs().t() @ b.double().abs())
    assert bool(((c_new.double() - ref).abs() <= bound).all()) and bool(((c_old.double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------ the training step (freeze_llm=false)
@pytest.fixture(scope="module")
def double_runs():
    """The CPU double's step on both golden cases, computed once."""
    from full_ft_ops import GOLDENS, FullFtFakeOps, build_ft, golden_case, llm_grads
    from test_lora_cpu import run_text
    out = {}
    for name in GOLDENS:
        z, geo, sd, batch = golden_case(name)
        cm = build_ft(geo, sd, FullFtFakeOps(), "cpu")
        sc = run_text(cm, batch)
        out[name] = (float(sc.dev["loss_out"][0]), llm_grads(cm), cm.projector_grads())
    return out


@pytest.mark.parametrize("route", ["policy", "tn", "composed"])
@pytest.mark.parametrize("name", ["mid_text_full_ft", "mid_text_full_ft_untied"])
def test_full_ft_step_hip_vs_reference_golden_and_double(ops, double_runs, name, route):
    """The step on the HIP kernels against the reference's fp32 gradients (the bf16 bars of the CPU test) and against the CPU double
    (loss within 2e-3, every tensor cosine > 0.9995 and relative error < 3e-2: the use_emb GPU test's bars); with the weight
    gradients on the route the shape policy picks, all on tasu_gemm_tn_bf16, and all on the composed route."""
    from full_ft_ops import build_ft, golden_case, llm_grads
    from test_full_ft_cpu import check_step_against_golden
    from test_lora_cpu import cosine, run_text
    z, geo, sd, batch = golden_case(name)
    gm = build_ft(geo, sd, ops, "cuda")
    gm.full_ft.tn_min_split = {"policy": gm.full_ft.tn_min_split, "tn": 1, "composed": 99}[route]
    sg = run_text(gm, batch)
    torch.cuda.synchronize()
    check_step_against_golden(gm, sg, z, show=f"{name} (HIP, {route})")
    loss_c, lg_c, pg_c = double_runs[name]
    assert abs(float(sg.dev["loss_out"][0]) - loss_c) < 2e-3
    worst = (2.0, 0.0, None)
    for k, g2 in lg_c.items():
        g1 = llm_grads(gm)[k].cpu() if k.endswith("embed_tokens.weight") else gm.full_ft.grads()[k].cpu()
        c, rel = cosine(g1, g2), float((g1 - g2).norm() / g2.norm())
        worst = min(worst, (c, rel, k))
        assert c > 0.9995 and rel < 3e-2, (k, c, rel)
    print(f"{name} ({route}): HIP vs double: lowest cosine {worst[0]:.6f} (relative error {worst[1]:.2e}) at {worst[2]}")
    for k, g2 in pg_c.items():
        assert cosine(gm.projector_grads()[k], g2) > 0.9995, k


@pytest.mark.parametrize("name", ["mid_text_full_ft", "mid_text_full_ft_untied"])
def test_full_ft_graph_replay_equals_eager_on_another_batch(ops, name):
    """Eager launches against hipGraph replay on a DIFFERENT batch of the same shape (first call eager, second captured, third
    replayed): the loss and the whole gradient bucket, bit for bit."""
    from full_ft_ops import build_ft, golden_case
    from ps_slm_amd.synthetic import synthetic_text_batch
    z, geo, sd, _ = golden_case(name)
    gm = build_ft(geo, sd, ops, "cuda")
    gm.keep_logits = False                                              # the throughput mode: the labelled rows only
    mk = lambda seed: synthetic_text_batch(geo, 3, seed=seed, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=False)
    b1, b2 = mk(41), mk(42)
    assert not torch.equal(b1["input_ids"], b2["input_ids"]) and b1["input_ids"].shape == b2["input_ids"].shape

    def step(batch, graphs):
        gm.use_graphs = graphs
        st = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"])
        gm.run_forward_text(st)
        gm.run_backward(st)
        torch.cuda.synchronize()
        gm.use_graphs = False
        return st, st.dev["loss_out"].clone(), gm.proj.g.clone()

    st1, loss_e, g_e = step(b2, False)
    step(b1, True), step(b1, True)
    st2, loss_g, g_g = step(b2, True)
    assert gm._shape_key(st2, ("fwd_text", True, True)) in gm._graphs and gm._shape_key(st2, "bwd") in gm._graphs
    assert torch.equal(loss_e, loss_g) and torch.equal(g_e, g_g)
    lo, hi = gm.full_ft.layer_range[0]
    assert float(g_g[lo:hi].abs().max()) > 0 and not torch.equal(g_g[lo:hi], step(b1, True)[2][lo:hi])


@pytest.mark.parametrize("tied", [True, False])
def test_full_ft_audio_branch_hip_vs_double(ops, tied):
    """One audio-branch step (encoder, PSD, projector, decoder) on the HIP kernels against the CPU double, on a sample of tensors."""
    import dataclasses
    from conftest import mid_audio_psd_case
    from full_ft_ops import FullFtFakeOps, build_ft
    from test_lora_cpu import cosine
    from test_use_emb_cpu import run_audio
    geo, sd, batch, z = mid_audio_psd_case()
    geo = dataclasses.replace(geo, tied=tied)
    if not tied:
        sd = dict(sd)
        sd["llm.lm_head.weight"] = torch.randn(geo.llm_vocab, geo.llm_dim, generator=torch.Generator().manual_seed(77)) * 0.05
    gm, cm = build_ft(geo, sd, ops, "cuda"), build_ft(geo, sd, FullFtFakeOps(), "cpu")
    sg, sc = run_audio(gm, batch), run_audio(cm, batch)
    torch.cuda.synchronize()
    assert sg.path == "audio" and abs(float(sg.dev["loss_out"][0]) - float(sc.dev["loss_out"][0])) < 2e-3
    g1, g2 = gm.full_ft.grads(), cm.full_ft.grads()
    keys = ["llm.model.layers.1.mlp.down_proj.weight", "llm.model.layers.0.self_attn.k_proj.weight", "llm.model.layers.0.self_attn.q_proj.bias",
            "llm.model.layers.1.post_attention_layernorm.weight", "llm.model.layers.0.mlp.up_proj.weight", "llm.model.norm.weight"]
    keys += [] if tied else ["llm.lm_head.weight"]
    for k in keys:
        c, rel = cosine(g1[k], g2[k]), float((g1[k].cpu() - g2[k]).norm() / g2[k].norm())
        assert c > 0.9995 and rel < 3e-2, (k, c, rel)
    e1, e2 = gm.embed_grad().cpu(), cm.embed_grad()
    assert cosine(e1, e2) > 0.9995 and float((e1 - e2).norm() / e2.norm()) < 3e-2


def _factory(tied, freeze_llm=False, fp16=True):
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    tc = TrainConfig(freeze_llm=freeze_llm, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True, use_fp16=fp16)
    mc = ModelConfig(llm_path="synthetic:mid" if tied else "synthetic:mid-untied", encoder_projector="linear-silu", llm_dim=256)
    model, tok = model_factory(tc, mc, device="cuda:0", init_seed=77)
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg["lr"] = 2e-2                                                    # one step has to move the argmax of some position
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10
    return model, eng


def test_factory_builds_and_steps_a_fully_trainable_llm():
    """model_factory(TrainConfig(freeze_llm=False, use_fp16=True, ...)) builds, and one engine step moves every tensor of the
    decoder (on the parent commit the factory raised NotImplementedError)."""
    from ps_slm_amd.synthetic import synthetic_text_batch
    from test_lora_cpu import to_call
    model, eng = _factory(True)
    core = model.core
    assert core.full_ft is not None and core.arith_train == "bf16"
    before = {k: v.clone() for k, v in model.state_dict().items()}
    raw = synthetic_text_batch(core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    out, _ = eng(**to_call(raw))
    eng.backward(out.loss)
    eng.step()
    torch.cuda.synchronize()
    after = model.state_dict()
    assert len(after) == 6 + 12 * core.geo.llm_layers + 2
    for k, v in after.items():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, before[k]), k


@pytest.mark.parametrize("tied", [True, False])
def test_decode_and_eval_follow_the_stepped_llm(tied):
    """generate() before the step fills every cache (fragment-order copies, decode graphs); after one engine step at lr 2e-2 it
    equals, token for token, generate() of a fresh model loaded from the stepped model's state_dict(), the eval loss bit for bit,
    and both differ from before the step.  The same checkpoint loaded into a freeze_llm=true, use_fp16=false model decodes on the
    fp32 path."""
    from ps_slm_amd.synthetic import synthetic_text_batch
    from test_lora_cpu import to_call
    model, eng = _factory(tied)
    core = model.core
    raw = synthetic_text_batch(core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
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
    model.eval()
    t1, l1 = gen(model), ev(model)
    ckpt = {k: v.cpu() for k, v in model.state_dict().items()}
    fresh, _ = _factory(tied)
    missing, unexpected = fresh.load_state_dict(ckpt)
    assert not missing and not unexpected
    t2, l2 = gen(fresh), ev(fresh)
    torch.cuda.synchronize()
    assert np.array_equal(t1, t2), (t1, t2)
    assert torch.equal(l1, l2) and not torch.equal(l1, l0)
    assert not np.array_equal(t0, t1)
    frozen32, _ = _factory(tied, freeze_llm=True, fp16=False)
    assert frozen32.core.arith == "fp32" and frozen32.core.full_ft is None
    missing, unexpected = frozen32.load_state_dict(ckpt)
    assert not missing and not unexpected
    t3 = gen(frozen32)
    l3 = ev(frozen32)
    torch.cuda.synchronize()
    assert t3.shape[0] == 2 and abs(float(l3) - float(l1)) < 2e-2      # fp32 arithmetic on the same weights: the project's bf16 loss bar
