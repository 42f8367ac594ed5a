"""The fp32 training step (ps_slm_amd/train_fp32.py) of the alternate projectors -- linear, cov1d-linear, cross-attention -- and of
LoRA models (use_peft: the adapters unmerged, dropout included) against
the REAL reference's fp32 goldens at the fp32 bars of tests/test_gpu_model.py::test_training_step_in_fp32_equals_the_reference_to_fp32_
rounding (loss 2e-5, accuracy 1e-6, projector gradients 2e-4 relative L2), the new kernels (tasu_f32_ca_attn_bwd, tasu_f32_ca_attn_lse,
tasu_f32_relu_bwd, tasu_f32_lora_dropout, the thin rank products) against float64, the audio branch against float64 autograd, and the opt-in selection through
train_config.mixed_precision."""
import dataclasses

import numpy as np
import pytest
import torch

from test_gpu_fp32_recipes import _projector_case, ca_double
from test_gpu_fp32_recipes import f32_model as _f32_eval_model

pytestmark = pytest.mark.gpu

CASES = ["linear_k1", "linear_k2", "cov1d_k1", "cov1d_k2", "ca"]
SUBSAMPLED = {".rows8": 8, ".rows16": 16, ".rows64": 64}


@pytest.fixture(scope="module")
def ops():
    from ps_slm_amd.ops import HipOps
    return HipOps()


def f32_model(geo, sd, ops, cfg=None, lsd=None):
    """What model_factory builds for use_fp16 = false with mixed_precision = false: the fp32 weight copies and arith = fp32 of the
    eval tests' model, and the fp32 training step selected for every recipe."""
    gm = _f32_eval_model(geo, sd, ops, cfg, lsd)
    gm.arith_train = "fp32"
    return gm


def test_training_step_is_refused_without_the_selection(ops):
    """A model built as the default selection builds it (arith_train = bf16) is refused by the fp32 step of these recipes."""
    from ps_slm_amd.train_fp32 import forward_train_fp32
    geo, sd, batch, _ = _projector_case("linear_k2")
    gm = _f32_eval_model(geo, sd, ops)
    st = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], batch.get("alphas"),
                         batch.get("keeps"))
    with pytest.raises(NotImplementedError, match="mixed_precision=false"):
        forward_train_fp32(gm, st)


def step_fp32(gm, batch):
    from ps_slm_amd.train_fp32 import forward_train_fp32
    st = gm.prepare_text(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["post_ids"], batch.get("alphas"),
                         batch.get("keeps"))
    forward_train_fp32(gm, st)
    gm.run_backward(st)
    torch.cuda.synchronize()
    return st


def check_golden_grads(gm, z):
    """Every projector gradient the golden stores, the same rows where it stores a sub-sample; returns how many it saw."""
    seen = 0
    for k, g in gm.projector_grads().items():
        short = "grad." + k[len("encoder_projector."):]
        ref = None
        if short in z:
            ref = torch.from_numpy(z[short])
        for suffix, every in SUBSAMPLED.items():
            if short + suffix in z:
                ref, g = torch.from_numpy(z[short + suffix]), g[::every]
        if ref is None:
            continue
        assert tuple(ref.shape) == tuple(g.shape), (k, ref.shape, g.shape)
        seen += 1
        err = float((g.cpu().double() - ref.double()).norm() / ref.double().norm())
        print(f"{k}: relative L2 {err:.3e}")
        assert err < 2e-4, (k, err)
    return seen


# ------------------------------------------------------------------------------------------ 1. against the real reference's goldens
@pytest.mark.parametrize("name", CASES)
def test_fp32_training_step_of_alternate_projectors_equals_the_reference(ops, name):
    from test_gpu_model import run_text
    geo, sd, batch, z = _projector_case(name)
    gm = f32_model(geo, sd, ops)
    st = step_fp32(gm, batch)
    assert st.fp32
    res = st.dev["loss_out"].cpu()
    print(f"{name}: loss {float(res[0]):.7f} golden {float(z['loss']):.7f} acc {float(res[1]):.7f} golden {float(z['acc']):.7f}")
    assert abs(float(res[0]) - float(z["loss"])) <= 2e-5 * max(1.0, abs(float(z["loss"])))
    assert abs(float(res[1]) - float(z["acc"])) < 1e-6
    n_stored = sum(1 for k in z if k.startswith("grad."))
    assert n_stored >= 1 and check_golden_grads(gm, z) == n_stored
    # a second step gives the same bits
    g1 = gm.proj.g.clone()
    gm.proj.g.fill_(7.0)
    step_fp32(gm, batch)
    assert torch.equal(gm.proj.g, g1)
    # the bf16 step of the same model is the looser neighbour, not the same code
    st16 = run_text(gm, batch)
    d16 = abs(float(st16.dev["loss_out"][0]) - float(z["loss"]))
    assert 1e-6 < d16 < 2e-2, d16



# ------------------------------------------------------------------------------------------ 1b. LoRA against the goldens
def lora_model(geo, cfg, sd, lsd, ops, rng=None):
    gm = f32_model(geo, sd, ops, cfg, lsd)
    if rng is not None:
        gm.lora.seed_dropout(int(rng[0]), int(rng[1]) - 1)         # the forward advances the step before it draws (test_lora_cpu.build)
    return gm


def fp16_storage_error(ref16):
    """|| ulp_fp16(ref) / 2 || / || ref ||: what rounding the reference's fp32 gradient to the golden's fp16 may have moved it by."""
    ref = ref16.astype(np.float64)
    return float(np.linalg.norm(np.spacing(np.abs(ref16)).astype(np.float64) / 2) / np.linalg.norm(ref))


@pytest.mark.parametrize("name", ["mid_text_lora", "mid_text_lora_qv", "mid_text_lora_drop"])
def test_fp32_training_step_of_lora_models_equals_the_reference(ops, name):
    from test_lora_cpu import golden_case
    z, geo, cfg, sd, lsd, batch = golden_case(name)
    rng = z["rng"] if cfg.lora_dropout > 0 else None
    gm = lora_model(geo, cfg, sd, lsd, ops, rng)
    st = step_fp32(gm, batch)
    assert st.fp32
    res = st.dev["loss_out"].cpu()
    print(f"{name}: loss {float(res[0]):.7f} golden {float(z['loss']):.7f} acc {float(res[1]):.7f} golden {float(z['acc']):.7f}")
    assert abs(float(res[0]) - float(z["loss"])) <= 2e-5 * max(1.0, abs(float(z["loss"])))
    assert abs(float(res[1]) - float(z["acc"])) < 1e-6
    n_stored = sum(1 for k in z if k.startswith("grad."))
    assert n_stored >= 1 and check_golden_grads(gm, z) == n_stored
    n, worst = 0, 0.0
    for k, g in gm.lora_grads().items():
        ref16 = z["lgrad." + k]
        assert ref16.dtype == np.float16
        ref = torch.from_numpy(ref16.astype(np.float64))
        if g.shape != ref.shape:                                    # the r = 64 fixtures keep every 2nd row / column
            g = g[::2, ::2]
        assert g.shape == ref.shape
        bar = 2e-4 + fp16_storage_error(ref16)
        err = float((g.cpu().double() - ref).norm() / ref.norm())
        worst = max(worst, err / bar)
        assert err < bar, (k, err, bar)
        n += 1
    print(f"{name}: {n} adapter gradients, worst error / bar {worst:.3f}")
    assert n == 2 * len(cfg.target_modules) * geo.llm_layers
    # a second step gives the same bits (the same mask: the dropout step is set back)
    g1 = gm.proj.g.clone()
    gm.proj.g[gm.lora.base:].fill_(7.0)                             # (the projector's LayerNorm pad columns are never written)
    if rng is not None:
        gm.lora.seed_dropout(int(rng[0]), int(rng[1]) - 1)
    step_fp32(gm, batch)
    assert torch.equal(gm.proj.g, g1)
    # the bf16 step of the same model is the looser neighbour
    if rng is not None:
        gm.lora.seed_dropout(int(rng[0]), int(rng[1]) - 1)
    from test_lora_cpu import run_text
    st16 = run_text(gm, batch)
    torch.cuda.synchronize()
    d16 = abs(float(st16.dev["loss_out"][0]) - float(z["loss"]))
    assert 1e-6 < d16 < 2e-2, d16


def double_adapter_grads(sd, lsd, cfg, geo, batch, audio=False):
    """Loss and every dA / dB by float64 autograd through the oracle with W + s B A composed from float64 leaves A, B."""
    from fp32_oracle_cases import lora_merged_double
    from oracle import tasu_oracle as O
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in lsd.items()}
    W = lora_merged_double(sd, leaves, cfg)
    if audio:
        out = O.forward_audio(W, dict(batch, input_features=batch["input_features"].double()), dataclasses.asdict(geo), mode="fp32")
    else:
        out = O.forward_text(W, batch, dataclasses.asdict(geo), mode="fp32")
    keys = list(leaves)
    return float(out["loss"].detach()), dict(zip(keys, torch.autograd.grad(out["loss"], [leaves[k] for k in keys])))


@pytest.mark.parametrize("zero_b", [False, True])
def test_adapter_gradients_at_full_precision_vs_double_autograd(ops, zero_b):
    """Fixture geometry and seeds of mid_text_lora, p = 0: every dA, dB within 2e-4 relative L2 of float64 autograd, the loss within
    2e-5; with B = 0 (peft's init) dA is exactly zero."""
    from test_lora_cpu import golden_case
    z, geo, cfg, sd, lsd, batch = golden_case("mid_text_lora")
    assert cfg.lora_dropout == 0.0
    if zero_b:
        lsd = {k: (torch.zeros_like(v) if "lora_B" in k else v) for k, v in lsd.items()}
    gm = lora_model(geo, cfg, sd, lsd, ops)
    st = step_fp32(gm, batch)
    loss, ref = double_adapter_grads(sd, lsd, cfg, geo, batch)
    got = float(st.dev["loss_out"][0])
    assert abs(got - loss) <= 2e-5 * max(1.0, abs(loss)), (got, loss)
    gg = gm.lora_grads()
    assert set(gg) == set(ref) and len(gg) == 2 * len(cfg.target_modules) * geo.llm_layers
    worst = 0.0
    for k, r in ref.items():
        g = gg[k].cpu().double()
        if zero_b and "lora_A" in k:
            assert float(g.abs().max()) == 0.0 and float(r.abs().max()) == 0.0, k
            continue
        err = float((g - r).norm() / r.norm())
        worst = max(worst, err)
        assert err < 2e-4, (k, err)
    print(f"zero_b {zero_b}: worst adapter gradient error {worst:.3e}")


def test_audio_branch_fp32_training_step_of_a_lora_model_vs_double_autograd(ops):
    from conftest import mid_audio_psd_case
    from oracle import tasu_oracle as O
    from ps_slm_amd.lora import LoraConfig
    from ps_slm_amd.synthetic import random_lora_state_dict
    from ps_slm_amd.train_fp32 import forward_train_fp32
    geo, sd, batch, z = mid_audio_psd_case()
    cfg = LoraConfig(r=8, lora_alpha=16, lora_dropout=0.0)
    lsd = random_lora_state_dict(geo, cfg, 31, b_scale=0.05)
    gm = lora_model(geo, cfg, sd, lsd, ops)
    st = gm.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"],
                          batch["input_feature_length"], fp32=True)
    assert np.array_equal(st.dev["psd_lens"], z["psd_lens"])
    forward_train_fp32(gm, st)
    gm.run_backward(st)
    torch.cuda.synchronize()
    loss, ref = double_adapter_grads(sd, lsd, cfg, geo, batch, audio=True)
    got = float(st.dev["loss_out"][0])
    print(f"audio lora: loss {got:.7f} float64 {loss:.7f}")
    assert abs(got - loss) <= 2e-5 * max(1.0, abs(loss))
    gg = gm.lora_grads()
    assert set(gg) == set(ref)
    for k, r in ref.items():
        err = float((gg[k].cpu().double() - r).norm() / r.norm())
        assert err < 2e-4, (k, err)
    from fp32_oracle_cases import lora_merged_double
    W = lora_merged_double(sd, lsd, cfg)
    _, pg = O.loss_and_projector_grads(W, dict(batch, input_features=batch["input_features"].double()), dataclasses.asdict(geo),
                                       mode="fp32", audio=True)
    for k, g in gm.projector_grads().items():
        err = float((g.cpu().double() - pg[k]).norm() / pg[k].norm())
        assert err < 2e-4, (k, err)


def test_lora_dropout_kernel_and_rank_products_vs_double(ops):
    """tasu_f32_lora_dropout: the mask bit for bit oracle.lora_oracle.lora_keep_mask, values exact (x / (1 - p) or 0), the
    accumulate mode; the thin products of the adapters on tasu_f32_gemm_nt (r = 8, 16, 64; the accumulate y += us B^T as ``resid``
    aliasing C on a column slice) within 2e-5 of float64."""
    from oracle.lora_oracle import lora_keep_mask
    M, C, p, sid = 37, 192, 0.25, 19
    rng = torch.tensor([20260101, 5], dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(8)
    x = torch.randn(M, C, generator=g, device="cuda") + 3.0        # no zeros: the kept set is visible in the output
    out = torch.full((M, C), 9.0, device="cuda")
    ops.f32_lora_dropout(x, out, M, C, p, rng, sid)
    keep = torch.from_numpy(lora_keep_mask(20260101, 5, sid, M * C, p)).view(M, C)
    assert torch.equal((out != 0).cpu(), keep) and 0.7 < float(keep.float().mean()) < 0.8
    ref = torch.where(keep, x.cpu().double() / (1.0 - float(np.float32(p))), torch.zeros((), dtype=torch.float64))
    assert float((out.cpu().double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    acc = torch.ones(M, C, device="cuda")
    ops.f32_lora_dropout(x, acc, M, C, p, rng, sid, accumulate=True)
    assert float((acc.cpu().double() - (1.0 + ref)).abs().max()) <= 1e-6 * float(ref.abs().max())
    ops.f32_lora_dropout(x, out, M, C, 0.0, rng, sid)
    assert torch.equal(out, x)
    for r in (8, 16, 64):
        rk, N, K = (r + 31) // 32 * 32, 320, 256
        xx, A = torch.randn(M, K, generator=g, device="cuda"), torch.randn(r, K, generator=g, device="cuda")
        Bp = torch.zeros(N, rk, device="cuda")
        Bp[:, :r] = torch.randn(N, r, generator=g, device="cuda")
        us = torch.zeros(M, rk, device="cuda")
        ops.f32_gemm(xx, A, us, M, r, K)
        ref_us = xx.double() @ A.double().t()
        assert float((us[:, :r].double() - ref_us).abs().max()) <= 2e-5 * float(ref_us.abs().max()) and not bool(us[:, r:].any())
        y = torch.randn(M, 2 * N, generator=g, device="cuda")
        want = y.double().clone()
        want[:, N:] += us[:, :r].double() @ Bp[:, :r].double().t()
        ops.f32_gemm(us, Bp, y[:, N:], M, N, rk, resid=y[:, N:])
        assert float((y.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())
        assert torch.equal(y[:, :N].double(), want[:, :N])


# ------------------------------------------------------------------------------------------ 2. the kernels
def ca_grad_double(q, table, dout, H):
    """dq of projector.py:111-126 by float64 autograd."""
    qd = q.double().requires_grad_(True)
    out = ca_double(qd, table, H)
    return torch.autograd.grad(out, qd, dout.double())[0], out.detach()


@pytest.mark.parametrize("dh", [64, 192, 448])
@pytest.mark.parametrize("V", [1000, 151936])
def test_ca_attn_bwd_kernel_vs_double_autograd(ops, dh, V):
    """Bar: max error per head <= 2e-5 of that head's gradient scale, the bar of test_gpu_fp32_ops.py::test_attention_backward_fp32
    (max |error| / max |gradient|).  The head's gradient scale is the largest |dq| of the head over the rows of the three calls
    (R = 1, 37, 300: one table, one query distribution), not of each call on its own: the R = 1 call consists of ONE near-one-hot
    row, whose float64 gradient is P (1 - P) ~ 1e-8 .. 1e-11 of an ordinary row's -- below the rounding of dP - delta, a difference of
    two fp32 numbers of size sqrt(dh), in any fp32 evaluation (the reference's own fp32 autograd included); the same rows inside
    the R = 37 and R = 300 calls are held to the bar in exactly this way.  Every call's figure is printed against both scales."""
    H = 8
    D = H * dh
    g = torch.Generator(device="cuda").manual_seed(dh * 11 + V)
    table = torch.randn(V, D, generator=g, device="cuda")
    runs = []
    for R in (1, 37, 300):
        q = torch.randn(R, D, generator=g, device="cuda") * 0.15
        for r in range(0, R, 3):                                    # near-one-hot rows, as the forward's test builds them
            v = int(torch.randint(0, V, (1,), generator=g, device="cuda"))
            q[r] = table[v] * (40.0 / dh ** 0.5)
        dout = torch.randn(R, D, generator=g, device="cuda")
        plain = torch.empty(R, D, device="cuda")
        ops.f32_ca_attn(q, table, plain, R, H)
        out, lse = torch.full((R, D), 7.0, device="cuda"), torch.empty(R, H, device="cuda")
        ops.f32_ca_attn_lse(q, table, out, lse, R, H)
        dq = torch.full((R, D), 5.0, device="cuda")
        ops.f32_ca_attn_bwd(q, table, out, dout, lse, dq, R, H)
        torch.cuda.synchronize()
        assert torch.equal(out, plain)                              # the lse-emitting forward: the same bits
        ref, _ = ca_grad_double(q, table, dout, H)
        ref_lse = (torch.einsum("rhd,vhd->rhv", q.double().view(R, H, dh), table.double().view(V, H, dh)) / dh ** 0.5).logsumexp(-1)
        assert float((lse.double() - ref_lse).abs().max()) < 2e-5 * float(ref_lse.abs().max())
        again = torch.empty_like(dq)
        ops.f32_ca_attn_bwd(q, table, out, dout, lse, again, R, H)
        torch.cuda.synchronize()
        assert torch.equal(dq, again)                               # a second run: the same bits
        runs.append((R, (dq.double() - ref).abs().view(R, H, dh).amax(dim=(0, 2)), ref.abs().view(R, H, dh).amax(dim=(0, 2))))
    scale = torch.stack([s for _, _, s in runs]).amax(0)
    for R, err, own in runs:
        print(f"dh {dh} V {V} R {R}: max error per head / head's gradient scale {(err / scale).max().item():.3e} "
              f"(/ the call's own largest gradient {(err / own).max().item():.3e})")
    for R, err, own in runs:
        assert bool((err <= 2e-5 * scale).all()), (dh, V, R, (err / scale).max().item())


def test_ca_attn_bwd_rejects_bad_arguments_and_leaves_dq_untouched(ops):
    from ps_slm_amd._lib import load
    lib = load()
    V, H, dh, R = 1000, 8, 64, 5
    D = H * dh
    q, table, dout = torch.randn(R, D, device="cuda"), torch.randn(V, D, device="cuda"), torch.randn(R, D, device="cuda")
    out, lse = torch.empty(R, D, device="cuda"), torch.full((R, H), 3.0, device="cuda")
    dq = torch.full((R, D), 3.0, device="cuda")
    n = lib.tasu_f32_ca_workspace_floats(R, V, D, H)
    ws = torch.empty(n, device="cuda")
    den = float(dh) ** 0.5
    fwd = [q.data_ptr(), D, table.data_ptr(), V, D, H, den, out.data_ptr(), D, lse.data_ptr(), R, ws.data_ptr(), n, None]
    for over in ({9: None}, {0: None}, {12: n - 1}, {5: 7}):       # no lse, no q, workspace too small, D % H
        args = list(fwd)
        for k, v in over.items():
            args[k] = v
        assert lib.tasu_f32_ca_attn_lse(*args) == 1, over
    torch.cuda.synchronize()
    assert bool((lse == 3.0).all())
    assert lib.tasu_f32_ca_attn_lse(*fwd) == 0
    good = [q.data_ptr(), D, table.data_ptr(), V, D, H, den, out.data_ptr(), D, dout.data_ptr(), D, lse.data_ptr(), dq.data_ptr(), D, R,
            ws.data_ptr(), n, None]
    bad = [{0: None}, {2: None}, {7: None}, {9: None}, {11: None}, {12: None}, {15: None},     # null operands
           {1: D - 4}, {8: D - 1}, {10: D - 4}, {13: D - 1}, {1: D + 2}, {10: D + 2},          # pitches < D, or not a multiple of 4
           {16: n - 1},                                                                        # workspace too small
           {4: 8 * 20, 1: 160, 8: 160, 10: 160, 13: 160},                                      # dh = 20: not a multiple of 16
           {4: 8 * 528, 1: 8 * 528, 8: 8 * 528, 10: 8 * 528, 13: 8 * 528},                     # dh = 528 > 512
           {5: 7}, {14: 0}, {3: 0}, {6: 0.0}]                                                  # D % H, R, V, denom
    for over in bad:
        args = list(good)
        for k, v in over.items():
            args[k] = v
        assert lib.tasu_f32_ca_attn_bwd(*args) == 1, over
    torch.cuda.synchronize()
    assert bool((dq == 3.0).all())
    assert lib.tasu_f32_ca_attn_bwd(*good) == 0
    torch.cuda.synchronize()
    assert not bool((dq == 3.0).any())


def test_relu_bwd_kernel_vs_double(ops):
    """dx = dy where the ReLU passed: exact in any precision (a selection), from the ReLU's input or from its output; in place."""
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(37, 1000, generator=g, device="cuda")
    x[0, :7] = 0.0                                                  # relu'(0) = 0 (torch's convention)
    dy = torch.randn(37, 1000, generator=g, device="cuda")
    xd = x.double().requires_grad_(True)
    ref = torch.autograd.grad(torch.relu(xd), xd, dy.double())[0]
    out = torch.full_like(x, 9.0)
    ops.f32_relu_bwd(x, dy, out)
    assert float((out.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) and torch.equal(out.double(), ref)
    ops.f32_relu_bwd(torch.relu(x), dy, out)
    assert torch.equal(out.double(), ref)
    dy2 = dy.clone()
    ops.f32_relu_bwd(x, dy2, dy2)
    assert torch.equal(dy2.double(), ref)


# ------------------------------------------------------------------------------------------ 3. audio branch
def test_audio_branch_fp32_training_step_of_cov1d_vs_double_autograd(ops):
    """A k = 2 cov1d-linear model on the mid_audio_psd inputs (fp32 encoder -> CTC softmax -> PSD -> projector -> decoder), built as
    test_audio_branch_eval_forward_in_fp32_vs_the_double_oracle builds it: loss within 2e-5 and every projector gradient within 2e-4
    relative L2 of float64 autograd through oracle.forward_audio; the same PSD lengths."""
    from conftest import mid_audio_psd_case
    from oracle import tasu_oracle as O
    from ps_slm_amd.synthetic import random_state_dict
    from ps_slm_amd.train_fp32 import forward_train_fp32
    geo, sd, batch, z = mid_audio_psd_case()
    geo = dataclasses.replace(geo, projector="cov1d-linear", projector_ds_rate=2, bottleneck=2048)
    sd = {n: v for n, v in sd.items() if not n.startswith("encoder_projector.")}
    sd.update({n: v for n, v in random_state_dict(geo, 91, with_encoder=False).items() if n.startswith("encoder_projector.")})
    gm = f32_model(geo, sd, ops)
    st = gm.prepare_audio(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["input_features"],
                          batch["input_feature_length"], fp32=True)
    assert np.array_equal(st.dev["psd_lens"], z["psd_lens"])
    forward_train_fp32(gm, st)
    gm.run_backward(st)
    torch.cuda.synchronize()
    W = {k: v.double() for k, v in sd.items()}
    ref, grads = O.loss_and_projector_grads(W, dict(batch, input_features=batch["input_features"].double()), dataclasses.asdict(geo),
                                            mode="fp32", audio=True)
    loss, ref_loss = float(st.dev["loss_out"][0]), float(ref["loss"].detach())
    print(f"audio cov1d k2: loss {loss:.7f} float64 {ref_loss:.7f}")
    assert abs(loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss))
    gg = gm.projector_grads()
    assert set(gg) == set(grads) and len(gg) == 6
    for k, r in grads.items():
        err = float((gg[k].cpu().double() - r).norm() / r.norm())
        print(f"{k}: relative L2 {err:.3e}")
        assert err < 2e-4, (k, err)


# ------------------------------------------------------------------------------------------ 4. selection and engine
def _factory(projector, use_peft=False, fp16=False, mixed=True, posterior=True):
    from ps_slm_amd.config import ModelConfig, TrainConfig
    from ps_slm_amd.ps_slm import model_factory
    kw = dict(peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0)) if use_peft else {}
    tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=posterior, gt_emb_noise=False, ctc_posterior=posterior, do_psd=True,
                     use_fp16=fp16, mixed_precision=mixed, use_peft=use_peft, **kw)
    extra = dict(encoder_projector_ds_rate=2) if projector in ("linear", "cov1d-linear") else {}
    mc = ModelConfig(llm_path="synthetic:mid", encoder_projector=projector, llm_dim=256, **extra)
    return model_factory(tc, mc, device="cuda:0", init_seed=77)


def _call(core):
    from ps_slm_amd.synthetic import synthetic_text_batch
    raw = synthetic_text_batch(core.geo, 2, seed=5, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=8, noise=False)
    return dict(input_ids=raw["input_ids"], attention_mask=raw["attention_mask"], labels=raw["labels"], input_features=None,
                input_feature_length=None, GT=[" ".join(map(str, p)) for p in raw["post_ids"]])


@pytest.mark.parametrize("projector", ["linear", "cov1d-linear", "cross-attention"])
def test_mixed_precision_false_selects_the_fp32_training_step(projector):
    """synthetic:mid at llm_dim 256 has cross-attention heads of 32 columns: a multiple of 16, served by the fp32 kernels."""
    model, _ = _factory(projector, mixed=False)
    core = model.core
    assert core.arith == "fp32" and core.arith_train == "fp32"
    model.train()
    out, _ = model(**_call(core))
    out.loss.backward()
    torch.cuda.synchronize()
    assert model.last_state.fp32
    g = core.proj.g.clone()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # the eval forward of the same model is the same fp32 arithmetic: the two losses agree to fp32 rounding
    model.eval()
    ev, _ = model(**_call(core))
    assert abs(float(ev.loss) - float(out.loss.detach())) <= 2e-5 * max(1.0, abs(float(ev.loss)))
    # mixed_precision = true (the default) and use_fp16 = true: what they are today
    for kw, arith, train in ((dict(mixed=True), "fp32", "bf16"), (dict(fp16=True, mixed=False), "bf16", "bf16")):
        other, _ = _factory(projector, **kw)
        assert (other.core.arith, other.core.arith_train) == (arith, train)
        if projector != "cross-attention":                          # (the bf16 cross-attention step needs heads of 64 columns)
            other.train()
            o2, _ = other(**_call(other.core))
            o2.loss.backward()
            torch.cuda.synchronize()
            assert not getattr(other.last_state, "fp32", False)


def test_mixed_precision_false_refuses_recipes_without_an_fp32_step():
    with pytest.raises(NotImplementedError, match="ctc_posterior=false"):
        _factory("linear", mixed=False, posterior=False)
    model, _ = _factory("linear-silu", mixed=False)                 # the shipped recipe: served before, served now
    assert model.core.arith_train == "fp32"


def test_engine_step_on_the_fp32_training_step_of_an_alternate_projector():
    """TasuEngine.backward() / step() route through TasuModel.run_backward: one optimizer step moves the projector, and the next
    fp32 eval forward equals that of a fresh model loaded from the stepped model's state_dict(), loss bit-equal."""
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    model, _ = _factory("cov1d-linear", mixed=False)
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg["lr"] = 1e-3
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10                                             # past DeepSpeed's two zero-lr steps
    call = _call(model.core)
    before = model.core.proj.p.clone()
    model.train()
    out, _ = eng(**call)
    eng.backward(out.loss)
    eng.step()
    torch.cuda.synchronize()
    assert model.last_state.fp32 and not torch.equal(model.core.proj.p, before)
    model.eval()
    l1 = model(**call)[0].loss.detach().cpu().clone()
    fresh, _ = _factory("cov1d-linear", mixed=False)
    fresh.load_state_dict(model.state_dict(), strict=False)
    fresh.eval()
    l2 = fresh(**call)[0].loss.detach().cpu().clone()
    assert torch.equal(l1, l2)


@pytest.mark.parametrize("frozen", [False, True])
def test_lora_model_through_the_plugin_and_engine_on_the_fp32_step(frozen):
    """use_fp16 = false, mixed_precision = false, use_peft = true: outputs.loss.backward() runs the fp32 step; one TasuEngine step
    changes the adapters, and the next eval forward equals that of a fresh model loaded from the stepped model's state_dict(), loss
    bit-equal (the merged fp32 weights were rebuilt).  freeze_projector = true: the projector's part of the bucket is not touched."""
    from ps_slm_amd.config import DEFAULT_DS_CONFIG, ModelConfig, TrainConfig, load_ds_config
    from ps_slm_amd.engine import TasuEngine
    from ps_slm_amd.ps_slm import model_factory
    from ps_slm_amd.synthetic import random_lora_state_dict

    def make():
        tc = TrainConfig(freeze_llm=True, freeze_encoder=True, gt_emb=True, gt_emb_noise=False, ctc_posterior=True, do_psd=True,
                         use_fp16=False, mixed_precision=False, use_peft=True, freeze_projector=frozen,
                         peft_config=dict(r=8, lora_alpha=16, lora_dropout=0.0))
        mc = ModelConfig(llm_path="synthetic:mid", encoder_projector="linear-silu", llm_dim=256)
        return model_factory(tc, mc, device="cuda:0", init_seed=77)[0]

    model = make()
    core = model.core
    assert core.arith == "fp32" and core.arith_train == "fp32" and core.freeze_projector == frozen
    core.lora.load_state_dict(random_lora_state_dict(core.geo, core.lora.cfg, 5, b_scale=0.05))
    core.sync_projector_copies()
    call = _call(core)
    model.train()
    core.proj.g.fill_(3.0)
    out, _ = model(**call)
    out.loss.backward()
    torch.cuda.synchronize()
    assert model.last_state.fp32
    base = core.lora.base
    assert bool(torch.isfinite(core.proj.g).all()) and not bool((core.proj.g[base:] == 3.0).all())
    assert bool((core.proj.g[:base] == 3.0).all()) == frozen
    cfg = load_ds_config(DEFAULT_DS_CONFIG)
    cfg["lr"] = 1e-3
    eng = TasuEngine(model, cfg)
    eng.sched_iter = 10
    model.eval()
    l0 = model(**call)[0].loss.detach().cpu().clone()              # (the merged fp32 weights exist before the step)
    model.train()
    before = core.proj.p.clone()
    out, _ = eng(**call)
    eng.backward(out.loss)
    eng.step()
    torch.cuda.synchronize()
    assert not torch.equal(core.proj.p[base:], before[base:]) and torch.equal(core.proj.p[:base], before[:base]) == frozen
    model.eval()
    l1 = model(**call)[0].loss.detach().cpu().clone()
    fresh = make()
    fresh.load_state_dict(model.state_dict(), strict=False)
    fresh.eval()
    l2 = fresh(**call)[0].loss.detach().cpu().clone()
    assert torch.equal(l1, l2) and not torch.equal(l0, l1)
