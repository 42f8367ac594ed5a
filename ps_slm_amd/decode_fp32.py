"""fp32 arithmetic mode of ``slam_model_asr.generate`` (``train_config.use_fp16 = false``).

The reference decodes WITHOUT autocast on fp32 weights (Multitask/inference_batch.py:113-117,146: the model is built in fp32,
``model.eval()``, ``model.generate(**batch)``; Multitask/model/ps-slm.py:660-675 -> HF ``generate(inputs_embeds=..., num_beams=4)``),
so its tokens are those of an fp32 forward pass.  The bf16 path (ps_slm_amd/decode.py) reproduces them only where rounding cannot
matter; this path computes what the reference computes: the fp32 projector on the master weights (project_fp32: linear-silu,
linear, cov1d-linear, and cross-attention through the fused tasu_f32_ca_attn over the input embedding table), fp32 embeddings and
residual stream, fp32 q|k|v / RoPE / attention / MLP on fp32 copies of the frozen Qwen2 weights (with use_peft: the merged
W + s B A of ps_slm_amd.lora.merged_llm_f32, one accessor, weights_f32), an fp32 KV cache, fp32 logits, log-softmax and top-k -- csrc/fp32.hip through the C-ABI (``tasu_f32_*``).  prompt_pass_fp32
is the only fp32 decoder forward: the eval forward, generate()'s prefill and, with its activations kept, the fp32 training step
(ps_slm_amd/train_fp32.py) run it, and its layer, _layer_fp32, is the only fp32 decoder layer (the decode step's as well; an adapted
training step hands it the adapter runner: the dependency runs one way, train_fp32 -> this module).  The beam search itself is the
same device-side bookkeeping as the bf16 path's (``tasu_beam_update``, the cache row index, ``DeviceBeam``), and a generated
position is one hipGraph replay.  Nothing is rounded to bf16; sums run in another order than the reference's CPU BLAS (fp32 MFMA,
K ascending, K-range slabs added in ascending order: deterministic).  The audio branch runs the frozen SenseVoice encoder, the CTC
softmax and PSD in fp32 as well (ps_slm_amd/encoder.py: encoder_posterior_fp32; TasuModel.prepare_audio takes it when
``arith == "fp32"`` and no labels are given).  Pinned by exact token equality with the REAL reference on 24 unfiltered random cases,
the 17 rounding-stable ones and the text + audio fixture (tests/test_gpu_model.py).

A Qwen3 decoder (``geo.qk_norm``: an RMSNorm over each 128-wide q and k head between the projection and the rotation, no q|k|v bias)
takes ``tasu_f32_gemm_qkv_norm_rope`` where a Qwen2 layer takes ``tasu_f32_gemm_qkv_rope`` -- HF's Qwen3RMSNorm on fp32 tensors, in the
launch that sums the projection's K-range slabs (csrc/qk_norm.hip, csrc/fp32.hip) -- and is otherwise the same path.

HBM-bound like the bf16 step, on twice the bytes: 6.2 GB of fp32 weights per generated position at Qwen2.5-1.5B.
"""
from types import SimpleNamespace

import numpy as np
import torch

from .decode import DeviceBeam, decode_positions, generate_args, kv_row_index, penalty_mode, prompt_rows
from .model import HD, StepState, rup

F32_MAX_CTX = 2048          # tasu_f32_attn_*: keys per query row


def _gemm_ws(model):
    """The fp32 GEMMs' slab workspace: 16 K-range slabs of the widest narrow projection, or the lm_head's two slabs at 64 beam rows
    (csrc/fp32.hip f32_stream_plan: a problem whose slabs do not fit runs unsplit on the tile kernel).  EVERY fp32 caller (decode,
    eval forward, training step, fp32 encoder) takes it from here: the K-split plans depend on its size, so one size from the first
    fp32 call on keeps a product's bits, and the captured graphs, independent of which fp32 path ran first."""
    return model._buf("f32_gemm_ws", (max(16 * 128 * 4096, 2 * 64 * model.geo.llm_vocab),), torch.float32)


def _fragments(model):
    """Fragment-order copies of the matrices the decode step STREAMS (gate|up, down, lm_head: csrc/fp32.hip f32_stream_kernel reads
    1 KiB per wave instruction from them instead of 16 rows x 64 B), made at the first generate(): +5.3 GB at Qwen2.5-1.5B.
    ``TASU_F32_FRAGMENTS=0``: A/B runs on the row-major matrices (the same bits)."""
    import os
    if os.environ.get("TASU_F32_FRAGMENTS", "1") == "0" or not hasattr(model.ops, "f32_to_fragments"):
        return None
    f32 = weights_f32(model)
    fr = f32.get("frag")
    if fr is None or fr.get("head") is None:               # (head None: the tied embedding table changed, the layers' copies stand)
        ops, nws = model.ops, _gemm_ws(model).numel()

        def to(w):                                         # only what the streaming kernel will read (Qwen2.5-7B's down projection,
            N, K = w.shape                                 # K = 18944, has no K slice it serves: no copy)
            return ops.f32_to_fragments(w) if ops.lib.tasu_f32_gemm_streams(64, N, K, nws) == 1 else w
        # a merged LoRA set shares the base lm_head: its fragment copy is the base set's, or the one kept across adapter updates
        base_fr = model.llm.f32.get("frag") if f32 is not model.llm.f32 else None
        head = base_fr["head"] if base_fr is not None and base_fr.get("head") is not None else f32.get("frag_head")
        if head is None:
            head = f32["frag_head"] = to(f32["head"])
        if fr is None:
            fr = f32["frag"] = dict(layers=[dict(wgu=to(f["wgu"]), wd=to(f["wd"])) for f in f32["layers"]])
        fr["head"] = head
    return fr


def project_fp32(model, st: StepState, keep=None):
    """The projector in fp32 on the master weights (``pr.view(pr.p, ...)``, the layout of the bf16 images): st.dev['y2_f32'] [Rap, D].
    linear-silu (EncoderProjectorLinearSiLU, Multitask/model/projector.py:128-151): LayerNorm -> Linear -> SiLU -> Linear;
    linear (EncoderProjectorConcat, :28-49): k consecutive frames as one row -> Linear -> ReLU -> Linear;
    cov1d-linear (EncoderProjectorCov1d, :53-73): Conv1d(kernel = stride = k) as one GEMM over the k-frame rows -> ReLU -> Linear ->
    ReLU -> Linear;  cross-attention (EncoderProjectorCTCCA, :104-126): Q = W_q(post), then tasu_f32_ca_attn over the fp32 input
    embedding table.  ``keep`` (the training step): what backward_fp32 reads.  linear-silu: the LayerNorm statistics are written and
    the SiLU runs on its own after W1 (xn_p, mean, rstd, h_pre, h).  linear / cov1d-linear: the same launches as without ``keep`` --
    the k-frame rows, the conv's output c0 and h are kept AFTER their ReLU, whose output carries the mask of its input (y > 0 where
    x > 0).  cross-attention: q, the attention's output and its per-(row, head) log-sum-exp (tasu_f32_ca_attn_lse: the same
    ``out`` bits)."""
    ops, pr = model.ops, model.proj
    f32 = torch.float32
    Fap, Rap, K, Kp, Hb, Do = st.Fap, st.Rap, pr.K, pr.Kp, pr.Hb, pr.Do
    if "post" not in st.dev:                                   # text branch: the pseudo-posterior rows (ps-slm.py:337-358)
        post = model._buf("post", (Fap, Kp), f32)
        ops.posterior_build(st.dev["post_ids"], st.dev["post_alpha"], post, Fap, K)
        st.dev["post"] = post
    ws = _gemm_ws(model)
    y2 = model._buf("f32_proj_y2", (Rap, Do), f32)
    if pr.is_ca:
        geo = model.geo
        q = model._buf("f32_ca_q", (Rap, Do), f32)
        ops.f32_gemm(st.dev["post"], pr.view(pr.p, "W_q.weight"), q, Rap, Do, Kp, ws=ws)
        cws = model._buf("f32_ca_ws", (ops.f32_ca_workspace_floats(Rap, geo.llm_vocab, Do, geo.ca_heads),), f32)
        if keep is None:
            ops.f32_ca_attn(q, model.llm.embed, y2, Rap, geo.ca_heads, ws=cws)
        else:
            lse = model._buf("f32t_ca_lse", (Rap, geo.ca_heads), f32)
            ops.f32_ca_attn_lse(q, model.llm.embed, y2, lse, Rap, geo.ca_heads, ws=cws)
            keep.update(q=q, lse=lse, out=y2, ca_ws=cws)
        st.dev["y2_f32"] = y2
        return y2
    if pr.has_norm:
        x = model._buf("f32_proj_xn", (Fap, Kp), f32)
        mean, rstd = (None, None) if keep is None else (model._buf("ln_mean", (Fap,), f32), model._buf("ln_rstd", (Fap,), f32))
        ops.layernorm_fwd(st.dev["post"], pr.view(pr.p, "norm.weight"), pr.view(pr.p, "norm.bias"), x, mean, rstd, Fap, K, model.geo.ln_eps)
    else:
        x = st.dev["post"]                                     # linear / cov1d-linear: the posterior as it is
    x = x.view(Rap, pr.k * Kp)                                 # k consecutive frames = one projector row (k = 1: linear-silu)
    if pr.has_conv:
        c0 = model._buf("f32_proj_c0", (Rap, Kp), f32)
        ops.f32_gemm(x, pr.view(pr.p, "conv1d.weight"), c0, Rap, Kp, pr.k * Kp, bias=pr.view(pr.p, "conv1d.bias"), act=2, ws=ws)
        x = c0
    h = model._buf("f32_proj_h", (Rap, Hb), f32)
    if keep is not None and not pr.has_norm:
        keep.update(xcat=st.dev["post"].view(Rap, pr.k * Kp), x1=x, h=h)
    if keep is None or not pr.has_norm:
        ops.f32_gemm(x, pr.view(pr.p, pr.n_w1), h, Rap, Hb, pr.kin * Kp, bias=pr.view(pr.p, pr.n_b1), act=1 if pr.has_norm else 2, ws=ws)
    else:
        h_pre = model._buf("f32t_h_pre", (Rap, Hb), f32)
        ops.f32_gemm(x, pr.view(pr.p, pr.n_w1), h_pre, Rap, Hb, pr.kin * Kp, bias=pr.view(pr.p, pr.n_b1), ws=ws)
        ops.f32_silu(h_pre, h)
        keep.update(xn_p=x, mean=mean, rstd=rstd, h_pre=h_pre, h=h)
    ops.f32_gemm(h, pr.view(pr.p, pr.n_w2), y2, Rap, Do, Hb, bias=pr.view(pr.p, pr.n_b2), ws=ws)
    st.dev["y2_f32"] = y2
    return y2


def weights_f32(model):
    """The fp32 weight set of the decoder, {"layers": [{wqkv, bqkv, wo, wgu, wd}], "head"}: the frozen copies, or -- use_peft -- the
    merged W + s B A of ps_slm_amd.lora.merged_llm_f32 (rebuilt when the adapters changed)."""
    if model.lora is not None:
        from .lora import merged_llm_f32
        return merged_llm_f32(model)
    return model.llm.f32


def _layer_fp32(model, l, b, attend, lo=None, drop=False, cache=None, ctx=0, frag=None):
    """One decoder layer, the only fp32 one.  ``b``, the buffers: in b.xn = RMSNorm(b.x_in, ln1[l]); out b.x_mid = x_in + attention,
    b.x_out = x_mid + MLP, b.xn = the NEXT norm of x_out (ln1[l + 1], or the final norm); b.qkv, b.ao, b.gu, b.act, b.cos, b.sin, b.ws
    and b.rows.  Decode and eval hand in one buffer three times; the training step hands in its kept slices and sets b.keep, with
    b.qk = (pre, rstd) on a qk_norm geometry (Qwen3): the plain projection and the heads' rstd, which the head norm's backward reads.
    Every Linear has one branch.  Where nothing stands between the projection and the row-wise kernel behind it, both are the ONE
    launch that sums the GEMM's K-range slabs (tasu_f32_gemm_qkv_rope or, with the per-head q/k RMSNorm in front of the rotation,
    _qkv_norm_rope; _resid_rmsnorm; _swiglu): 9 launches per layer at <= 64 beam rows instead of 13.  Else: base GEMM -> the adapters'
    branches -> the row operator.  What stands between is a tensor kept for the backward (gate|up; pre) or ``lo``, the adapter
    runner of the training step (train_fp32.LoraF32): training runs the adapters unmerged, y = W x + s B (A drop(x)), so with ``lo``
    the layer reads the BASE fp32 weights and EVERY Linear is unfused, those of a group without an adapted member too."""
    ops, geo, llm = model.ops, model.geo, model.llm
    D, I, H, G, L = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_layers
    f, w = (llm.f32 if lo is not None else weights_f32(model))["layers"][l], llm.layers[l]
    next_norm = llm.layers[l + 1]["ln1"] if l + 1 < L else llm.norm
    xn, qkv, act, rows, ws, eps, keep = b.xn, b.qkv, b.act, b.rows, b.ws, geo.rms_eps, b.keep
    kv = dict(zip(("kc", "vc", "slot"), cache or (None, None, None)), ctx=ctx)

    def linear(g, x, wt, y, N, K, **kw):                   # the unfused form
        ops.f32_gemm(x, wt, y, rows, N, K, **kw, ws=ws)
        if lo is not None:
            lo.forward(l, g, x, y, rows, ws, drop)

    if geo.qk_norm and (keep or lo is not None):
        linear("qkv", xn, f["wqkv"], b.qk[0], (H + 2 * G) * HD, D)
        ops.f32_qk_norm_rope(b.qk[0], f["q_norm"], f["k_norm"], b.cos, b.sin, qkv, b.qk[1], rows, H, G, eps, **kv)
    elif geo.qk_norm:
        ops.f32_gemm_qkv_norm_rope(xn, f["wqkv"], None, qkv, f["q_norm"], f["k_norm"], b.cos, b.sin, rows, H, G, D, eps, ws, **kv)
    elif lo is not None:                                   # (the training step: no cache to fill)
        linear("qkv", xn, f["wqkv"], qkv, (H + 2 * G) * HD, D, bias=f["bqkv"])
        ops.f32_rope(qkv, b.cos, b.sin, rows, H, G)
    else:
        ops.f32_gemm_qkv_rope(xn, f["wqkv"], f["bqkv"], qkv, b.cos, b.sin, rows, H, G, D, ws, **kv)
    attend(l, qkv, b.ao)
    if lo is None:
        ops.f32_gemm_resid_rmsnorm(b.ao, f["wo"], b.x_mid, w["ln2"], xn, rows, D, H * HD, eps, ws, resid=b.x_in)
    else:
        linear("o", b.ao, f["wo"], b.x_mid, D, H * HD, resid=b.x_in)
        ops.f32_rmsnorm(b.x_mid, w["ln2"], xn, rows, D, eps)
    wgu, wd = (f["wgu"], f["wd"]) if frag is None else (ops.f32_weight(frag["layers"][l]["wgu"], rows, ws), ops.f32_weight(frag["layers"][l]["wd"], rows, ws))
    if lo is None and not keep:
        ops.f32_gemm_swiglu(xn, wgu, b.gu, act, rows, I, D, ws)
    else:
        linear("gu", xn, wgu, b.gu, 2 * I, D)
        ops.f32_swiglu(b.gu, act, rows, I)
    if lo is None:
        ops.f32_gemm_resid_rmsnorm(act, wd, b.x_out, next_norm, xn, rows, D, I, eps, ws, resid=b.x_mid)
    else:
        linear("down", act, wd, b.x_out, D, I, resid=b.x_mid)
        ops.f32_rmsnorm(b.x_out, next_norm, xn, rows, D, eps)


def _need_f32(model):
    if not getattr(model.llm, "f32", None):
        raise RuntimeError("the fp32 path needs the fp32 copies of the LLM weights: build the model with train_config.use_fp16=false "
                           "(model_factory sets LLMWeights.keep_f32 before loading)")


def prompt_pass_fp32(model, st: StepState, on_layer=None, keep=None, lo=None, drop=False):
    """The decoder over the merged prompt in fp32, the one fp32 decoder forward of the eval forward, generate()'s prefill and the
    training step: projector -> embedding merge -> 28 layers (causal attention; a batch's padding is on one side: left-padded
    prompts mask their first ``S - valid`` keys, right-padded training batches need no key mask under the causal one -- their padded
    QUERY rows hold garbage nobody reads).  ``on_layer(l, qkv)``: called with the layer's rotated q|k|v (generate() fills its cache
    there).  ``keep`` (a dict: the training step): every layer's activations go to stacked buffers -- layer l reads xs[2l] and
    writes xs[2l + 1] and xs[2l + 2] -- gate|up runs unfused, and ``keep`` receives what backward_fp32 reads (xs, qkvs, aos, gus,
    cos, sin, kstart and the projector's, project_fp32; on a qk_norm geometry also qkv_pres and qk_rstds, the plain projections and
    the heads' rstd).  ``lo``, ``drop`` (the training step of an adapted decoder, from forward_train_fp32): the adapter runner every
    layer gets, and whether this step draws dropout masks.  Returns (xn0 = the final-normed hidden states [B * S, D], valid, left)."""
    ops, geo, llm = model.ops, model.geo, model.llm
    _need_f32(model)
    B, S = st.B, st.S
    if S > F32_MAX_CTX:
        raise ValueError(f"sequence length {S} exceeds the fp32 attention's limit {F32_MAX_CTX}")
    km = np.asarray(st.plan.key_mask)[:, :S].astype(bool)
    valid = km.sum(1).astype(np.int64)
    left = all(km[b, S - valid[b]:].all() for b in range(B))
    right = all(km[b, :valid[b]].all() for b in range(B))
    if not (left or right):
        raise ValueError("the fp32 path expects every row's padding on one side (left: inference collator, right: training collator)")
    M0 = B * S
    D, I, H, G, L = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_layers
    LDQ = (H + 2 * G) * HD
    scale = HD ** -0.5
    f32 = torch.float32
    buf, d = model._buf, st.dev
    ws = _gemm_ws(model)
    y2 = project_fp32(model, st, keep)
    kstart_b = model._upload("f32_kstart_b", ((S - valid) if left else np.zeros(B, dtype=np.int64)).astype(np.int32))
    if keep is None:                       # one buffer per activation, rewritten by every layer
        x0 = buf("f32_x0", (M0, D), f32)
        xs, qkvs = [x0] * (2 * L + 1), [buf("f32_qkv0", (M0, LDQ), f32)] * L
        aos, gus = [buf("f32_ao0", (M0, H * HD), f32)] * L, [buf("f32_gu0", (M0, 2 * I), f32)] * L
    else:
        xs, qkvs = buf("f32t_xs", (2 * L + 1, M0, D), f32), buf("f32t_qkv", (L, M0, LDQ), f32)
        aos, gus = buf("f32t_ao", (L, M0, H * HD), f32), buf("f32t_gu", (L, M0, 2 * I), f32)
    # Qwen3's training step: every layer's plain projection and head rstd, what tasu_f32_qk_norm_bwd reads
    pres, rstds = (buf("f32t_qkv_pre", (L, M0, LDQ), f32), buf("f32t_qk_rstd", (L, M0, H + G), f32)) if keep is not None and geo.qk_norm else (None, None)
    ops.f32_embed_merge(llm.embed, y2, d["kind"], d["idx"], xs[0], M0, D)
    cos0, sin0 = buf("f32_cos0", (M0, HD // 2), f32), buf("f32_sin0", (M0, HD // 2), f32)
    ops.rope_table(d["pos"], cos0, sin0, HD, geo.rope_theta)
    xn0, act0 = buf("f32_xn0", (M0, D), f32), buf("f32_act0", (M0, I), f32)

    def attend_prompt(l, qkv, ao):
        if on_layer is not None:
            on_layer(l, qkv)
        ops.f32_attn_prefill(qkv, kstart_b, ao, B, S, H, G, scale)

    ops.f32_rmsnorm(xs[0], llm.layers[0]["ln1"], xn0, M0, D, geo.rms_eps)
    for l in range(L):
        b = SimpleNamespace(x_in=xs[2 * l], x_mid=xs[2 * l + 1], x_out=xs[2 * l + 2], xn=xn0, qkv=qkvs[l], ao=aos[l], gu=gus[l], act=act0,
                            rows=M0, cos=cos0, sin=sin0, ws=ws, keep=keep is not None, qk=(pres[l], rstds[l]) if pres is not None else None)
        _layer_fp32(model, l, b, attend_prompt, lo, drop)
    if keep is not None:
        keep.update(xs=xs, qkvs=qkvs, aos=aos, gus=gus, cos=cos0, sin=sin0, kstart=kstart_b)
        if pres is not None:
            keep.update(qkv_pres=pres, qk_rstds=rstds)
    return xn0, valid, left


def forward_fp32(model, st: StepState, compute_loss=True):
    """The eval-mode forward in the reference's fp32 arithmetic (``train_config.use_fp16 = false``: ``evaluation()`` of
    Multitask/utils/deepspeed_utils.py:394-498 and any ``model(**batch)`` outside autocast): fp32 logits for every position
    (``st.dev['logits']`` [B * S, V]), the shifted CE over the labelled rows and the token accuracy (``st.dev['loss_out']`` =
    [mean loss, accuracy, count, 1 / count]).  No activations are kept: there is no fp32 backward."""
    ops, geo = model.ops, model.geo
    xn0, _, _ = prompt_pass_fp32(model, st)
    M0, D, V = st.B * st.S, geo.llm_dim, geo.llm_vocab
    f32, i32 = torch.float32, torch.int32
    buf, d = model._buf, st.dev
    ws = _gemm_ws(model)
    logits = buf("f32_logits_all", (M0, V), f32)
    ops.f32_gemm(xn0, weights_f32(model)["head"], logits, M0, V, D, ws=ws)
    d.update(logits=logits)
    if not compute_loss:
        return
    row_loss, row_hit = buf("row_loss", (M0,), f32), buf("row_hit", (M0,), i32)
    row_arg, row_lse = buf("row_arg", (M0,), i32), buf("f32_row_lse", (M0,), f32)
    ops.f32_ce(logits, d["shift_labels"], M0, V, row_loss, row_hit, row_arg, row_lse)
    res = buf("loss_out", (4,), f32)
    ops.ce_reduce(row_loss, row_hit, d["shift_labels"], M0, res)
    d.update(loss_out=res, row_arg=row_arg, row_lse=row_lse)


def beam_search_generate_fp32(model, st: StepState, num_beams=4, max_new_tokens=200, min_length=1, length_penalty=1.0,
                              eos_token_id=None, pad_token_id=None, repetition_penalty=1.0, sampling=None):
    """st: a prepared state (prepare_text / prepare_audio); ``sampling`` as in decode.beam_search_generate.  Returns LongTensor
    [B, n_new] (CPU)."""
    ops, geo, llm = model.ops, model.geo, model.llm
    _need_f32(model)
    min_length, eos, pad = generate_args(model, st, num_beams, max_new_tokens, min_length, eos_token_id, pad_token_id, F32_MAX_CTX,
                                         "the fp32 attention's", repetition_penalty, kv_elem_bytes=4, kv_names=("f32_kc", "f32_vc"),
                                         sampling=sampling, sample_ops=("sample_uniform", "f32_sample_rows"),
                                         beam_sample_ops=("f32_beam_sample_rows", "beam_update_drawn"))
    B, S, nb = st.B, st.S, num_beams
    ctx = S + max_new_tokens
    M, K = B * nb, 2 * nb
    D, I, H, G, V, L = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_vocab, geo.llm_layers
    LDQ, W = (H + 2 * G) * HD, G * HD
    scale = HD ** -0.5
    f32, i32 = torch.float32, torch.int32
    buf = model._buf
    ws = _gemm_ws(model)
    frag = _fragments(model)
    head = weights_f32(model)["head"] if frag is None else ops.f32_weight(frag["head"], M, ws)

    # ---- KV cache (fp32) + the beam row index of the bf16 path
    kc = buf("f32_kc", (L, M * ctx * W), f32)
    vc = buf("f32_vc", (L, M * ctx * W), f32)
    index, index_tmp = kv_row_index(model, B, nb, S, ctx)
    # ---- prompt pass; every layer's rotated K / V go to the cache row of the utterance's first beam
    xn0, valid, left = prompt_pass_fp32(model, st, on_layer=lambda l, qkv_l: ops.f32_kv_fill(qkv_l, kc[l], vc[l], B, S, H, G, nb, ctx))
    if not left:
        raise ValueError("fp32 decode expects left-padded prompts (what the reference's inference collator builds)")
    kstart, last_rows = prompt_rows(model, B, S, nb, valid)
    x, xn = buf("f32_x", (M, D), f32), buf("f32_xn", (M, D), f32)
    logits = buf("f32_logits", (M, V), f32)
    ops.embed_rows(xn0, last_rows, xn, B, D)                    # the final-normed last prompt position of every utterance
    ops.f32_gemm(xn, weights_f32(model)["head"], logits, B, V, D, ws=ws)
    tv, ti = buf("dec_topv", (M, K), f32), buf("dec_topi", (M, K), i32)
    tkey = buf("dec_topkey", (M, K), f32) if sampling is not None and nb > 1 else None      # beam-sample: the candidates' keys
    bs = DeviceBeam(model, B, nb, max_new_tokens, eos, length_penalty, min_length, S, valid, repetition_penalty, sampling)
    topk_ws = buf("f32_topk_ws", (M * 16 * (2 + 2 * K),), f32)               # the row split over 16 workgroups (tasu_f32_logprob_topk)
    penalised, pmode = bs.penalty != 1.0, penalty_mode(nb)

    def topk_and_update(rows, first):
        """decode.py's topk_and_update on the fp32 logits (``repetition_penalty == 1.0``: exactly the launches without the knob)."""
        if tkey is not None:
            ops.f32_beam_sample_rows(logits, M, V, K, first, bs, 1, sampling.temperature, sampling.top_k, sampling.top_p, tkey, tv, ti)
            ops.beam_update_drawn(tkey, tv, ti, bs)
            if penalised:
                ops.beam_hist_update(bs)
            return
        if sampling is not None:
            ops.sample_uniform(bs.seed, bs.ctl, rows, bs.u)
            ops.f32_sample_rows(logits, rows, V, bs.u, bs.banned, 1, bs.hist, bs.hist_len, bs.penalty, sampling.temperature, sampling.top_k,
                                sampling.top_p, tv, ti)
        elif penalised:
            ops.f32_logprob_topk_hist(logits, rows, V, K, bs.banned, 1, bs.hist, bs.hist_len, bs.penalty, pmode, tv, ti, ws=topk_ws)
        else:
            ops.f32_logprob_topk(logits, rows, V, K, bs.banned, 1, tv, ti, ws=topk_ws)
        ops.beam_update(tv, ti, bs, first)
        if penalised:
            ops.beam_hist_update(bs)

    topk_and_update(B, True)                                                 # first position: empty history
    qkv, ao = buf("f32_qkv", (M, LDQ), f32), buf("f32_ao", (M, H * HD), f32)
    gu, act = buf("f32_gu", (M, 2 * I), f32), buf("f32_act", (M, I), f32)
    cos, sin = buf("dec_cos", (M, HD // 2), f32), buf("dec_sin", (M, HD // 2), f32)
    kcv, vcv = kc.view(L, M * ctx * W), vc.view(L, M * ctx * W)
    bufs = SimpleNamespace(x_in=x, x_mid=x, x_out=x, xn=xn, qkv=qkv, ao=ao, gu=gu, act=act, rows=M, cos=cos, sin=sin, ws=ws, keep=False)

    def attend_cache(l, qkv_, ao_):
        ops.f32_attn_decode(qkv_, kcv[l], vcv[l], index, kstart, bs.next_lens, ao_, M, H, G, ctx, scale)

    def device_step():
        """One generated position for all M beams (the launch sequence of decode.py's device_step, fp32 kernels)."""
        ops.kv_index_reorder(index, index_tmp, bs.next_src, bs.next_slot, M, ctx)       # beam reorder of the positions before this one
        ops.kv_index_reorder(index_tmp, index, None, bs.next_slot, M, ctx)
        ops.embed_rows(llm.embed, bs.next_ids, x, M, D)
        ops.rope_table(bs.next_pos, cos, sin, HD, geo.rope_theta)
        ops.f32_rmsnorm(x, llm.layers[0]["ln1"], xn, M, D, geo.rms_eps)
        for l in range(L):
            _layer_fp32(model, l, bufs, attend_cache, cache=(kcv[l], vcv[l], bs.next_slot), ctx=ctx, frag=frag)
        ops.f32_gemm(xn, head, logits, M, V, D, ws=ws)                                 # xn: the final norm, from the last layer's finisher
        topk_and_update(M, False)

    return decode_positions(model, bs, device_step, pad, "decode_fp32")
