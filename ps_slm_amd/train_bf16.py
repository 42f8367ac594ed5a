"""The decoder part of the bf16 training step: embedding merge -> 28 x decoder layer -> final norm -> lm_head -> shifted CE, and its
backward down to d(loss)/d(inputs_embeds) -- functions of (model, st); ps_slm_amd/train_fp32.py holds the fp32 step the same way.
TasuModel.forward_llm / backward_llm / _loss_on_labelled_rows / _head_wgrad delegate here.

The layer is spelt ONCE: layer_fwd and layer_bwd serve every recipe through two optional collaborators.

  * the adapter runner (``model._lora_run``, ps_slm_amd/lora.py: LoraRunner; None = no adapters, also the decode prefill on merged
    weights).  Per group (q|k|v, o, gate|up, down) it hands out the GEMM's operand and the head of it the producer writes, the
    weight and the contraction length -- [x | us] [W | B]^T at K = kext for an adapted group, x W^T otherwise -- and runs the
    members' rank GEMMs, their backward and the side stream's weight-gradient chains.
  * the full-fine-tuning hooks (``model.full_ft``, ps_slm_amd/full_ft.py; None = frozen decoder): the kept operands of every layer
    in the forward, a weight gradient next to each dgrad that consumes the same dY in the backward.

The step is replayed as a hipGraph on buffers the layers alias on purpose (``xn`` / ``act`` are overwritten per layer, operands live
in the head of the K-extended adapter buffers, ``dxb`` / ``dgu`` / ``dqkv`` are read in place by the side-stream chains): the order
of the launches and the buffer behind every argument are part of the contract, pinned per recipe by tests/test_step_trace_cpu.py.
"""
from types import SimpleNamespace

import torch

from .model import HD, StepState, rup
from .ops import GEMM_F32, GEMM_RESID


class _NoAdapters:
    """The adapter runner of a decoder without adapters: every group is the frozen Linear, nothing runs on a side stream."""
    members = {}

    def group(self, g, l, M, x, w, K):
        return x, x, w, K, ()

    def us(self, *a, **k):
        pass

    bwd = _wait_side = join = us


NO_ADAPTERS = _NoAdapters()


def forward_llm(model, st: StepState, compute_loss=True, need_backward=True, logits_rows="all"):
    ops, geo, llm = model.ops, model.geo, model.llm
    B, M = st.B, st.M
    D, I, H, G, V = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_vocab
    Spad, Vp, LDQ = st.plan.Spad, rup(V, 64), (H + 2 * G) * HD
    L = geo.llm_layers
    d, buf = st.dev, model._buf
    bf, f32 = torch.bfloat16, torch.float32
    xs = buf("xs", (2 * L + 1, M, D), f32)                 # x_in[l] = xs[2l], x_mid[l] = xs[2l+1], final = xs[2L]
    ops.embed_merge(llm.embed, d["y2"], d["kind"], d["idx"], xs[0], M, D)
    cos, sin = buf("cos", (M, HD // 2), f32), buf("sin", (M, HD // 2), f32)
    ops.rope_table(d["pos"], cos, sin, HD, geo.rope_theta)
    rstd = buf("rstd", (2 * L + 1, M), f32)
    b = SimpleNamespace(xs=xs, rstd=rstd, cos=cos, sin=sin, qkv=buf("qkv", (L, M, LDQ), bf), ao=buf("ao", (L, M, H * HD), bf),
                        lse=buf("lse", (L, B * H * Spad), f32), gu=buf("gu", (L, M, 2 * I), bf), xn=buf("xn_llm", (M, D), bf),
                        act=buf("act", (M, I), bf))
    if geo.qk_norm and need_backward:
        # Qwen3: the plain q|k|v projection of every layer (the head norm's backward reads it) and the heads' rstd; without a
        # backward (eval forward, decode prefill) the norm runs in place on qkv[l] and keeps nothing
        b.qkv_pre, b.qk_rstd = buf("qkv_pre", (L, M, LDQ), bf), buf("qk_rstd", (L, M, H + G), f32)
    lora, ft = model._lora_run, model.full_ft
    # full fine-tuning keeps the GEMM operands of every layer for the weight gradients (the normed inputs and the SwiGLU output;
    # the frozen step overwrites one buffer), and runs no compact tail: the last layer's MLP weights want all rows' operands in
    # the same [M, .] form as every other layer's
    keep = ft is not None and need_backward
    if keep:
        d.update(ft_xn=buf("ft_xn", (2 * L, M, D), bf), ft_act=buf("ft_act", (L, M, I), bf))
    tail = bool(model.tail_rows and compute_loss and need_backward and not model.keep_logits and logits_rows != "none"
                and "lab_rows" in d and st.nLp > 0 and lora is None and ft is None)
    drop = lora is not None and model.lora.drop_on(model.training)
    if drop:
        ops.rng_advance(model.lora.rng)                    # new masks for this micro-step (a launch: graph replays advance too)
    st.lora_drop = drop
    for l in range(L):
        layer_fwd(model, st, l, b, lora, ft if keep else None, drop, tail and l == L - 1)
    d.update(xs=xs, cos=cos, sin=sin, rstd=rstd, qkv=b.qkv, ao=b.ao, lse=b.lse, gu=b.gu)
    if geo.qk_norm and need_backward:
        d.update(qkv_pre=b.qkv_pre, qk_rstd=b.qk_rstd)
    if logits_rows == "none":                              # decode prefill: the caller projects the last rows only
        return
    if compute_loss and need_backward and not model.keep_logits:
        return loss_on_labelled_rows(model, st)
    xn = b.xn                                              # (never a layer's kept operand)
    ops.rmsnorm_fwd(xs[2 * L], llm.norm, xn, rstd[2 * L], geo.rms_eps)
    logits = buf("logits", (M, Vp), bf)
    ops.gemm(xn, llm.head, logits, M, V, D)
    d.update(logits=logits, xn_head=xn)
    if not compute_loss:
        return
    row_loss, row_hit = buf("row_loss", (M,), f32), buf("row_hit", (M,), torch.int32)
    # per-row argmax (the reference's `preds`, ps-slm.py:533) only matters at labelled rows for the accuracy; the kernel
    # skips the scan of ignored rows when no argmax buffer is passed, which the training step does
    row_arg = None if need_backward else buf("row_arg", (M,), torch.int32)
    dlogits = buf("dlogits", (M, Vp), bf) if need_backward else None          # (the throughput mode left above: its dlogits overwrite the compact logits)
    ops.ce_fwd_bwd(logits, d["shift_labels"], M, V, row_loss, row_hit, row_arg, dlogits, d["inv_count"])
    res = buf("loss_out", (4,), f32)
    ops.ce_reduce(row_loss, row_hit, d["shift_labels"], M, res)
    d.update(dlogits=dlogits, loss_out=res, row_arg=row_arg)


def layer_fwd(model, st, l, b, lora=None, ft=None, drop=False, tail=False):
    """One decoder layer (modeling_qwen2.py's Qwen2DecoderLayer; an adapted Linear = base + low-rank branch in ONE K-extended GEMM).
    ``tail``: the last layer of the frozen throughput step -- its MLP runs on the nLp labelled rows only."""
    ops, geo, d, w = model.ops, model.geo, st.dev, model.llm.layers[l]
    B, S, M = st.B, st.S, st.M
    D, I, H, G, eps = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.rms_eps
    ad = lora or NO_ADAPTERS
    x_in, x_mid, x_out = b.xs[2 * l], b.xs[2 * l + 1], b.xs[2 * l + 2]
    xn1, xn2, act = (b.xn, b.xn, b.act) if ft is None else (d["ft_xn"][2 * l], d["ft_xn"][2 * l + 1], d["ft_act"][l])
    # ---- attention block: the norm writes straight into the head of the q|k|v operand; bias + RoPE in the GEMM's epilogue
    a, x1, wq, K, ts = ad.group("qkv", l, M, xn1, w["wqkv"], D)
    ops.rmsnorm_fwd(x_in, w["ln1"], x1, b.rstd[2 * l], eps)
    ad.us(l, "qkv", ts, M, x1, drop, norm=(x_in, w["ln1"], b.rstd[2 * l]))
    if geo.qk_norm:
        # Qwen3: a plain NT GEMM, then the per-head q/k RMSNorm and the rotation in one row-wise launch (csrc/qk_norm.hip)
        kept = hasattr(b, "qkv_pre")                       # (a backward follows; else in place: out == pre, no rstd -- the same bits)
        pre = b.qkv_pre[l] if kept else b.qkv[l]
        ops.gemm(a, wq, pre, M, (H + 2 * G) * HD, K)
        ops.qk_norm_rope_fwd(pre, w["q_norm"], w["k_norm"], b.cos, b.sin, b.qkv[l], b.qk_rstd[l] if kept else None, M, H, G, eps)
    else:
        ops.gemm_qkv_rope(a, wq, w["bqkv"], b.qkv[l], b.cos, b.sin, M, H, G, K)
    ops.attn_fwd(b.qkv[l], None, d["key_mask"], b.ao[l], b.lse[l], B, S, H, G, HD ** -0.5, True)
    a, _, wo, K, ts = ad.group("o", l, M, b.ao[l], w["wo"], H * HD)
    if ts:
        ops.copy_rows(b.ao[l], a, M, H * HD)               # (the attention kernels write a dense [M, H * 128])
        ad.us(l, "o", ts, M, b.ao[l], drop)
    ops.gemm(a, wo, x_mid, M, D, K, resid=x_in, mode=GEMM_RESID)
    if tail:
        # the last layer's MLP on the nLp labelled rows (compact operands; row gathers by the plan's index)
        n, buf, bf, f32 = st.nLp, model._buf, torch.bfloat16, torch.float32
        xn_t, rstd_t = buf("xn_tail", (n, D), bf), buf("rstd_tail", (n,), f32)
        ops.rmsnorm_fwd_rows(x_mid, d["lab_rows"], w["ln2"], xn_t, rstd_t, eps)
        gu_t, act_t = buf("gu_tail", (n, 2 * I), bf), buf("act_tail", (n, I), bf)
        ops.gemm_gate_up_swiglu(xn_t, w["wgu"], gu_t, act_t, n, I, D)
        xmid_t = buf("xmid_tail", (n, D), f32)
        ops.embed_rows(x_mid, d["lab_rows0"], xmid_t, n, D)
        xout_t = buf("xout_tail", (n, D), f32)
        ops.gemm(act_t, w["wd"], xout_t, n, D, I, resid=xmid_t, mode=GEMM_RESID)
        d.update(rstd_tail=rstd_t, gu_tail=gu_t, xout_tail=xout_t)
        return
    # ---- MLP block: the SwiGLU epilogue writes act into the head of the down projection's operand
    a_d, act, wd, K_d, ts_d = ad.group("down", l, M, act, w["wd"], I)
    a, x2, wg, K, ts = ad.group("gu", l, M, xn2, w["wgu"], D)
    ops.rmsnorm_fwd(x_mid, w["ln2"], x2, b.rstd[2 * l + 1], eps)
    ad.us(l, "gu", ts, M, x2, drop, norm=(x_mid, w["ln2"], b.rstd[2 * l + 1]))
    ops.gemm_gate_up_swiglu(a, wg, b.gu[l], act, M, I, K)
    ad.us(l, "down", ts_d, M, act, drop)
    ops.gemm(a_d, wd, x_out, M, D, K_d, resid=x_mid, mode=GEMM_RESID)


def loss_on_labelled_rows(model, st: StepState):
    """Throughput form of the loss head (training step, ``keep_logits=False``): the shifted CE ignores every position
    without a label (loss_utils.py:49-71, ignore_index -100), so final norm -> lm_head -> CE -> dlogits run over the
    labelled rows only, gathered into a compact [nLp, D] operand (half of the 4096 rows of the benchmark batch, whose
    prompt and audio positions carry no label).  Loss, accuracy and every gradient equal the full-materialisation path's
    (rows without a label have dlogits == 0 there); ``outputs.logits`` does not exist in this mode."""
    ops, geo, llm, d, buf = model.ops, model.geo, model.llm, st.dev, model._buf
    D, V, L = geo.llm_dim, geo.llm_vocab, geo.llm_layers
    Vp, n = rup(V, 64), st.nLp
    bf, f32 = torch.bfloat16, torch.float32
    xn_c, rstd_c = buf("xn_lab", (n, D), bf), buf("rstd_lab", (n,), f32)
    if "xout_tail" in d:                                   # the last layer already produced the labelled rows compact
        ops.rmsnorm_fwd(d["xout_tail"], llm.norm, xn_c, rstd_c, geo.rms_eps)
    else:
        ops.rmsnorm_fwd_rows(d["xs"][2 * L], d["lab_rows"], llm.norm, xn_c, rstd_c, geo.rms_eps)
    logits = buf("logits", (n, Vp), bf)
    ops.gemm(xn_c, llm.head, logits, n, V, D)
    row_loss, row_hit = buf("row_loss", (n,), f32), buf("row_hit", (n,), torch.int32)
    ops.ce_fwd_bwd(logits, d["lab_compact"], n, V, row_loss, row_hit, None, logits, d["inv_count"])   # dlogits in place
    res = buf("loss_out", (4,), f32)
    ops.ce_reduce(row_loss, row_hit, d["lab_compact"], n, res)
    d.update(dlogits=logits, loss_out=res, row_arg=None, rstd_lab=rstd_c, labelled_only=True, xn_head=xn_c)
    d.pop("logits", None)


def head_wgrad(model, st, dst=None):
    """use_emb with tied embeddings: the lm_head's weight gradient dW = dlogits^T h is the second term of the table's gradient
    (h: the final-normed rows that fed the lm_head GEMM -- the compact labelled rows in the throughput mode).  fp32, on the MFMA
    GEMM behind the transposes the projector's dW1 uses, straight into (overwriting) the table's range of the bucket; rows
    without a label and the padding rows have dlogits == 0 / h == 0."""
    ops, geo, d = model.ops, model.geo, st.dev
    V, D, Vp = geo.llm_vocab, geo.llm_dim, rup(geo.llm_vocab, 64)
    n = st.nLp if d.get("labelled_only") else st.M
    npad = rup(n, 64)
    dl_t = model._buf("emb_dl_t", (Vp, npad), torch.bfloat16)
    h_t = model._buf("emb_h_t", (D, npad), torch.bfloat16)
    ops.transpose(d["dlogits"], dl_t, n, Vp, npad, Vp)
    ops.transpose(d["xn_head"], h_t, n, D, npad, D)
    # (dst: the untied lm_head's own range when the whole decoder trains -- the same product)
    ops.gemm(dl_t, h_t, model.embed_view(model.proj.g) if dst is None else dst, V, D, npad, mode=GEMM_F32)


def backward_llm(model, st: StepState, span=None):
    """lm_head dgrad, final norm, 28 decoder layers (dgrad only unless the LLM trains).  Leaves d(loss)/d(inputs_embeds)
    in the fp32 workspace buffer ``dx``.  ``span`` = (hi, lo): only layers hi - 1 .. lo (the loss head with the span that
    starts at the last layer) -- the adapters' gradient exchange cuts the backward into such spans (run_backward)."""
    ops, geo, llm = model.ops, model.geo, model.llm
    B, M = st.B, st.M
    D, I, H, G, V = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_vocab
    Spad, Vp, LDQ = st.plan.Spad, rup(V, 64), (H + 2 * G) * HD
    L = geo.llm_layers
    d, buf = st.dev, model._buf
    bf, f32 = torch.bfloat16, torch.float32
    xs, rstd = d["xs"], d["rstd"]
    b = SimpleNamespace(dx=buf("dx", (M, D), f32), dxb=buf("dxb", (M, D), bf),
                        dn=buf("dn", (M, D), bf),          # gradient wrt a normed activation
                        dact=buf("dact", (M, I), bf), dgu=buf("dgu", (M, 2 * I), bf), dao=buf("dao", (M, H * HD), bf),
                        delta=buf("delta", (B * H * Spad,), f32), dqkv=buf("dqkv", (M, LDQ), bf), dkp=buf("dkp", (M, H * HD), f32),
                        dvp=buf("dvp", (M, H * HD), f32))
    dx, dxb, dn = b.dx, b.dxb, b.dn
    l_hi, l_lo = span if span is not None else (L, 0)
    lora, ft = model._lora_run, model.full_ft
    # lm_head dgrad (K = Vpad: dlogits pad columns are zero) and final norm
    if l_hi == L and model.embed_base is not None and geo.tied:
        head_wgrad(model, st)
    elif l_hi == L and ft is not None:
        head_wgrad(model, st, ft.view(model.proj.g, "head"))
    if l_hi < L:                                           # a later span: the loss head ran with the first one
        pass
    elif d.get("labelled_only"):
        n = st.nLp
        dn_c = buf("dn_lab", (n, D), bf)
        # [nLp, D] outputs in 128 x 192 tiles behind K = Vp: when they cover at most half of the 256 CUs the K range is
        # split so that every CU works (2048 labelled rows x 1536: 128 tiles x 2 ranges)
        tiles = ((n + 127) // 128) * ((D + 191) // 192)
        ksplit = max(1, min(256 // tiles, 8))
        while ksplit > 1 and Vp % (64 * ksplit):
            ksplit -= 1
        if ksplit > 1 and D % 4 == 0:
            ws = buf("dn_lab_slabs", (ksplit, n, D), f32)
            ops.gemm_splitk(d["dlogits"], llm.head_t, dn_c, n, D, Vp, ksplit, ws)
        else:
            ops.gemm(d["dlogits"], llm.head_t, dn_c, n, D, Vp)
        if "xout_tail" in d:
            # final norm and the last layer's MLP on the compact rows; the post-attention norm's backward scatters the result
            # (+ the rows' residual gradient) back to all M rows for that layer's attention backward
            w = llm.layers[L - 1]
            dx_t, dxb_t = buf("dx_tail", (n, D), f32), buf("dxb_tail", (n, D), bf)
            ops.rmsnorm_bwd(dn_c, d["xout_tail"], llm.norm, d["rstd_lab"], dx_t, dxb_t, False)
            dact_t, dgu_t = buf("dact_tail", (n, I), bf), buf("dgu_tail", (n, 2 * I), bf)
            ops.gemm_dswiglu(dxb_t, w["wd_t"], d["gu_tail"], dgu_t, dact_t, n, I, D)
            ops.gemm(dgu_t, w["wgu_t"], dn_c, n, D, 2 * I)
            ops.rmsnorm_bwd_rows_resid(dn_c, xs[2 * L - 1], w["ln2"], d["rstd_tail"], d["lab_slot"], dx_t, dx, dxb)
        else:
            if ft is not None:                             # model.norm.weight: compact dy / rstd, x by the labelled rows' index
                ft.norm_wgrad(dn_c, xs[2 * L], d["rstd_lab"], "norm", None, src_rows=d["lab_rows"])
            ops.rmsnorm_bwd_rows(dn_c, xs[2 * L], llm.norm, d["rstd_lab"], d["lab_slot"], dx, dxb)
    else:
        ops.gemm(d["dlogits"], llm.head_t, dn, M, D, Vp)
        if ft is not None:
            ft.norm_wgrad(dn, xs[2 * L], rstd[2 * L], "norm", None)
        ops.rmsnorm_bwd(dn, xs[2 * L], llm.norm, rstd[2 * L], dx, dxb, False)
    drop = bool(getattr(st, "lora_drop", False))
    for l in range(l_hi - 1, l_lo - 1, -1):
        layer_bwd(model, st, l, b, lora, ft, drop, mlp=not (l == L - 1 and "xout_tail" in d))
    if lora is not None:
        lora.join()                                        # the adapters' weight-gradient chains (side stream) are back
    d["dx"] = dx


def layer_bwd(model, st, l, b, lora=None, ft=None, drop=False, mlp=True):
    """Backward of one decoder layer: the dgrad chain; with ``ft`` every weight gradient next to the dgrad that consumes the same
    dY; with ``lora`` a group's adapter backward behind the base dgrad that produced its dx_base.  The adapters' weight-gradient
    chains on the side stream read the group's output gradient IN PLACE (dxb, dgu, dqkv: no transposed copy, tasu_gemm_tn_rank):
    the main stream waits for a group's chain right before the kernel that rewrites that buffer.  ``mlp=False``: the compact tail
    has done this (the last) layer's MLP."""
    ops, geo, d, w = model.ops, model.geo, st.dev, model.llm.layers[l]
    B, S, M = st.B, st.S, st.M
    D, I, H, G = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads
    LDQ, ad = (H + 2 * G) * HD, lora or NO_ADAPTERS
    xs, rstd = d["xs"], d["rstd"]
    x_in, x_mid = xs[2 * l], xs[2 * l + 1]
    dx, dxb, dn, dgu, dqkv = b.dx, b.dxb, b.dn, b.dgu, b.dqkv
    if mlp:
        if "down" in ad.members:                           # its adapters want d(act) itself: dgrad and SwiGLU backward apart
            ops.gemm(dxb, w["wd_t"], b.dact, M, I, D)
            ad.bwd(l, "down", dxb, D, M, I, b.dact, drop)
            ad._wait_side("gu")                                  # (the previous layer's chain over dgu)
            ops.swiglu_bwd(b.dact, d["gu"][l], dgu, M, I)
        else:
            ad._wait_side("gu")
            ops.gemm_dswiglu(dxb, w["wd_t"], d["gu"][l], dgu, b.dact, M, I, D)
        if ft is not None:
            ft.wgrad(dxb, d["ft_act"][l], "wd", l)
        ops.gemm(dgu, w["wgu_t"], dn, M, D, 2 * I)
        if ft is not None:
            ft.wgrad(dgu, d["ft_xn"][2 * l + 1], "wgu", l)
            ft.norm_wgrad(dn, x_mid, rstd[2 * l + 1], "ln2", l)
        ad.bwd(l, "gu", dgu, 2 * I, M, D, dn, drop)
        ad._wait_side("down")                                    # its chain read dxb
        ops.rmsnorm_bwd(dn, x_mid, w["ln2"], rstd[2 * l + 1], dx, dxb, True)
    if ft is not None:
        ft.wgrad(dxb, d["ao"][l], "wo", l)
    ops.gemm(dxb, w["wo_t"], b.dao, M, H * HD, D)
    ad.bwd(l, "o", dxb, D, M, H * HD, b.dao, drop, shared=d["ao"][l])
    ad._wait_side("qkv")                                         # (the previous layer's chain over dqkv)
    # delta = rowsum(dO . O), dQ, dK / dV and the rotary embedding's backward behind one entry point: the single-pass kernels
    # for Spad <= 256 (delta inside the kernel; dkp / dvp = one fp32 partial per query head), else the tiled kernels
    ops.attn_bwd_fused(d["qkv"][l], d["key_mask"], b.dao, d["ao"][l], d["lse"][l], b.delta, d["cos"], d["sin"], dqkv, b.dkp, b.dvp,
                       B, S, H, G, HD ** -0.5, True)
    if geo.qk_norm:                                        # dqkv: gradient of the normed heads -> of the plain projection
        if ft is not None:                                 # the head norms' weight gradients read dqkv before it is overwritten
            ft.qk_wgrad(dqkv, d["qkv_pre"][l], d["qk_rstd"][l], l)
        ops.qk_norm_bwd(dqkv, d["qkv_pre"][l], w["q_norm"], w["k_norm"], d["qk_rstd"][l], M, H, G)
    if ft is not None:
        ft.wgrad(dqkv, d["ft_xn"][2 * l], "wqkv", l)
        if geo.qkv_bias:
            ft.bias_wgrad(dqkv, "bqkv", l)                 # q|k|v bias: dqkv behind the RoPE backward
    ops.gemm(dqkv, w["wqkv_t"], dn, M, D, LDQ)
    if ft is not None:
        ft.norm_wgrad(dn, x_in, rstd[2 * l], "ln1", l)
    ad.bwd(l, "qkv", dqkv, LDQ, M, D, dn, drop)
    ad._wait_side("o")                                           # its chain read dxb
    ops.rmsnorm_bwd(dn, x_in, w["ln1"], rstd[2 * l], dx, dxb, True)
