"""fp32 arithmetic mode of the TRAINING step (``train_config.use_fp16 = false``: the reference's shipped recipe,
Multitask/scripts/finetune_deespeed_sensevoice.sh:37 -- forward and backward outside autocast, Multitask/utils/deepspeed_utils.py:160,
205-236).  Same network, same schedule as ps_slm_amd/model.py's bf16 step, every tensor fp32:

  forward   posterior -> LayerNorm -> Linear -> SiLU -> Linear (fp32 masters) -> embedding merge -> 28 x [RMSNorm, q|k|v + bias + RoPE,
            causal attention, o + residual, RMSNorm, gate|up, SwiGLU, down + residual] -> RMSNorm -> lm_head -> shifted CE
            (decode_fp32.prompt_pass_fp32, the one fp32 decoder forward, with ``keep``: the activations of every layer kept --
            residual stream, rotated q|k|v, attention output, gate|up -- and the projector's LayerNorm statistics and pre-SiLU rows)
  backward  dlogits (written by the CE kernel over the logits) -> lm_head dgrad -> 28 x [MLP, attention] dgrad through the frozen
            decoder (tasu_f32_gemm_nt on transposed fp32 weight copies; csrc/fp32_train.hip for RMSNorm / SwiGLU / attention / RoPE
            backward; attention probabilities are recomputed from the saved q|k|v) -> the audio rows' gradient -> projector weight
            gradients straight into the flat fp32 bucket ``proj.g`` (what TasuEngine's AdamW and the autograd boundary read).

A correctness mode: ~10x slower than the bf16 step at Qwen2.5-1.5B (271 against 28 ms per 16 utterances: the fp32 matrix rate is 1/16 of bf16's; the step runs at 0.61 of it); pinned on the
real reference's fp32 goldens (loss within 2e-5, projector gradients within 2e-4 relative L2: tests/test_gpu_model.py).  By default the
decoder's weights stay frozen (dgrad only).  With freeze_llm = false every decoder tensor trains here as well (ps_slm_amd/full_ft.py:
the fp32 masters of the bucket ARE the weights this forward reads; csrc/wgrad_f32.hip forms dW = dY^T X next to the dgrad that
consumes the same dY, from the kept activations -- the normed inputs and the SwiGLU output are rebuilt, not stored), and with
use_peft + use_emb the embedding table's gradient (lookup term + the tied head's term) joins the adapters'.  Every projector the package serves trains here -- linear-silu, linear and cov1d-linear
(ReLU backward by the kept outputs' mask, the conv as one GEMM over the k-frame rows) and cross-attention (dq over the whole
embedding table: tasu_f32_ca_attn_bwd, then dW_q = dq^T post) -- and so does an adapted decoder (use_peft: LoraF32 below, the
unmerged forward y = W x + s B (A drop(x)) and the adapters' gradients into the bucket's tail).

The layer is spelt ONCE per direction, as ps_slm_amd/train_bf16.py spells the bf16 step's -- decode_fp32._layer_fp32 (decode's and
eval's layer, handed the adapter runner) and layer_bwd below -- and serves every recipe through two optional collaborators that
exclude each other: the adapter runner (LoraF32) and the full-fine-tuning hooks (``model.full_ft``).  The sums are order-dependent
by design (K ascending, slabs in ascending order), so the ORDER of the launches and the buffer behind every argument fix the bits of
the loss and the gradients: pinned per recipe on a CPU double by tests/test_f32_step_trace_cpu.py.
"""
from types import SimpleNamespace

import torch

from .decode_fp32 import _gemm_ws, prompt_pass_fp32
from .full_ft import f32_wgrad
from .model import HD, StepState, rup


def _transposed_weights(model):
    """fp32 W^T copies of the frozen decoder weights for the dgrad GEMMs (built once per model: +1x the fp32 weight bytes)."""
    llm = model.llm
    t = llm.f32.get("t")
    if t is None or t.get("head") is None:                 # (head None: the tied embedding table changed, the layers' copies stand)
        Vp = rup(model.geo.llm_vocab, 64)
        head = llm.f32["head"]
        head_t = torch.zeros(head.shape[1], Vp, dtype=torch.float32, device=head.device)
        head_t[:, : head.shape[0]].copy_(head.t())
        if t is None:
            t = llm.f32["t"] = dict(layers=[{k: f[k].t().contiguous() for k in ("wqkv", "wo", "wgu", "wd")} for f in llm.f32["layers"]])
        t["head"] = head_t
    return t


def forward_train_fp32(model, st: StepState):
    """Forward of the training step in fp32: the shared prompt pass with everything the backward needs kept in ``st.dev['f32t']``,
    then the Vp-wide logits with the CE gradient written over them; loss / accuracy in ``st.dev['loss_out']`` like the bf16 step;
    ``st.fp32 = True`` routes ``TasuModel.run_backward`` to ``backward_fp32``."""
    ops, geo, llm, pr = model.ops, model.geo, model.llm, model.proj
    # The shipped recipe (linear-silu, no adapters) trains in fp32 whenever use_fp16 = false.  The other recipes are opt-in: their
    # default selection pins the bf16 step (model_factory: train_config.mixed_precision), so a model that was not selected for the
    # fp32 step (arith_train != "fp32") is refused here, before any fp32 launch, instead of silently changing arithmetic
    if model.arith_train != "fp32":
        if model.lora is not None:
            raise NotImplementedError("the fp32 training step of a LoRA model is opt-in: select it with train_config.use_fp16=false and "
                                      "mixed_precision=false (arith_train = 'fp32'); by default an adapted model trains on the bf16 path")
        if pr.kind != "linear-silu":
            raise NotImplementedError(f"the fp32 training step serves the shipped projector (linear-silu) by default; for {pr.kind!r} it "
                                      "is opt-in: train_config.use_fp16=false and mixed_precision=false (arith_train = 'fp32')")
    if pr.kind != "linear-silu" and model.raw_features:
        raise NotImplementedError("the fp32 training step of the alternate projectors serves the CTC-posterior branch (ctc_posterior=true)")
    M, D, V = st.M, geo.llm_dim, geo.llm_vocab
    f32, i32 = torch.float32, torch.int32
    buf, d = model._buf, st.dev
    keep = {}
    lo = lora_f32(model) if model.lora is not None else None       # an adapted decoder trains with its adapters unmerged
    st.lora_drop = lo is not None and model.lora.drop_on(model.training)
    if st.lora_drop:
        ops.rng_advance(model.lora.rng)        # new masks for this micro-step, as the bf16 step draws them (TasuModel.forward_llm)
    xn, _, _ = prompt_pass_fp32(model, st, keep=keep, lo=lo, drop=st.lora_drop)
    # ---- loss head: logits for every position (pad columns zeroed once: the lm_head dgrad contracts over Vp), CE + its gradient
    logits = buf("f32t_logits", (M, rup(V, 64)), f32)
    ops.f32_gemm(xn, llm.f32["head"], logits, M, V, D, ws=_gemm_ws(model))
    row_loss, row_hit = buf("row_loss", (M,), f32), buf("row_hit", (M,), i32)
    ops.f32_ce(logits, d["shift_labels"], M, V, row_loss, row_hit, dlogits=logits, inv_count=d["inv_count"])   # dlogits in place
    res = buf("loss_out", (4,), f32)
    ops.ce_reduce(row_loss, row_hit, d["shift_labels"], M, res)
    d.update(loss_out=res, f32t=dict(keep, dlogits=logits))
    d.pop("logits", None)
    st.fp32 = True


def _rebuilt(model, st, which, l=None):
    """A weight gradient's operand that the step does not keep, rebuilt from what it keeps, for whichever collaborator wants it:
    ``"norm"`` the final norm of xs[2L], ``"ln2"`` of xs[2l + 1], ``"ln1"`` of xs[2l]; ``"act"`` the SwiGLU of gus[l]."""
    ops, geo, llm, a = model.ops, model.geo, model.llm, st.dev["f32t"]
    if which == "act":
        out = model._buf("f32t_lora_act", (st.M, geo.llm_inter), torch.float32)
        ops.f32_swiglu(a["gus"][l], out, st.M, geo.llm_inter)
        return out
    x, w = (a["xs"][2 * geo.llm_layers], llm.norm) if which == "norm" else (a["xs"][2 * l + (which == "ln2")], llm.layers[l][which])
    out = model._buf("f32t_lora_xn", (st.M, geo.llm_dim), torch.float32)
    ops.f32_rmsnorm(x, w, out, st.M, geo.llm_dim, geo.rms_eps)
    return out


def layer_bwd(model, st, l, b, lo, ft, drop):
    """Backward of one decoder layer: the dgrad chain from b.dx, the gradient of the layer's output, to that of its input (in b.dx),
    and behind every base dgrad what the one collaborator that is set (backward_fp32) hangs there."""
    ops, geo, a = model.ops, model.geo, st.dev["f32t"]
    M, D, I, H, G = st.M, geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads
    xs, ws, w, t = a["xs"], b.ws, model.llm.layers[l], b.wt["layers"][l]
    dx, dn, dact, dgu, dao, dqkv = b.dx, b.dn, b.dact, b.dgu, b.dao, b.dqkv

    def behind(g, dy, dx_base, name, which):
        """Behind the dgrad dy -> dx_base of group ``g`` (Linear ``name``), on the group's input -- ``which`` of _rebuilt, None: the
        kept attention output: ``lo``: the members' adapter backward, their dx added to dx_base; ``ft``: every weight gradient
        next to the dgrad that consumes the same dY -- the Linear's, its bias', and the norm's in front of it."""
        if ft is None and (lo is None or g not in lo.members):
            return
        x = a["aos"][l] if which is None else _rebuilt(model, st, which, l)
        if lo is not None:
            return lo.backward(l, g, x, dy, dx_base, M, ws, drop)
        ft.wgrad32(dy, x, name, l)
        if name == "wqkv" and geo.qkv_bias:
            ft.bias_wgrad32(dy, "bqkv", l)                 # q|k|v bias: dqkv behind the inverse RoPE
        if which in ("ln1", "ln2"):
            ft.norm_wgrad32(dx_base, xs[2 * l + (which == "ln2")], which, l)

    # MLP block: x_out = x_mid + down(swiglu(gate|up(norm(x_mid))))
    ops.f32_gemm(dx, t["wd"], dact, M, I, D, ws=ws)
    behind("down", dx, dact, "wd", "act")
    ops.f32_swiglu_bwd(dact, a["gus"][l], dgu, M, I)
    ops.f32_gemm(dgu, t["wgu"], dn, M, D, 2 * I, ws=ws)
    behind("gu", dgu, dn, "wgu", "ln2")
    ops.f32_rmsnorm_bwd(dn, xs[2 * l + 1], w["ln2"], dx, M, D, geo.rms_eps, True)
    # attention block: x_mid = x_in + o(attention(rope(q|k|v(norm(x_in)))))
    ops.f32_gemm(dx, t["wo"], dao, M, H * HD, D, ws=ws)
    behind("o", dx, dao, "wo", None)
    ops.f32_attn_bwd(a["qkvs"][l], dao, a["kstart"], dqkv, b.lse, b.delta, st.B, st.S, H, G, HD ** -0.5)
    ops.f32_rope(dqkv, a["cos"], a["sin"], M, H, G, inverse=True)
    if geo.qk_norm:                                        # dqkv: gradient of the normed heads -> of the plain projection
        if ft is not None:                                 # the head norms' weight gradients read dqkv before it is overwritten
            ft.qk_wgrad(dqkv, a["qkv_pres"][l], a["qk_rstds"][l], l)
        ops.f32_qk_norm_bwd(dqkv, a["qkv_pres"][l], w["q_norm"], w["k_norm"], a["qk_rstds"][l], M, H, G)
    ops.f32_gemm(dqkv, t["wqkv"], dn, M, D, (H + 2 * G) * HD, ws=ws)
    behind("qkv", dqkv, dn, "wqkv", "ln1")
    ops.f32_rmsnorm_bwd(dn, xs[2 * l], w["ln1"], dx, M, D, geo.rms_eps, True)


def backward_fp32(model, st: StepState, on_ready=None):
    """dgrad through the decoder and the weight gradients of everything that trains -- the projector, the adapters, the decoder's
    own tensors (freeze_llm = false), the embedding table -- into ``proj.g``, all fp32.  ``on_ready(lo, hi)``: the engine's
    gradient exchange hook, called once for the trained part of the bucket at the end (this mode does not overlap the exchange)."""
    ops, geo, llm, pr = model.ops, model.geo, model.llm, model.proj
    B, S, M = st.B, st.S, st.M
    D, I, H, G, V, L = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_vocab, geo.llm_layers
    f32, buf, d = torch.float32, model._buf, st.dev
    a = d["f32t"]
    lo, ft = lora_f32(model) if model.lora is not None else None, model.full_ft
    # the two collaborators exclude each other (enable_llm_training refuses a LoRA model: with use_peft the base weights stay frozen),
    # so wherever both could want a group's rebuilt operand, one of them does
    assert lo is None or ft is None
    drop = bool(getattr(st, "lora_drop", False))
    head_term = ft is not None or (model.embed_base is not None and geo.tied)   # dW of the lm_head: its own tensor, or the tied table's
    b = SimpleNamespace(wt=_transposed_weights(model), ws=_gemm_ws(model),
                        dx=buf("f32t_dx", (M, D), f32), dn=buf("f32t_dn", (M, D), f32),          # dn: gradient wrt a normed activation
                        dact=buf("f32t_dact", (M, I), f32), dgu=buf("f32t_dgu", (M, 2 * I), f32),
                        dao=buf("f32t_dao", (M, H * HD), f32), dqkv=buf("f32t_dqkv", (M, (H + 2 * G) * HD), f32),
                        lse=buf("f32t_lse", (B * H * S,), f32), delta=buf("f32t_delta", (B * H * S,), f32))
    # loss head
    if head_term:
        # dlogits^T xn over all rows (rows without a label hold zeros): the untied lm_head's gradient, or the head term of the tied
        # table's, which backward_embed's lookup term is added to
        xn = _rebuilt(model, st, "norm")
        if ft is not None:
            ft.wgrad32(a["dlogits"][:, :V], xn, "head", dst=model.embed_view(pr.g) if geo.tied else None)
        else:
            f32_wgrad(model, a["dlogits"][:, :V], xn, model.embed_view(pr.g))
    ops.f32_gemm(a["dlogits"], b.wt["head"], b.dn, M, D, rup(V, 64), ws=b.ws)
    if ft is not None:
        ft.norm_wgrad32(b.dn, a["xs"][2 * L], "norm", None)
    ops.f32_rmsnorm_bwd(b.dn, a["xs"][2 * L], llm.norm, b.dx, M, D, geo.rms_eps, False)
    for l in range(L - 1, -1, -1):
        layer_bwd(model, st, l, b, lo, ft, drop)
    d["dx"] = b.dx
    if model.embed_base is not None:           # the table's lookup term, on top of the head term (tied) or of zeros
        model.backward_embed(st)
    if model.freeze_projector:                 # (a frozen projector: the adapters' / the decoder's part of the bucket alone)
        if on_ready is not None:
            on_ready(model.trainable_lo, pr.numel)
        return
    # ---- merge backward + projector backward (projector.py:149-151 / :38-49 / :60-73 / :111-126 reversed); weight gradients land
    # in the flat bucket
    Rap, Kp, Do = st.Rap, pr.Kp, pr.Do
    rows = d["audio_rows_pad"] if "audio_rows_pad" in d else model._pad_rows(st)
    dy2 = buf("f32t_dy2", (Rap, Do), f32)
    ops.f32_gather_rows(b.dx, rows, dy2, Rap, Do)

    def wgrad(dy, x, name):                    # g[name] [N, K] = dy^T x over the Rap rows (a multiple of 64: the route pads nothing)
        f32_wgrad(model, dy, x, pr.view(pr.g, name), route="composed")

    def dgrad(dy, name, tag):                  # dy [Rap, N] W[name] [N, K] -> [Rap, K]
        N, K = pr.view(pr.p, name).shape
        w_t, out = buf(f"f32t_{tag}_w_t", (K, N), f32), buf(f"f32t_{tag}_dx", (Rap, K), f32)
        ops.f32_transpose(pr.view(pr.p, name), w_t, N, K, N)
        ops.f32_gemm(dy, w_t, out, Rap, K, N, ws=b.ws)
        return out

    if pr.is_ca:
        # dq of softmax(q E^T / sqrt(dh)) E over the whole embedding table, then dW_q = dq^T post
        dq = buf("f32t_ca_dq", (Rap, Do), f32)
        ops.f32_ca_attn_bwd(a["q"], llm.embed, a["out"], dy2, a["lse"], dq, Rap, geo.ca_heads, ws=a["ca_ws"])
        wgrad(dq, d["post"], "W_q.weight")
    elif pr.has_norm:
        _projector_backward_linear_silu(model, st, dy2, wgrad, dgrad)
    else:
        # linear: [k frames] -> Linear -> ReLU -> Linear;  cov1d-linear: Conv1d over the k-frame rows -> ReLU -> the same
        ops.f32_colsum(dy2, pr.view(pr.g, pr.n_b2), Rap, Do)
        wgrad(dy2, a["h"], pr.n_w2)
        dh = dgrad(dy2, pr.n_w2, "w2")
        ops.f32_relu_bwd(a["h"], dh, dh)
        ops.f32_colsum(dh, pr.view(pr.g, pr.n_b1), Rap, pr.Hb)
        wgrad(dh, a["x1"], pr.n_w1)
        if pr.has_conv:
            dc0 = dgrad(dh, pr.n_w1, "w1")
            ops.f32_relu_bwd(a["x1"], dc0, dc0)
            ops.f32_colsum(dc0, pr.view(pr.g, "conv1d.bias"), Rap, Kp)
            wgrad(dc0, a["xcat"], "conv1d.weight")
    if on_ready is not None:
        on_ready(0, pr.numel)


# ------------------------------------------------------------------------------------------------ LoRA (use_peft = true) in fp32
class LoraF32:
    """The adapters of an adapted decoder in the fp32 training step.  In training mode peft's lora.Linear runs UNMERGED,
    y = W x + s B (A drop(x)) (a dropout mask cannot be merged into W), so the step's forward runs every adapted Linear on the base
    fp32 weights and adds the low-rank branch; eval mode and generate() keep the merged W + s B A (lora.merged_llm_f32).

    forward, per adapted Linear t of a group:   us_t = drop(x) (s A_t)^T  [M, r]   (kept per layer: 4 r bytes per row and target)
                                                y[:, cols of t] += us_t B_t^T
    backward, from the group's output gradient: v = dy_t (s B_t)  [M, r];   dx += mask . (v A_t);   dB_t = dy_t^T us_t;   dA_t = v^T drop(x)
    The adapter inputs are not stored: drop(x) is rebuilt in the backward from what the step keeps anyway (the residual stream ->
    RMSNorm, the attention output, gate|up -> SwiGLU) and the counter-based mask of the forward (tasu_f32_lora_dropout: the masks of
    the bf16 step, regenerated from {seed, step, stream id, element index}) -- the same bits as the forward's, no [L, M, in] copies.
    Every thin product ([M, r], r = 8..64) is tasu_f32_gemm_nt: it serves any M and N, its K granule is 32, so operands whose
    contraction runs over the rank are zero-padded to rk = 32-multiples (working copies below) and the accumulate y += us B^T is
    its ``resid`` aliasing C; the weight gradients contract the M rows (both operands transposed, rows zero-padded to 32)."""

    def __init__(self, model):
        self.m, self.lp = model, model.lora
        self.members = dict(self.lp.groups)                # adapted group -> its adapted members (train_bf16's runner has the same)
        self.rk = rup(self.lp.r, 32)
        self.version = -1
        self.w = {}

    def weights(self):
        """fp32 working copies from the master adapters, rebuilt when they changed (lp.version: a load, an optimizer step):
        sA [r, in], Bp [out, rk] (rank columns zero-padded), sBt [r, out] = s B^T, At [in, rk] = A^T zero-padded."""
        lp = self.lp
        if self.version == lp.version:
            return self.w
        p, s, r, rk = lp.proj.p, float(lp.cfg.scaling), lp.r, self.rk
        for l in range(self.m.geo.llm_layers):
            for t in lp.cfg.target_modules:
                (i, o), A, B = lp.dims[t], lp.view(p, l, t, "A"), lp.view(p, l, t, "B")
                w = self.w.get((l, t))
                if w is None:
                    z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=p.device)
                    w = self.w[(l, t)] = dict(sA=z(r, i), Bp=z(o, rk), sBt=z(r, o), At=z(i, rk))
                w["sA"].copy_(A).mul_(s)
                w["Bp"][:, :r].copy_(B)
                w["sBt"].copy_(B.t()).mul_(s)
                w["At"][:, :r].copy_(A.t())
        self.version = lp.version
        return self.w

    def _us(self, t, M):
        """[L, M, rk] rank activations of target t, kept for the backward; the pad columns [r, rk) are zero."""
        m, name = self.m, "f32t_lora_us_" + t
        before = m._ws.get(name)
        buf = m._buf(name, (m.geo.llm_layers, M, self.rk), torch.float32)
        if before is not m._ws[name]:
            m._ws[name].zero_()
        return buf

    def _dropped(self, l, t, x, M, width, drop):
        if not drop:
            return x
        xd = self.m._buf("f32t_lora_xd", (M, width), torch.float32)
        self.m.ops.f32_lora_dropout(x, xd, M, width, self.lp.cfg.lora_dropout, self.lp.rng, self.lp.sid(l, t))
        return xd

    def forward(self, l, gname, x, y, M, ws, drop):
        """y [M, nout of the group] (the base Linear's output, bias / residual included) += every member's low-rank branch."""
        lp, ops, W = self.lp, self.m.ops, self.weights()
        for t in self.members.get(gname, ()):
            (i, o), c0, w = lp.dims[t], lp.cols[t], W[(l, t)]
            us = self._us(t, M)[l]
            ops.f32_gemm(self._dropped(l, t, x, M, i, drop), w["sA"], us, M, lp.r, i, ws=ws)
            ops.f32_gemm(us, w["Bp"], y[:, c0:c0 + o], M, o, self.rk, resid=y[:, c0:c0 + o], ws=ws)

    def backward(self, l, gname, x, dy, dx_base, M, ws, drop):
        """dy [M, nout of the group]; x: the group's (undropped) input [M, in]; dx_base [M, in] += every member's input gradient;
        dA / dB of the members into the adapter tail of the bucket: full_ft.f32_wgrad's composed route spelt out here, because the
        members share dy_t (and x_t, where dropout gives them no input of their own): the helper per member would add launches."""
        lp, m, ops, W = self.lp, self.m, self.m.ops, self.weights()
        targets = self.members.get(gname, ())
        if not targets:
            return
        f32, r, rk, Mp = torch.float32, lp.r, self.rk, rup(M, 32)
        p, g = lp.cfg.lora_dropout, lp.proj.g
        inn, width = lp.dims[targets[0]][0], dy.shape[1]
        dy_t = m._buf("f32t_lora_dy_t", (width, Mp), f32)
        ops.f32_transpose(dy, dy_t, M, width, Mp)
        v = m._buf("f32t_lora_v", (M, rk), f32)
        if rk != r:
            v[:, r:].zero_()
        x_t, last = m._buf("f32t_lora_x_t", (inn, Mp), f32), None
        r_t = m._buf("f32t_lora_r_t", (rk, Mp), f32)
        for t in targets:
            (i, o), c0, w = lp.dims[t], lp.cols[t], W[(l, t)]
            ops.f32_gemm(dy[:, c0:c0 + o], w["sBt"], v, M, r, o, ws=ws)                        # v = dy_t (s B)
            if drop:                                                                           # dx += mask . (v A)
                tmp = m._buf("f32t_lora_tmp", (M, i), f32)
                ops.f32_gemm(v, w["At"], tmp, M, i, rk, ws=ws)
                ops.f32_lora_dropout(tmp, dx_base, M, i, p, lp.rng, lp.sid(l, t), accumulate=True)
            else:
                ops.f32_gemm(v, w["At"], dx_base, M, i, rk, resid=dx_base, ws=ws)
            ops.f32_transpose(self._us(t, M)[l], r_t, M, rk, Mp)
            ops.f32_gemm(dy_t[c0:c0 + o], r_t, lp.view(g, l, t, "B"), o, r, Mp, ws=ws)         # dB = dy_t^T us
            xd = self._dropped(l, t, x, M, i, drop)
            if drop or last is None:                                                           # members share x unless dropout gave each its own
                ops.f32_transpose(xd, x_t, M, i, Mp)
                last = xd
            ops.f32_transpose(v, r_t, M, rk, Mp)
            ops.f32_gemm(r_t, x_t, lp.view(g, l, t, "A"), r, i, Mp, ws=ws)                     # dA = v^T drop(x)


def lora_f32(model):
    run = getattr(model, "_lora_f32", None)
    if run is None or run.lp is not model.lora:
        run = model._lora_f32 = LoraF32(model)
    return run


def _projector_backward_linear_silu(model, st, dy2, wgrad, dgrad):
    """LayerNorm -> Linear -> SiLU -> Linear (the shipped projector) from the output rows' gradient dy2; ``wgrad`` / ``dgrad``:
    backward_fp32's helpers for a Linear of the projector."""
    ops, pr, d = model.ops, model.proj, st.dev
    a = d["f32t"]
    ops.f32_colsum(dy2, pr.view(pr.g, pr.n_b2), st.Rap, pr.Do)
    wgrad(dy2, a["h"], pr.n_w2)                                                              # dW2 = dy2^T h
    dh = dgrad(dy2, pr.n_w2, "w2")
    ops.f32_silu(a["h_pre"], dh, dy=dh)                                                      # dh_pre, in place
    ops.f32_colsum(dh, pr.view(pr.g, pr.n_b1), st.Rap, pr.Hb)
    wgrad(dh, a["xn_p"], pr.n_w1)                                                            # dW1 = dh_pre^T xn
    dxn = dgrad(dh, pr.n_w1, "w1")
    ops.f32_layernorm_bwd_params(dxn, d["post"], a["mean"], a["rstd"], pr.view(pr.g, "norm.weight"), pr.view(pr.g, "norm.bias"), st.Rap, pr.K)
