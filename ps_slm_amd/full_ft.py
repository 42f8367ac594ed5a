"""Full fine-tuning of the decoder (train_config.freeze_llm = false without use_peft; Multitask/model/ps-slm.py:105-108 leaves every
parameter of Qwen2ForCausalLM trainable, checkpoint_handler.py:214 saves them): where the LLM's tensors live in the flat trainable
bucket, their weight gradients, the copies that follow an optimizer step, and their names in a checkpoint.  The role
ps_slm_amd/lora.py plays for the adapters.

Bucket (``TasuModel.proj``: p / g / m / v fp32 and pb, the bf16 image AdamW writes):
    [projector | model.norm | lm_head (untied only) | layer L-1 | ... | layer 0 | embedding table]
every tensor starts on a multiple of 64 elements (the gaps hold zeros: zero gradient, zero value, AdamW leaves them zero).  A
layer is [down | gate|up | post_attention_layernorm | o | q|k|v weight | q|k|v bias | input_layernorm] -- on a Qwen3 geometry
(``geo.qk_norm``) [down | gate|up | post_attention_layernorm | o | q_norm | k_norm | q|k|v weight | input_layernorm]: the two [128]
head-norm weights where the backward completes them and no bias (qkv_bias is false: the zero bias LLMWeights keeps for its consumers
stays frozen, outside the bucket and every state dict) -- the order in which the backward completes them, layers last to first, so that ``grad_ranges()`` hands the engine contiguous ranges in completion order.
q|k|v and gate|up stay fused as the kernels read them; the reference's per-module names are row blocks of the fused tensors.  The
embedding table goes last and IS the use_emb mechanism (TasuModel.enable_embedding_training: lookup term + the tied head's term).

``LLMWeights``' tensors become views: the bf16 Linear weights and the q|k|v bias of ``pb``, the fp32 norm weights of ``p``.  The
forward and the dgrads read them as before; what is derived from them -- the transposed copies for the dgrads, the untied head's
transpose, the fragment-order decode copies and the decode graphs -- follows every optimizer step and load (``refresh``).

Weight gradients (fp32, straight into the bucket): dW = dY^T X by tasu_gemm_tn_bf16 from the row-major bf16 operands the step keeps
(the normed inputs, the attention output, the SwiGLU output: per layer in this mode), the q|k|v bias by tasu_colsum_bf16_split of dqkv
behind the RoPE backward, the norm weights by tasu_rmsnorm_wgrad from exactly what tasu_rmsnorm_bwd reads, Qwen3's q_norm / k_norm
by tasu_qk_norm_wgrad (tasu_f32_qk_norm_wgrad on the fp32 step) from what tasu_qk_norm_bwd reads, before it overwrites dqkv.  On the main stream,
next to the dgrad that consumes the same dY.

On the fp32 training step (``arith_train == "fp32"``: use_fp16 = false) the bucket layout is the same, and the masters ARE the weights:
``llm.f32["layers"][l][wqkv | bqkv | wo | wgu | wd]`` and the untied ``llm.f32["head"]`` become views of ``p`` (the separately allocated
fp32 copies are released; the bf16 views of ``pb`` stay, AdamW keeps writing the image), the weight gradients come from the fp32
operands of ps_slm_amd/train_fp32.py by csrc/wgrad_f32.hip (``wgrad32`` -- per tensor on the faster of tasu_f32_gemm_tn and the composed
route --, ``bias_wgrad32``, ``norm_wgrad32``), and after a step the
fp32 transposed copies of the dgrads are redone in place and the fp32 fragment-order decode copies dropped."""
import numpy as np
import torch

from .model import rup

HD = 128
PRE = "llm."
EMBED_KEY = PRE + "model.embed_tokens.weight"
HEAD_KEY = PRE + "lm_head.weight"
NORM_KEY = PRE + "model.norm.weight"
LAYER_ORDER = ("wd", "wgu", "ln2", "wo", "wqkv", "bqkv", "ln1")     # completion order of one layer's gradients
QK_NORM_LAYER_ORDER = ("wd", "wgu", "ln2", "wo", "q_norm", "k_norm", "wqkv", "ln1")     # ... of a Qwen3 layer: head norms, no q|k|v bias
F32_TENSORS = ("ln1", "ln2", "q_norm", "k_norm")                     # read from the fp32 masters; the others from the bf16 image


def is_llm_key(k):
    return k.startswith(PRE + "model.") or k == HEAD_KEY


class LLMTrainables:
    def __init__(self, model):
        geo, pr = model.geo, model.proj
        self.model, self.geo = model, geo
        self.tn_min_split = 3                                # wgrad(): tasu_gemm_tn_bf16 from this many row ranges on (tests: 1 / 99 force a route)
        # wgrad32(): the route of every fused tensor's weight gradient on the fp32 step, the faster one measured per shape at
        # Qwen2.5-1.5B (other geometries: not measured, the same map); f32_route = "tn" / "composed" forces one (tests)
        self.f32_routes = {"wqkv": "composed", "wo": "tn", "wgu": "tn", "wd": "composed", "head": "tn"}
        self.f32_route = None
        D, I, H, G, V, L = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_vocab, geo.llm_layers
        if D % 8 or I % 8:
            raise NotImplementedError(f"freeze_llm=false: llm_dim {D} / intermediate_size {I} must be multiples of 8 (tasu_gemm_tn_bf16)")
        if self.fp32 and V % 4:
            raise NotImplementedError(f"freeze_llm=false on the fp32 step: vocabulary size {V} must be a multiple of 4 (tasu_f32_gemm_tn)")
        Q, KV = H * HD, G * HD
        # a Qwen3 layer (geo.qk_norm) carries the two head-norm weights where a Qwen2 layer carries the q|k|v bias; its zero bias
        # stays a frozen tensor of LLMWeights, outside the bucket and every state dict
        self.layer_order = QK_NORM_LAYER_ORDER if geo.qk_norm else LAYER_ORDER
        self.shapes = {"wd": (D, I), "wgu": (2 * I, D), "ln2": (D,), "wo": (D, Q), "wqkv": (Q + 2 * KV, D), "bqkv": (Q + 2 * KV,), "ln1": (D,),
                       "q_norm": (HD,), "k_norm": (HD,)}
        # reference module name -> (fused tensor, first row, rows)
        self.parts = {
            "input_layernorm.weight": ("ln1", 0, D), "post_attention_layernorm.weight": ("ln2", 0, D),
            "self_attn.q_proj.weight": ("wqkv", 0, Q), "self_attn.k_proj.weight": ("wqkv", Q, KV), "self_attn.v_proj.weight": ("wqkv", Q + KV, KV),
            "self_attn.q_proj.bias": ("bqkv", 0, Q), "self_attn.k_proj.bias": ("bqkv", Q, KV), "self_attn.v_proj.bias": ("bqkv", Q + KV, KV),
            "self_attn.o_proj.weight": ("wo", 0, D),
            "mlp.gate_proj.weight": ("wgu", 0, I), "mlp.up_proj.weight": ("wgu", I, I), "mlp.down_proj.weight": ("wd", 0, D),
        }
        if geo.qk_norm:
            self.parts = {k: v for k, v in self.parts.items() if v[0] != "bqkv"}
            self.parts.update({"self_attn.q_norm.weight": ("q_norm", 0, HD), "self_attn.k_norm.weight": ("k_norm", 0, HD)})
        self.lo = pr.numel                                   # the projector's tensors end here (proj_end)
        off = rup(pr.numel, 64)
        self.offsets = {}                                    # (name, layer or None) -> (offset, shape)

        def put(key, shape):
            nonlocal off
            self.offsets[key] = (off, shape)
            off += rup(int(np.prod(shape)), 64)

        put(("norm", None), (D,))
        if not geo.tied:
            put(("head", None), (V, D))
        self.layers_lo = off
        self.layer_range = [None] * L
        for l in range(L - 1, -1, -1):
            lo = off
            for n in self.layer_order:
                put((n, l), self.shapes[n])
            self.layer_range[l] = (lo, off)
        self.end = off
        pr.extend(self.end - pr.numel)

    @property
    def fp32(self):
        """The decoder trains on the fp32 step: the forward reads the fp32 masters themselves."""
        return self.model.arith_train == "fp32"

    # ---- views
    def view(self, flat, name, layer=None):
        off, shp = self.offsets[(name, layer)]
        return flat[off:off + int(np.prod(shp))].view(*shp)

    def num_parameters(self):
        return sum(int(np.prod(s)) for _, s in self.offsets.values())

    def grad_ranges(self):
        """[norm | head] (with the alignment gap behind the projector), then one range per layer, last layer first."""
        L = self.geo.llm_layers
        return [(self.lo, self.layers_lo)] + [self.layer_range[l] for l in range(L - 1, -1, -1)]

    def names(self):
        """(checkpoint key, fused tensor, layer, first row, rows) of every tensor but the embedding table, in the reference's module
        order."""
        out = []
        for l in range(self.geo.llm_layers):
            for mod, (n, r0, nr) in self.parts.items():
                out.append((f"{PRE}model.layers.{l}.{mod}", n, l, r0, nr))
        out.append((NORM_KEY, "norm", None, 0, self.geo.llm_dim))
        if not self.geo.tied:
            out.append((HEAD_KEY, "head", None, 0, self.geo.llm_vocab))
        return out

    def named_views(self, flat):
        for key, n, l, r0, nr in self.names():
            yield key, self.view(flat, n, l)[r0:r0 + nr]

    # ---- weights in, views out
    def adopt(self, sd=None):
        """Moves the decoder's tensors into the bucket -- from the fp32 tensors of ``sd`` (reference names) when given, else from
        the bf16 copies LLMWeights holds -- and re-points LLMWeights at the bucket.  Every captured graph and decode copy refers to
        the old tensors and is dropped; the caller runs sync_projector_copies() afterwards."""
        m = self.model
        llm, pr, dev = m.llm, m.proj, m.device
        f = lambda t: t.to(dev, torch.float32)
        f32w = llm.f32 if self.fp32 and llm.f32 else None              # fp32 step: masters from (and then instead of) the fp32 copies
        for l, w in enumerate(llm.layers):
            if sd is not None:
                for mod, (n, r0, nr) in self.parts.items():
                    self.view(pr.p, n, l)[r0:r0 + nr].copy_(f(sd[f"{PRE}model.layers.{l}.{mod}"]))
            else:
                for n in self.layer_order:
                    if w[n].data_ptr() != self.view(pr.p if n in F32_TENSORS else pr.pb, n, l).data_ptr():
                        src = f32w["layers"][l].get(n, w[n]) if f32w is not None else w[n]
                        if src.data_ptr() != self.view(pr.p, n, l).data_ptr():
                            self.view(pr.p, n, l).copy_(f(src))
            for n in self.layer_order:
                new = self.view(pr.p if n in F32_TENSORS else pr.pb, n, l)
                if n in ("wqkv", "wo", "wgu", "wd") and w[n].data_ptr() != new.data_ptr():
                    llm._stale_ptrs.append(w[n].data_ptr())          # its fragment-order decode copy dies with it
                w[n] = new
            if f32w is not None:
                for n in self.layer_order:
                    if n not in ("ln1", "ln2"):                        # (the fp32 paths read the layer norms from LLMWeights.layers)
                        f32w["layers"][l][n] = self.view(pr.p, n, l)
        norm = self.view(pr.p, "norm")
        if sd is not None:
            norm.copy_(f(sd[NORM_KEY]))
        elif llm.norm.data_ptr() != norm.data_ptr():
            norm.copy_(f(llm.norm))
        llm.norm = norm
        if not self.geo.tied:
            head = self.view(pr.pb, "head")
            if sd is not None:
                self.view(pr.p, "head").copy_(f(sd.get(HEAD_KEY, sd[EMBED_KEY])))
            elif llm.head.data_ptr() != head.data_ptr():
                src = f32w["head"] if f32w is not None and f32w.get("head") is not None else llm.head
                if src.data_ptr() != self.view(pr.p, "head").data_ptr():
                    self.view(pr.p, "head").copy_(f(src))
                llm._stale_ptrs.append(llm.head.data_ptr())
            llm.head = head
            if f32w is not None:
                f32w["head"] = self.view(pr.p, "head")
        if f32w is not None:                                            # copies derived from the replaced fp32 tensors
            for k in ("t", "frag", "frag_head"):
                f32w.pop(k, None)
        llm._decode_ready = False
        m._graphs.clear()
        m._dec_graphs.clear()

    def load(self, key, t):
        """One checkpoint tensor (reference name and shape) into its fp32 master; the caller runs sync_projector_copies()."""
        for k, v in self.named_views(self.model.proj.p):
            if k == key:
                v.copy_(t.to(self.model.device, torch.float32))
                return
        raise KeyError(key)

    def state_dict(self):
        return {k: v.detach().clone() for k, v in self.named_views(self.model.proj.p)}

    def grads(self):
        return {k: v.detach().clone() for k, v in self.named_views(self.model.proj.g)}

    def refresh_working_copies(self, ops):
        """After the bucket's bf16 image changed (an optimizer step, a load): the transposed copies the dgrads read, the untied
        head's transpose, and the decode step's fragment-order copies (dropped here, registered again by the next generate(); the
        decode graphs hold their addresses).  The embedding table's own copies follow in TasuModel._embed_changed."""
        m = self.model
        llm, geo = m.llm, self.geo
        for w in llm.layers:
            for n in ("wqkv", "wo", "wgu", "wd"):
                N, K = w[n].shape
                ops.transpose(w[n], w[n + "_t"], N, K, N, K)
        ptrs = [w[n].data_ptr() for w in llm.layers for n in ("wqkv", "wo", "wgu", "wd")]
        if not geo.tied:
            V, D = geo.llm_vocab, geo.llm_dim
            ops.transpose(llm.head, llm.head_t, V, D, rup(V, 64), D)
            ptrs.append(llm.head.data_ptr())
        if hasattr(ops, "forget_decode_weights"):
            ops.forget_decode_weights(ptrs)
        llm._decode_ready = False
        m._dec_graphs.clear()
        if self.fp32 and llm.f32:
            # the fp32 paths: the dgrads' transposed copies follow in place (tasu_f32_transpose; the tied head's in _embed_changed);
            # the fragment-order decode copies are dropped and made again by the next generate()
            t = llm.f32.get("t")
            if t is not None:
                for f, ft in zip(llm.f32["layers"], t["layers"]):
                    for n in ("wqkv", "wo", "wgu", "wd"):
                        N, K = f[n].shape
                        ops.f32_transpose(f[n], ft[n], N, K, N)
                if not geo.tied and t.get("head") is not None:
                    ops.f32_transpose(llm.f32["head"], t["head"], geo.llm_vocab, geo.llm_dim, t["head"].shape[1])
            llm.f32.pop("frag", None)
            if not geo.tied:
                llm.f32.pop("frag_head", None)

    # ---- the backward's weight-gradient calls
    def wgrad(self, dy, x, name, layer):
        """g[name] = dy^T x (fp32, overwriting).  Two routes, chosen per shape by what was measured on MI355X:
        tasu_gemm_tn_bf16 where the output has so few tiles that it is cut into ``tn_min_split`` or more row ranges (o_proj at
        Qwen2.5-1.5B, everything at the test geometries), else the composed route -- two transposes + the NT GEMM with fp32
        output -- whose 256-wide tiles win on the large outputs."""
        from .ops import GEMM_F32
        m = self.model
        ops = m.ops
        N, K = self.shapes[name]
        R = dy.shape[0]
        dst = self.view(m.proj.g, name, layer)
        ns = ops.gemm_tn_split(R, N, K)
        if ns >= self.tn_min_split:
            ws = m._buf("wgrad_tn_ws", (ns * N * K,), torch.float32) if ns > 1 else None
            return ops.gemm_tn(dy, x, dst, R, N, K, accumulate=False, nsplit=ns, ws=ws)
        Rp = rup(R, 64)
        dy_t = m._buf("wgrad_dy_t", (N, Rp), torch.bfloat16)
        x_t = m._buf("wgrad_x_t", (K, Rp), torch.bfloat16)
        ops.transpose(dy, dy_t, R, N, Rp, N)
        ops.transpose(x, x_t, R, K, Rp, K)
        ops.gemm(dy_t, x_t, dst, N, K, Rp, mode=GEMM_F32)

    def bias_wgrad(self, dy, name, layer):
        """g[name] = the column sums of dy (the q|k|v bias: dqkv behind the RoPE backward)."""
        from .ops import RMS_WGRAD_SPLIT
        m = self.model
        R, C = dy.shape
        ws = m._buf("wgrad_bias_ws", (RMS_WGRAD_SPLIT * C,), torch.float32)
        m.ops.colsum_split(dy, self.view(m.proj.g, name, layer), ws, R, C)

    def norm_wgrad(self, dy, x, rstd, name, layer, src_rows=None):
        from .ops import RMS_WGRAD_SPLIT
        m = self.model
        ws = m._buf("wgrad_rms_ws", (RMS_WGRAD_SPLIT * self.geo.llm_dim,), torch.float32)
        m.ops.rmsnorm_wgrad(dy, x, rstd, self.view(m.proj.g, name, layer), ws, src_rows=src_rows, accumulate=False)

    def qk_wgrad(self, dqkv, pre, rstd, layer):
        """g[q_norm], g[k_norm] of a Qwen3 layer = sum over rows and heads of dqkv * (pre * rstd), from what the head norm's backward
        reads and BEFORE it overwrites dqkv (tasu_qk_norm_wgrad on the bf16 step, tasu_f32_qk_norm_wgrad on the fp32 step)."""
        from .ops import QK_WGRAD_SPLIT
        m, geo = self.model, self.geo
        ws = m._buf("wgrad_qk_ws", (QK_WGRAD_SPLIT * 2 * HD,), torch.float32)
        op = m.ops.f32_qk_norm_wgrad if self.fp32 else m.ops.qk_norm_wgrad
        op(dqkv, pre, rstd, self.view(m.proj.g, "q_norm", layer), self.view(m.proj.g, "k_norm", layer), ws, dqkv.shape[0], geo.llm_heads,
           geo.llm_kv_heads, accumulate=False)

    # ---- ... on the fp32 step (ps_slm_amd/train_fp32.py backward_fp32)
    def wgrad32(self, dy, x, name, layer=None, dst=None):
        """g[name] [N, K] = dy^T x from the fp32 operands (overwriting) on the route ``f32_routes`` keeps for it; ``dst``: another
        destination of the same shape (the tied table's range for the head term).  See ``f32_wgrad``."""
        f32_wgrad(self.model, dy, x, self.view(self.model.proj.g, name, layer) if dst is None else dst, self.f32_route or self.f32_routes[name])

    def bias_wgrad32(self, dy, name, layer):
        from .ops import RMS_WGRAD_SPLIT
        m = self.model
        R, C = dy.shape
        ws = m._buf("f32t_wgrad_bias_ws", (RMS_WGRAD_SPLIT * C,), torch.float32)
        m.ops.f32_colsum_split(dy, self.view(m.proj.g, name, layer), ws, R, C)

    def norm_wgrad32(self, dy, x, name, layer):
        """g[name] = sum_r dy . x . rstd with rstd recomputed from x, as tasu_f32_rmsnorm_bwd does."""
        from .ops import RMS_WGRAD_SPLIT
        m = self.model
        R, D = dy.shape
        ws = m._buf("f32t_wgrad_rms_ws", (RMS_WGRAD_SPLIT * D + rup(R, 4),), torch.float32)
        m.ops.f32_rmsnorm_wgrad(dy, x, self.view(m.proj.g, name, layer), ws, self.geo.rms_eps)


def f32_wgrad(model, dy, x, dst, route="tn"):
    """dst [N, K] (fp32, overwriting) = dy[:, :N]^T x[:, :K] over all rows of the fp32 operands.  Two routes (DESIGN.md 4l has the
    measured times): "tn" = tasu_f32_gemm_tn on the row-major operands, cut into the row ranges its split plan gives; "composed" =
    the route the projector's weight gradients take -- two tasu_f32_transpose (rows zero-padded to 32, the NT GEMM's K granule) +
    tasu_f32_gemm_nt."""
    from .decode_fp32 import _gemm_ws
    ops = model.ops
    R = dy.shape[0]
    N, K = dst.shape
    if route == "tn":
        ns = ops.f32_gemm_tn_split(R, N, K)
        ws = model._buf("f32t_wgrad_tn_ws", (ns * N * K,), torch.float32) if ns > 1 else None
        return ops.f32_gemm_tn(dy, x, dst, R, N, K, accumulate=False, nsplit=ns, ws=ws)
    if route != "composed":
        raise ValueError(f"f32_wgrad: unknown route {route!r}")
    Rp = rup(R, 32)
    dy_t = model._buf("f32t_wgrad_dy_t", (N, Rp), torch.float32)
    x_t = model._buf("f32t_wgrad_x_t", (K, Rp), torch.float32)
    ops.f32_transpose(dy, dy_t, R, N, Rp)
    ops.f32_transpose(x, x_t, R, K, Rp)
    ops.f32_gemm(dy_t, x_t, dst, N, K, Rp, ws=_gemm_ws(model))
