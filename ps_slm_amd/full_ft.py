"""Full fine-tuning of the decoder (train_config.freeze_llm = false without use_peft; Multitask/model/ps-slm.py:105-108 leaves every
parameter of Qwen2ForCausalLM trainable, checkpoint_handler.py:214 saves them): where the LLM's tensors live in the flat trainable
bucket, their weight gradients, the copies that follow an optimizer step, and their names in a checkpoint.  The role
ps_slm_amd/lora.py plays for the adapters.

Bucket (``TasuModel.proj``: p / g / m / v fp32 and pb, the bf16 image AdamW writes):
    [projector | model.norm | lm_head (untied only) | layer L-1 | ... | layer 0 | embedding table]
every tensor starts on a multiple of 64 elements (the gaps hold zeros: zero gradient, zero value, AdamW leaves them zero).  A
layer is [down | gate|up | post_attention_layernorm | o | q|k|v weight | q|k|v bias | input_layernorm] -- the order in which the
backward completes them, layers last to first, so that ``grad_ranges()`` hands the engine contiguous ranges in completion order.
q|k|v and gate|up stay fused as the kernels read them; the reference's per-module names are row blocks of the fused tensors.  The
embedding table goes last and IS the use_emb mechanism (TasuModel.enable_embedding_training: lookup term + the tied head's term).

``LLMWeights``' tensors become views: the bf16 Linear weights and the q|k|v bias of ``pb``, the fp32 norm weights of ``p``.  The
forward and the dgrads read them as before; what is derived from them -- the transposed copies for the dgrads, the untied head's
transpose, the fragment-order decode copies and the decode graphs -- follows every optimizer step and load (``refresh``).

Weight gradients (fp32, straight into the bucket): dW = dY^T X by tasu_gemm_tn_bf16 from the row-major bf16 operands the step keeps
(the normed inputs, the attention output, the SwiGLU output: per layer in this mode), the q|k|v bias by tasu_colsum_bf16_split of dqkv
behind the RoPE backward, the norm weights by tasu_rmsnorm_wgrad from exactly what tasu_rmsnorm_bwd reads.  On the main stream,
next to the dgrad that consumes the same dY."""
import numpy as np
import torch

HD = 128
PRE = "llm."
EMBED_KEY = PRE + "model.embed_tokens.weight"
HEAD_KEY = PRE + "lm_head.weight"
NORM_KEY = PRE + "model.norm.weight"
LAYER_ORDER = ("wd", "wgu", "ln2", "wo", "wqkv", "bqkv", "ln1")     # completion order of one layer's gradients
F32_TENSORS = ("ln1", "ln2")                                         # read from the fp32 masters; the others from the bf16 image


def rup(x, m):
    return (x + m - 1) // m * m


def is_llm_key(k):
    return k.startswith(PRE + "model.") or k == HEAD_KEY


class LLMTrainables:
    def __init__(self, model):
        geo, pr = model.geo, model.proj
        self.model, self.geo = model, geo
        self.tn_min_split = 3                                # wgrad(): tasu_gemm_tn_bf16 from this many row ranges on (tests: 1 / 99 force a route)
        D, I, H, G, V, L = geo.llm_dim, geo.llm_inter, geo.llm_heads, geo.llm_kv_heads, geo.llm_vocab, geo.llm_layers
        if D % 8 or I % 8:
            raise NotImplementedError(f"freeze_llm=false: llm_dim {D} / intermediate_size {I} must be multiples of 8 (tasu_gemm_tn_bf16)")
        Q, KV = H * HD, G * HD
        self.shapes = {"wd": (D, I), "wgu": (2 * I, D), "ln2": (D,), "wo": (D, Q), "wqkv": (Q + 2 * KV, D), "bqkv": (Q + 2 * KV,), "ln1": (D,)}
        # reference module name -> (fused tensor, first row, rows)
        self.parts = {
            "input_layernorm.weight": ("ln1", 0, D), "post_attention_layernorm.weight": ("ln2", 0, D),
            "self_attn.q_proj.weight": ("wqkv", 0, Q), "self_attn.k_proj.weight": ("wqkv", Q, KV), "self_attn.v_proj.weight": ("wqkv", Q + KV, KV),
            "self_attn.q_proj.bias": ("bqkv", 0, Q), "self_attn.k_proj.bias": ("bqkv", Q, KV), "self_attn.v_proj.bias": ("bqkv", Q + KV, KV),
            "self_attn.o_proj.weight": ("wo", 0, D),
            "mlp.gate_proj.weight": ("wgu", 0, I), "mlp.up_proj.weight": ("wgu", I, I), "mlp.down_proj.weight": ("wd", 0, D),
        }
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
            for n in LAYER_ORDER:
                put((n, l), self.shapes[n])
            self.layer_range[l] = (lo, off)
        self.end = off
        pr.extend(self.end - pr.numel)

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
        for l, w in enumerate(llm.layers):
            if sd is not None:
                for mod, (n, r0, nr) in self.parts.items():
                    self.view(pr.p, n, l)[r0:r0 + nr].copy_(f(sd[f"{PRE}model.layers.{l}.{mod}"]))
            else:
                for n in LAYER_ORDER:
                    if w[n].data_ptr() != self.view(pr.p if n in F32_TENSORS else pr.pb, n, l).data_ptr():
                        self.view(pr.p, n, l).copy_(f(w[n]))
            for n in LAYER_ORDER:
                new = self.view(pr.p if n in F32_TENSORS else pr.pb, n, l)
                if n in ("wqkv", "wo", "wgu", "wd") and w[n].data_ptr() != new.data_ptr():
                    llm._stale_ptrs.append(w[n].data_ptr())          # its fragment-order decode copy dies with it
                w[n] = new
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
                self.view(pr.p, "head").copy_(f(llm.head))
                llm._stale_ptrs.append(llm.head.data_ptr())
            llm.head = head
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
