"""TEST HELPER (not a test, never shipped): the oracle's decoder (oracle/tasu_oracle.py: qwen2_hidden / qwen2_hidden_step) restated
for Qwen3 -- no q|k|v bias, an RMSNorm over each 128-wide q and k head between the projection and the rotation (transformers
modeling_qwen3.py: Qwen3Attention.q_norm / k_norm) -- in the oracle's two modes, built on its ``linear``, ``rbf``, ``rms_norm`` and
``apply_rope``.  mode "bf16" is HF's Qwen3RMSNorm under autocast: the statistic and x * r in fp32, rounded to bf16 (the cast back to
the input dtype), times the fp32 weight in fp32; the rotation in fp32 and one rounding behind it.

The loss / projector-gradient and generate loops are the oracle's own (forward_text, forward_audio, loss_and_projector_grads,
beam_search_generate): they reach the decoder through the module's names ``qwen2_hidden`` / ``qwen2_hidden_step``, which
``as_qwen3()`` points at the functions below for the length of a call.  ``variant``: "norm" (the model), "no-norm" (the head norm
left out) and "swapped" (q_norm and k_norm exchanged) -- the two mistakes the fixtures are built to see."""
import contextlib
import functools

import torch
import torch.nn.functional as F

from oracle import tasu_oracle as O
from oracle.tasu_oracle import apply_rope, linear, rbf, rms_norm

EPS = 1e-6


def head_norm(x, w, mode, eps=EPS):
    """x [..., heads, 128] (the projection's output), w [128]"""
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return w * rbf(x * r, mode)


def _qk(W, p, h, R, S, n_heads, n_kv, hd, cos, sin, mode, variant):
    q = linear(h, W[p + "self_attn.q_proj.weight"], None, mode).view(R, S, n_heads, hd)
    k = linear(h, W[p + "self_attn.k_proj.weight"], None, mode).view(R, S, n_kv, hd)
    v = linear(h, W[p + "self_attn.v_proj.weight"], None, mode).view(R, S, n_kv, hd).transpose(1, 2)
    wq, wk = W[p + "self_attn.q_norm.weight"], W[p + "self_attn.k_norm.weight"]
    if variant == "swapped":
        wq, wk = wk, wq
    if variant != "no-norm":
        q, k = head_norm(q, wq, mode), head_norm(k, wk, mode)
    q = rbf(apply_rope(q.transpose(1, 2), cos, sin), mode)
    k = rbf(apply_rope(k.transpose(1, 2), cos, sin), mode)
    return q, k, v


def _mlp(W, p, x, mode):
    h = rms_norm(x, W[p + "post_attention_layernorm.weight"])
    g = linear(h, W[p + "mlp.gate_proj.weight"], None, mode)
    u = linear(h, W[p + "mlp.up_proj.weight"], None, mode)
    return x + linear(rbf(rbf(F.silu(g), mode) * u, mode), W[p + "mlp.down_proj.weight"], None, mode)


def qwen3_hidden(W, emb, mask, position_ids, n_heads, n_kv, theta=1e6, mode="fp32", pre="llm.", return_kv=False, variant="norm"):
    """qwen2_hidden with Qwen3's attention block"""
    B, S, _ = emb.shape
    hd = W[pre + "model.layers.0.self_attn.q_proj.weight"].shape[0] // n_heads
    cos, sin = O.rope_tables(position_ids, hd, theta)
    allow = torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None] & mask.bool()[:, None, None, :]
    x, kvs, rep = emb, [], n_heads // n_kv
    for l in range(O.qwen2_geometry(W, pre)):
        p = f"{pre}model.layers.{l}."
        q, k, v = _qk(W, p, rms_norm(x, W[p + "input_layernorm.weight"]), B, S, n_heads, n_kv, hd, cos, sin, mode, variant)
        kvs.append((k, v))
        sc = (q @ k.repeat_interleave(rep, dim=1).transpose(-1, -2)) * hd ** (-0.5)
        pr = torch.nan_to_num(torch.softmax(sc.masked_fill(~allow, float("-inf")), dim=-1), nan=0.0)
        a = rbf(rbf(pr, mode) @ v.repeat_interleave(rep, dim=1), mode).transpose(1, 2).reshape(B, S, n_heads * hd)
        x = x + linear(a, W[p + "self_attn.o_proj.weight"], None, mode)
        x = _mlp(W, p, x, mode)
    x = rms_norm(x, W[pre + "model.norm.weight"])
    return (x, kvs) if return_kv else x


def qwen3_hidden_step(W, x, kvs, key_mask, position_ids, n_heads, n_kv, theta=1e6, mode="fp32", pre="llm.", variant="norm"):
    """qwen2_hidden_step with Qwen3's attention block"""
    R = x.shape[0]
    hd = W[pre + "model.layers.0.self_attn.q_proj.weight"].shape[0] // n_heads
    cos, sin = O.rope_tables(position_ids, hd, theta)
    allow, rep, out = key_mask.bool()[:, None, None, :], n_heads // n_kv, []
    for l in range(O.qwen2_geometry(W, pre)):
        p = f"{pre}model.layers.{l}."
        q, k, v = _qk(W, p, rms_norm(x, W[p + "input_layernorm.weight"]), R, 1, n_heads, n_kv, hd, cos, sin, mode, variant)
        k, v = torch.cat([kvs[l][0], k], 2), torch.cat([kvs[l][1], v], 2)
        out.append((k, v))
        sc = (q @ k.repeat_interleave(rep, dim=1).transpose(-1, -2)) * hd ** (-0.5)
        pr = torch.softmax(sc.masked_fill(~allow, float("-inf")), dim=-1)
        a = rbf(rbf(pr, mode) @ v.repeat_interleave(rep, dim=1), mode).transpose(1, 2).reshape(R, 1, n_heads * hd)
        x = x + linear(a, W[p + "self_attn.o_proj.weight"], None, mode)
        x = _mlp(W, p, x, mode)
    return rms_norm(x, W[pre + "model.norm.weight"]), out


@contextlib.contextmanager
def as_qwen3(variant="norm"):
    """the oracle's loops on the Qwen3 decoder for the length of the block"""
    keep = O.qwen2_hidden, O.qwen2_hidden_step
    O.qwen2_hidden = functools.partial(qwen3_hidden, variant=variant)
    O.qwen2_hidden_step = functools.partial(qwen3_hidden_step, variant=variant)
    try:
        yield O
    finally:
        O.qwen2_hidden, O.qwen2_hidden_step = keep


def forward_text(W, batch, geo, mode="fp32", variant="norm"):
    with as_qwen3(variant):
        return O.forward_text(W, batch, geo, mode)


def forward_audio(W, batch, geo, mode="fp32", variant="norm"):
    with as_qwen3(variant):
        return O.forward_audio(W, batch, geo, mode)


def loss_and_projector_grads(W, batch, geo, mode="fp32", audio=False, variant="norm"):
    with as_qwen3(variant):
        return O.loss_and_projector_grads(W, batch, geo, mode, audio=audio)


def beam_search_generate(W, emb, mask, geo, variant="norm", **kw):
    with as_qwen3(variant):
        return O.beam_search_generate(W, emb, mask, geo, **kw)


# ------------------------------------------------------------------------------------------------ the fixtures
def mid_qwen3_geometry():
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY
    return Geometry.from_dict(dict(MID_GEOMETRY, qk_norm=True, qkv_bias=False))


def step_case():
    """(geo, state dict with the encoder, batch, z) of tests/golden/mid_qwen3_step.npz (tools/make_golden_qwen3.py): z holds, for
    tag in (text, audio), {tag}_loss, {tag}_acc, {tag}_logits_cols (at z["cols"]) and {tag}_grad.<projector tensor> of the REAL
    reference in fp32 on ``batch`` (text: the clean posterior of batch["post_ids"]; audio: batch["input_features"])."""
    from conftest import load_npz
    from ps_slm_amd.synthetic import qwen3_state_dict, synthetic_text_batch
    z = load_npz("mid_qwen3_step")
    geo = mid_qwen3_geometry()
    sd = qwen3_state_dict(geo, int(z["seed_w"]), with_encoder=True, scale=float(z["scale"]))
    batch = synthetic_text_batch(geo, 3, seed=int(z["seed_b"]), prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12,
                                 noise=False, ragged=True)
    batch["input_features"] = torch.randn(3, 12, geo.feat_dim, generator=torch.Generator().manual_seed(int(z["feat_seed"]))).half().float()
    return geo, sd, batch, z


def generate_cases():
    """(geo, state dict, cases) of tests/golden/mid_qwen3_generate.npz: each case dict(ids, am, post_ids, kw, tokens, bf16_stable,
    swap_differs); tokens = the REAL reference's."""
    from conftest import load_npz, split_flat
    from ps_slm_amd.synthetic import qwen3_state_dict
    z = load_npz("mid_qwen3_generate")
    geo = mid_qwen3_geometry()
    sd = qwen3_state_dict(geo, int(z["seed_w"]), decode_fixture=True)
    cases = []
    for n in range(int(z["n_cases"])):
        nb, new, min_len = (int(v) for v in z[f"c{n}_kw"])
        cases.append(dict(ids=torch.from_numpy(z[f"c{n}_input_ids"]), am=torch.from_numpy(z[f"c{n}_attention_mask"]),
                          post_ids=split_flat(z[f"c{n}_post_ids_flat"], z[f"c{n}_post_lens"]), tokens=z[f"c{n}_tokens"],
                          bf16_stable=bool(z["bf16_stable"][n]), swap_differs=bool(z["swap_differs"][n]),
                          kw=dict(num_beams=nb, max_new_tokens=new, min_length=min_len, length_penalty=float(z[f"c{n}_length_penalty"]))))
    return geo, sd, cases


def knob_cases(cases):
    """(penalty case, sampled case) of mid_qwen3_generate.npz: copies of two of its cases with the knob's keywords and the bf16
    RESTATEMENT's jitter-stable tokens (tools/make_golden_qwen3.py: knob_cases) -- downstream of the logits, one of each."""
    from conftest import load_npz
    z = load_npz("mid_qwen3_generate")
    pen = dict(cases[int(z["pen_case"])], tokens=z["pen_tokens"])
    pen["kw"] = dict(pen["kw"], repetition_penalty=float(z["pen_penalty"]))
    smp = dict(cases[int(z["smp_case"])], tokens=z["smp_tokens"], manual_seed=int(z["smp_manual_seed"]))
    T, top_k, top_p = (float(v) for v in z["smp_kw"])
    smp["kw"] = dict(max_new_tokens=smp["kw"]["max_new_tokens"], min_length=smp["kw"]["min_length"], num_beams=1)
    smp["sampling"] = (T, int(top_k), top_p)
    return pen, smp


def decode_case(model, geo, c, graphs=None):
    """the product's decode loop on a fixture case (a penalty / sampled one included): numpy tokens"""
    from ps_slm_amd.decode import beam_search_generate, check_sampling
    kw = dict(c["kw"])
    if "sampling" in c:
        kw["sampling"] = check_sampling(*c["sampling"])
        torch.manual_seed(c["manual_seed"])
    st = model.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    model.forward_projector_text(st)
    keep = model.decode_graphs
    if graphs is not None:
        model.decode_graphs = graphs
    try:
        return beam_search_generate(model, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw).numpy()
    finally:
        model.decode_graphs = keep


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
