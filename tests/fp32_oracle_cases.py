"""Seeded UNFILTERED decode cases for the fp32 path of the adapted decoder and the alternate projectors: every drawn prompt is
kept, and the float64 oracle (oracle/tasu_oracle.py, restating the reference's generate) decides which of them the comparison can
hold the GPU to -- those where its fp32 and float64 runs produce the same tokens (a case that flips between the two is a near-tie
no fp32 implementation can be held to)."""
import dataclasses

import numpy as np
import torch

from oracle import tasu_oracle as O

PLANS = [dict(num_beams=4, max_new_tokens=12), dict(num_beams=4, max_new_tokens=8, length_penalty=0.5), dict(num_beams=2, max_new_tokens=9),
         dict(num_beams=3, max_new_tokens=10, min_length=14), dict(num_beams=1, max_new_tokens=7), dict(num_beams=4, max_new_tokens=16)]


def draw_case(geo, seed, min_post=2):
    """(input_ids, attention_mask, post_ids, generate kwargs): 1-3 left-padded prompts with one speech token each."""
    rng = np.random.default_rng(seed)
    B = int(rng.integers(1, 4))
    rows = [rng.integers(0, 900, int(rng.integers(2, 9))).tolist() + [geo.speech_id] + rng.integers(0, 900, int(rng.integers(0, 4))).tolist()
            for _ in range(B)]
    L = max(len(r) for r in rows)
    ids = torch.tensor([[geo.eos_id] * (L - len(r)) + r for r in rows])
    am = torch.tensor([[0] * (L - len(r)) + [1] * len(r) for r in rows]).bool()
    post_ids = [rng.integers(1, geo.ctc_vocab, int(rng.integers(min_post, 13))).tolist() for _ in range(B)]
    kw = dict(PLANS[seed % len(PLANS)])
    kw.setdefault("min_length", 1)
    kw.setdefault("length_penalty", 1.0)
    return ids, am, post_ids, kw


def oracle_tokens(W, geo, ids, am, post_ids, kw, dtype):
    """The oracle's generate() on weights W, every tensor in ``dtype`` (fp32 arithmetic mode: nothing rounded to bf16)."""
    gd = dataclasses.asdict(geo)
    post, plen = O.pseudo_posterior(post_ids, geo.ctc_vocab)
    post = post.to(dtype)
    proj = O.projector(W, post, "fp32")
    if "encoder_projector.conv1d.weight" in W:
        plen = plen // W["encoder_projector.conv1d.weight"].shape[2]
    elif "encoder_projector.linear1.weight" in W:
        plen = plen // (W["encoder_projector.linear1.weight"].shape[1] // post.shape[-1])
    emb, mask, _, _ = O.merge(proj, plen, W["llm.model.embed_tokens.weight"][ids], ids, am, None, geo.speech_id)
    return O.beam_search_generate(W, emb.detach(), mask, gd, mode="fp32", kv_cache=True, eos_token_id=geo.eos_id,
                                  pad_token_id=geo.eos_id, **kw)


def lora_merged_double(sd, lsd, cfg):
    """{name: float64 tensor} with W + s B A on every adapted Linear (the adapters merged in float64)."""
    from ps_slm_amd.lora import key_of
    W = {k: v.double() for k, v in sd.items()}
    parent = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn", "gate_proj": "mlp",
              "up_proj": "mlp", "down_proj": "mlp"}
    n_layers = len({k.split(".")[3] for k in sd if k.startswith("llm.model.layers.")})
    for l in range(n_layers):
        for t in cfg.target_modules:
            k = f"llm.model.layers.{l}.{parent[t]}.{t}.weight"
            W[k] = W[k] + cfg.scaling * (lsd[key_of(l, t, "B")].double() @ lsd[key_of(l, t, "A")].double())
    return W


def compare(gen_gpu, W64, geo, seeds, min_post=2):
    """Runs every seeded case on the GPU (gen_gpu(ids, am, post_ids, kw) -> tokens) and on the oracle in fp32 and float64.
    Returns (number of qualifying cases, [(seed, gpu, float64) of qualifying cases where the GPU differs])."""
    W32 = {k: v.float() for k, v in W64.items()}
    n_ok, bad = 0, []
    for seed in seeds:
        ids, am, post_ids, kw = draw_case(geo, seed, min_post)
        t32 = oracle_tokens(W32, geo, ids, am, post_ids, kw, torch.float32)
        t64 = oracle_tokens(W64, geo, ids, am, post_ids, kw, torch.float64)
        if t32.shape != t64.shape or not torch.equal(t32, t64):
            continue
        n_ok += 1
        got = gen_gpu(ids, am, post_ids, kw)
        if got.shape != tuple(t64.shape) or not np.array_equal(got, t64.numpy()):
            bad.append((seed, got.tolist(), t64.tolist()))
    return n_ok, bad
