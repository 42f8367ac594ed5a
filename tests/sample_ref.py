"""TEST INFRASTRUCTURE ONLY -- generate(do_sample=True, num_beams=1) restated: HF's ``_sample`` loop (transformers generation/utils.py)
on the oracle's network functions, like tests/penalty_ref.py, with the logits processors and warpers in HF's order and HF's own torch
float32 expressions (logits_process.py: RepetitionPenaltyLogitsProcessor, MinLengthLogitsProcessor, TemperatureLogitsWarper,
TopKLogitsWarper, TopPLogitsWarper), the softmax, and -- in torch.multinomial's place -- the project's draw: inverse CDF in token-id
order with the counter-based uniform of (seed, position, row) (tests/sample_ref64.py).  The fixture generator
(tools/make_golden_generate_sample.py) puts the same draw into the REAL reference's call, so the tokens are comparable one by one.

A row that drew EOS is padded from then on; the loop ends when every row has, or at max_new_tokens.  ``mode`` "fp32" / "bf16",
``logit_jitter``, ``logits_trace`` / ``logits_replay`` as in tests/penalty_ref.py."""
import numpy as np
import torch

from penalty_ref import _network, penalise, prompt_embeddings, same  # noqa: F401
from sample_ref64 import inverse_cdf, uniforms


def warp(scores, temperature, top_k, top_p):
    """TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper (min_tokens_to_keep = 1) on [R, V] float32 scores."""
    scores = scores / temperature
    k = min(top_k, scores.size(-1))
    scores = scores.masked_fill(scores < torch.topk(scores, k)[0][..., -1, None], float("-inf"))
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        remove = sorted_logits.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        remove[..., -1:] = 0
        scores = scores.masked_fill(remove.scatter(1, sorted_indices, remove), float("-inf"))
    return scores


def draw(probs, seed, cur):
    """What stands in torch.multinomial's place at generated position ``cur``: LongTensor [R]."""
    u = uniforms(seed, cur, probs.shape[0])
    return torch.tensor([inverse_cdf(probs[r].numpy(), u[r]) for r in range(probs.shape[0])], dtype=torch.long)


def generate_sampled(W, emb, mask, geo, seed, max_new_tokens=200, min_length=1, repetition_penalty=1.0, temperature=1.0, top_k=50,
                     top_p=1.0, eos_token_id=None, pad_token_id=None, mode="fp32", logit_jitter=None, logits_trace=None,
                     logits_replay=None):
    """New tokens [B, n_new] (LongTensor); None when a replayed trace no longer matches the tokens drawn."""
    B, S, _ = emb.shape
    p = float(repetition_penalty)
    min_length = max(int(min_length) - S, 0)                      # HF: min_length counts the embedded prompt
    eos = geo["eos_id"] if eos_token_id is None else eos_token_id
    pad = eos if pad_token_id is None else pad_token_id
    seq = torch.full((B, max_new_tokens), pad, dtype=torch.long)
    alive = torch.ones(B, dtype=torch.bool)
    cur = 0
    while cur < max_new_tokens and bool(alive.any()):
        toks = seq[:, :cur]
        if logits_replay is not None:
            if cur >= len(logits_replay) or not torch.equal(logits_replay[cur][1], toks):
                return None
            lg = logits_replay[cur][0].clone()
        else:
            lg = _network(W, geo, emb, mask, toks, mode)
        if logits_trace is not None:
            logits_trace.append((lg.clone(), toks.clone()))
        if logit_jitter is not None:
            lg = logit_jitter(lg)
        sc = penalise(lg, toks, p)
        if cur < min_length:
            sc[:, eos] = float("-inf")
        probs = torch.softmax(warp(sc, temperature, top_k, top_p), dim=-1)
        tok = draw(probs, seed, cur)
        tok = torch.where(alive, tok, torch.full_like(tok, pad))
        seq[:, cur] = tok
        alive = alive & (tok != eos)
        cur += 1
    return seq[:, :cur]


def relative_jitter(seed, rel=2e-5):
    """A ``logit_jitter``: every logit moves by a uniform relative amount in [-rel, rel] -- the documented agreement of the fp32 path
    with the reference (sums in another order than the reference's BLAS)."""
    g = torch.Generator().manual_seed(seed)

    def jitter(logits):
        return logits * (1 + rel * (2 * torch.rand(logits.shape, generator=g) - 1))
    return jitter


def sample_cases():
    """(geo, state dict, cases) of tests/golden/mid_generate_sample.npz (tools/make_golden_generate_sample.py): each case
    dict(ids, am, post_ids, kw, manual_seed, seed, tokens, fp32_stable, bf16_stable) -- kw = the generate() keywords of the sampled
    call, ``manual_seed`` what torch.manual_seed receives before it, ``seed`` the 64-bit seed the call then draws, tokens = the REAL
    reference's."""
    from conftest import load_npz, split_flat
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, decode_fixture_state_dict

    z = load_npz("mid_generate_sample")
    geo = Geometry.from_dict(MID_GEOMETRY)
    sd = decode_fixture_state_dict(geo, int(z["seed_w"]))
    cases = []
    for n in range(int(z["n_cases"])):
        new, min_len, top_k = (int(v) for v in z[f"c{n}_kw"])
        T, top_p, pen = (float(v) for v in z[f"c{n}_kwf"])
        cases.append(dict(ids=torch.from_numpy(z[f"c{n}_input_ids"]), am=torch.from_numpy(z[f"c{n}_attention_mask"]),
                          post_ids=split_flat(z[f"c{n}_post_ids_flat"], z[f"c{n}_post_lens"]), tokens=z[f"c{n}_tokens"],
                          manual_seed=int(z[f"c{n}_manual_seed"]), seed=int(z[f"c{n}_seed"]),
                          fp32_stable=bool(z["fp32_stable"][n]), bf16_stable=bool(z["bf16_stable"][n]),
                          kw=dict(max_new_tokens=new, min_length=min_len, top_k=top_k, temperature=T, top_p=top_p, repetition_penalty=pen)))
    return geo, sd, cases


def draw_seed(manual_seed):
    """The 64-bit seed a sampled generate() call draws right after torch.manual_seed(manual_seed) (ps_slm_amd/decode.py: DeviceBeam)."""
    torch.manual_seed(manual_seed)
    return int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64))


def sampled_tokens_on_weights(W, geo, ids, am, post_ids, kw, seed, dtype):
    """generate_sampled on the weights W with every tensor in ``dtype`` (fp32 mode: nothing rounded to bf16) -- e.g. the LoRA-merged
    W + s B A of tests/fp32_oracle_cases.py::lora_merged_double in float32 and float64 (tests/penalty_ref.py::tokens_on_weights)."""
    import dataclasses

    from oracle import tasu_oracle as O
    W = {k: v.to(dtype) for k, v in W.items()}
    post, plen = O.pseudo_posterior(post_ids, geo.ctc_vocab)
    emb, mask, _, _ = O.merge(O.projector(W, post.to(dtype), "fp32"), plen, W["llm.model.embed_tokens.weight"][ids], ids, am, None,
                              geo.speech_id)
    return generate_sampled(W, emb.detach(), mask, dataclasses.asdict(geo), seed, mode="fp32", eos_token_id=geo.eos_id,
                            pad_token_id=geo.eos_id, **kw)
