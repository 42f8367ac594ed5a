"""TEST INFRASTRUCTURE ONLY -- generate(repetition_penalty = p) restated: the decode loop of oracle/tasu_oracle.py::beam_search_generate
with HF's RepetitionPenaltyLogitsProcessor where HF applies it (transformers generation/utils.py + logits_process.py; measured on the
imported reference, pinned by tests/golden/mid_generate_penalty.npz):

  * the history is the GENERATED tokens only -- under ``inputs_embeds`` HF's ``input_ids`` starts empty, the prompt is never penalised;
  * num_beams >= 2 (``_beam_search``): the processor receives the log_softmax output; ``s' = s * p if s < 0 else s / p`` for every token
    of the beam's own prefix, once per distinct token (gather / scatter), no renormalisation; the EOS ban of min_length comes after it;
  * num_beams == 1 (greedy, ``_sample`` without sampling): the processor receives the RAW logits; same rule, then argmax.  Beam search
    is not called: a row that emitted EOS is padded, the loop ends when every row has.

The oracle's own loop has no hook after the softmax and oracle/ is frozen, so the loop is restated here on the oracle's network
functions.  ``mode`` "fp32" / "bf16", ``logit_jitter``, ``logits_trace`` / ``logits_replay`` as in the oracle's loop."""
import numpy as np
import torch

from oracle import tasu_oracle as O

NEG = -1.0e9


def penalise(scores, hist, p):
    """RepetitionPenaltyLogitsProcessor.__call__: scores [R, V] float32, hist [R, t] generated tokens."""
    if hist.shape[1] == 0 or p == 1.0:
        return scores
    s = torch.gather(scores, 1, hist)
    s = torch.where(s < 0, s * p, s / p)
    return scores.scatter(1, hist, s)


def _network(W, geo, emb_b, mask_b, toks, mode):
    table = W["llm.model.embed_tokens.weight"]
    x = torch.cat([emb_b, table[toks]], 1)
    m = torch.cat([mask_b.bool(), torch.ones(toks.shape[0], toks.shape[1], dtype=torch.bool)], 1)
    pos = (m.long().cumsum(-1) - 1).masked_fill(~m, 1)
    hid = O.qwen2_hidden(W, x, m, pos, geo["llm_heads"], geo["llm_kv_heads"], geo.get("rope_theta", 1e6), mode)
    return O.linear(hid[:, -1], O.lm_head_weight(W), None, mode).float()


def generate_penalised(W, emb, mask, geo, num_beams=4, max_new_tokens=200, min_length=1, length_penalty=1.0, repetition_penalty=1.0,
                       eos_token_id=None, pad_token_id=None, mode="fp32", logit_jitter=None, logits_trace=None, logits_replay=None):
    """New tokens [B, n_new] (LongTensor)."""
    B, S, _ = emb.shape
    nb, p = num_beams, float(repetition_penalty)
    min_length = max(int(min_length) - S, 0)                      # HF: min_length counts the embedded prompt
    eos = geo["eos_id"] if eos_token_id is None else eos_token_id
    pad = eos if pad_token_id is None else pad_token_id
    emb_b, mask_b = emb.repeat_interleave(nb, 0), mask.repeat_interleave(nb, 0)

    def logits_of(toks, cur):
        if logits_replay is not None:
            if cur >= len(logits_replay) or not torch.equal(logits_replay[cur][1], toks):
                return None
            lg = logits_replay[cur][0].clone()
        else:
            lg = _network(W, geo, emb_b, mask_b, toks, mode)
        if logits_trace is not None:
            logits_trace.append((lg.clone(), toks.clone()))
        return logit_jitter(lg) if logit_jitter is not None else lg

    if nb == 1:                                                   # ---- greedy
        seq = torch.full((B, max_new_tokens), pad, dtype=torch.long)
        alive = torch.ones(B, dtype=torch.bool)
        cur = 0
        while cur < max_new_tokens and bool(alive.any()):
            lg = logits_of(seq[:, :cur], cur)
            if lg is None:
                return None
            sc = penalise(lg, seq[:, :cur], p)
            if cur < min_length:
                sc[:, eos] = float("-inf")
            tok = sc.argmax(-1)
            tok = torch.where(alive, tok, torch.full_like(tok, pad))
            seq[:, cur] = tok
            alive = alive & (tok != eos)
            cur += 1
        return seq[:, :cur]

    K, V = 2 * nb, O.lm_head_weight(W).shape[0]                   # ---- beam search (the oracle's loop + the processor)
    run_seq = torch.full((B, nb, max_new_tokens), pad, dtype=torch.long)
    fin_seq = run_seq.clone()
    run_scores = torch.zeros(B, nb)
    run_scores[:, 1:] = NEG
    fin_scores = torch.full((B, nb), NEG)
    fin_len = torch.zeros(B, nb, dtype=torch.long)
    is_fin = torch.zeros(B, nb, dtype=torch.bool)
    unsat = torch.ones(B, 1, dtype=torch.bool)
    top_mask = torch.cat([torch.ones(nb, dtype=torch.bool), torch.zeros(K - nb, dtype=torch.bool)])
    cur = 0
    while True:
        toks = run_seq.view(B * nb, -1)[:, :cur]
        lg = logits_of(toks, cur)
        if lg is None:
            return None
        logp = penalise(torch.log_softmax(lg, -1), toks, p)
        if cur < min_length:
            logp[:, eos] = float("-inf")
        acc = (logp.view(B, nb, V) + run_scores[:, :, None]).view(B, nb * V)
        top_lp, top_ix = torch.topk(acc, K)
        beam_ix, tok = top_ix // V, top_ix % V
        cand = torch.gather(run_seq, 1, beam_ix[:, :, None].expand(-1, -1, max_new_tokens)).clone()
        cand[:, :, cur] = tok
        stop = (tok == eos) | (cur + 1 >= max_new_tokens)
        run_lp = top_lp + stop.float() * NEG
        nxt = torch.topk(run_lp, nb)[1]
        run_seq = torch.gather(cand, 1, nxt[:, :, None].expand(-1, -1, max_new_tokens))
        run_scores = torch.gather(run_lp, 1, nxt)
        just = stop & top_mask[None]
        sc = top_lp / ((cur + 1) ** length_penalty)
        sc = sc + (~unsat).float() * NEG + (~just).float() * NEG
        m_seq = torch.cat([fin_seq, cand], 1)
        m_sc = torch.cat([fin_scores, sc], 1)
        m_len = torch.cat([fin_len, torch.full((B, K), cur + 1, dtype=torch.long)], 1)
        m_fin = torch.cat([is_fin, just], 1)
        keep = torch.topk(m_sc, nb)[1]
        fin_seq = torch.gather(m_seq, 1, keep[:, :, None].expand(-1, -1, max_new_tokens))
        fin_scores = torch.gather(m_sc, 1, keep)
        fin_len = torch.gather(m_len, 1, keep)
        is_fin = torch.gather(m_fin, 1, keep)
        cur += 1
        best_run = run_scores[:, :1] / (cur ** length_penalty)
        worst_fin = torch.where(is_fin, fin_scores.min(1, keepdim=True)[0], torch.full_like(fin_scores, NEG))
        unsat = unsat & (best_run > worst_fin).any(-1, keepdim=True)
        if not (bool(unsat.any()) and not bool(stop.all())):
            break
    n = int(fin_len[:, 0].max())
    return fin_seq[:, 0, :n]


def prompt_embeddings(sd, geo, ids, am, post_ids, mode):
    """(emb [B, S, D], mask) of a text-branch prompt: the oracle's projector + merge."""
    post, plen = O.pseudo_posterior(post_ids, geo.ctc_vocab)
    emb, mask, _, _ = O.merge(O.projector(sd, post, mode), plen, sd["llm.model.embed_tokens.weight"][ids], ids, am, None, geo.speech_id)
    return emb.detach(), mask


def penalty_cases():
    """(geo, state dict, cases) of tests/golden/mid_generate_penalty.npz (tools/make_golden_generate_penalty.py): each case
    dict(ids, am, post_ids, kw, tokens, bf16_stable, differs) -- kw includes repetition_penalty; tokens = the REAL reference's."""
    from conftest import load_npz, split_flat
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, decode_fixture_state_dict

    z = load_npz("mid_generate_penalty")
    geo = Geometry.from_dict(MID_GEOMETRY)
    sd = decode_fixture_state_dict(geo, int(z["seed_w"]))
    cases = []
    for n in range(int(z["n_cases"])):
        nb, new, min_len = (int(v) for v in z[f"c{n}_kw"])
        cases.append(dict(ids=torch.from_numpy(z[f"c{n}_input_ids"]), am=torch.from_numpy(z[f"c{n}_attention_mask"]),
                          post_ids=split_flat(z[f"c{n}_post_ids_flat"], z[f"c{n}_post_lens"]), tokens=z[f"c{n}_tokens"],
                          bf16_stable=bool(z["bf16_stable"][n]), differs=bool(z["differs_from_p1"][n]),
                          kw=dict(num_beams=nb, max_new_tokens=new, min_length=min_len, length_penalty=float(z[f"c{n}_length_penalty"]),
                                  repetition_penalty=float(z[f"c{n}_repetition_penalty"]))))
    return geo, sd, cases


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def tokens_on_weights(W, geo, ids, am, post_ids, kw, dtype):
    """generate_penalised on the weights W with every tensor in ``dtype`` (fp32 mode: nothing rounded to bf16) -- e.g. the
    LoRA-merged W + s B A of tests/fp32_oracle_cases.py::lora_merged_double in float32 and float64."""
    import dataclasses
    W = {k: v.to(dtype) for k, v in W.items()}
    post, plen = O.pseudo_posterior(post_ids, geo.ctc_vocab)
    emb, mask, _, _ = O.merge(O.projector(W, post.to(dtype), "fp32"), plen, W["llm.model.embed_tokens.weight"][ids], ids, am, None,
                              geo.speech_id)
    return generate_penalised(W, emb.detach(), mask, dataclasses.asdict(geo), mode="fp32", eos_token_id=geo.eos_id,
                              pad_token_id=geo.eos_id, **kw)
