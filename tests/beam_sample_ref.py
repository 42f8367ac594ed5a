"""TEST INFRASTRUCTURE ONLY -- generate(do_sample=True, num_beams > 1) restated: HF's ``_beam_search`` loop with do_sample
(transformers generation/utils.py; "beam-search multinomial sampling") on the oracle's network functions, like tests/penalty_ref.py's
beam loop, with the processors and warpers in HF's order on the log-softmax output and HF's own torch float32 expressions
(RepetitionPenaltyLogitsProcessor, MinLengthLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper; with more
than one beam HF builds the warpers with min_tokens_to_keep = 2), the accumulated scores, and -- in torch.multinomial's place -- the
project's draw: the 2 nb largest Gumbel keys of an utterance's accumulated scores in key order (tests/beam_sample_ref64.py::draw_flat).
The fixture generator (tools/make_golden_generate_beam_sample.py) puts the same draw into the REAL reference's call.

What depends on the draw order, as in HF: the drawn candidates are NOT sorted by score; the running beams are the best nb non-stopped
by accumulated score (ties: the earlier slot), and only the first nb slots of the draw may enter the finished heap.
``mode`` "fp32" / "bf16", ``logit_jitter``, ``logits_trace`` / ``logits_replay`` as in tests/penalty_ref.py; ``steps`` (a list, or
None) receives the state after every position for tests that compare BeamState.update_drawn with this loop."""
import numpy as np
import torch

from oracle import tasu_oracle as O
from beam_sample_ref64 import draw_flat
from penalty_ref import NEG, _network, penalise, prompt_embeddings, same  # noqa: F401
from sample_ref import draw_seed, relative_jitter  # noqa: F401


def warp2(scores, temperature, top_k, top_p, keep=2):
    """TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper with min_tokens_to_keep = ``keep`` on [R, V] float32 scores."""
    scores = scores / temperature
    k = min(max(top_k, keep), scores.size(-1))
    scores = scores.masked_fill(scores < torch.topk(scores, k)[0][..., -1, None], float("-inf"))
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        remove = sorted_logits.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        remove[..., -keep:] = 0
        scores = scores.masked_fill(remove.scatter(1, sorted_indices, remove), float("-inf"))
    return scores


def generate_beam_sampled(W, emb, mask, geo, seed, num_beams=4, max_new_tokens=200, min_length=1, length_penalty=1.0,
                          repetition_penalty=1.0, temperature=1.0, top_k=50, top_p=1.0, eos_token_id=None, pad_token_id=None, mode="fp32",
                          logit_jitter=None, logits_trace=None, logits_replay=None, steps=None):
    """New tokens [B, n_new] (LongTensor); None when a replayed trace no longer matches the beams' tokens."""
    B, S, _ = emb.shape
    nb, p = num_beams, float(repetition_penalty)
    min_length = max(int(min_length) - S, 0)                      # HF: min_length counts the embedded prompt
    eos = geo["eos_id"] if eos_token_id is None else eos_token_id
    pad = eos if pad_token_id is None else pad_token_id
    emb_b, mask_b = emb.repeat_interleave(nb, 0), mask.repeat_interleave(nb, 0)
    K, V = 2 * nb, O.lm_head_weight(W).shape[0]
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
        if logits_replay is not None:
            if cur >= len(logits_replay) or not torch.equal(logits_replay[cur][1], toks):
                return None
            lg = logits_replay[cur][0].clone()
        else:
            lg = _network(W, geo, emb_b, mask_b, toks, mode)
        if logits_trace is not None:
            logits_trace.append((lg.clone(), toks.clone()))
        if logit_jitter is not None:
            lg = logit_jitter(lg)
        logp = penalise(torch.log_softmax(lg, -1), toks, p)
        if cur < min_length:
            logp[:, eos] = float("-inf")
        logp = warp2(logp, temperature, top_k, top_p)
        acc = (logp.view(B, nb, V) + run_scores[:, :, None]).view(B, nb * V)
        top_ix = torch.from_numpy(draw_flat(acc.numpy(), seed, cur, K))          # (torch.multinomial(softmax(acc), K)'s stand-in)
        top_lp = torch.gather(acc, 1, top_ix)                                    # in draw order, not sorted
        beam_ix, tok = top_ix // V, top_ix % V
        cand = torch.gather(run_seq, 1, beam_ix[:, :, None].expand(-1, -1, max_new_tokens)).clone()
        cand[:, :, cur] = tok
        stop = (tok == eos) | (cur + 1 >= max_new_tokens)
        run_lp = top_lp + stop.float() * NEG
        nxt = torch.sort(run_lp, dim=1, descending=True, stable=True)[1][:, :nb]
        run_seq = torch.gather(cand, 1, nxt[:, :, None].expand(-1, -1, max_new_tokens))
        run_scores = torch.gather(run_lp, 1, nxt)
        just = stop & top_mask[None]
        sc = top_lp / ((cur + 1) ** length_penalty)
        sc = sc + (~unsat).float() * NEG + (~just).float() * NEG
        m_seq = torch.cat([fin_seq, cand], 1)
        m_sc = torch.cat([fin_scores, sc], 1)
        m_len = torch.cat([fin_len, torch.full((B, K), cur + 1, dtype=torch.long)], 1)
        m_fin = torch.cat([is_fin, just], 1)
        keep = torch.sort(m_sc, dim=1, descending=True, stable=True)[1][:, :nb]
        fin_seq = torch.gather(m_seq, 1, keep[:, :, None].expand(-1, -1, max_new_tokens))
        fin_scores = torch.gather(m_sc, 1, keep)
        fin_len = torch.gather(m_len, 1, keep)
        is_fin = torch.gather(m_fin, 1, keep)
        cur += 1
        best_run = run_scores[:, :1] / (cur ** length_penalty)
        worst_fin = torch.where(is_fin, fin_scores.min(1, keepdim=True)[0], torch.full_like(fin_scores, NEG))
        unsat = unsat & (best_run > worst_fin).any(-1, keepdim=True)
        done = not (bool(unsat.any()) and not bool(stop.all()))
        if steps is not None:
            steps.append(dict(acc=acc.clone(), top_ix=top_ix.clone(), run_seq=run_seq.clone(), run_scores=run_scores.clone(),
                              fin_seq=fin_seq.clone(), fin_scores=fin_scores.clone(), fin_len=fin_len.clone(), is_fin=is_fin.clone(),
                              unsat=unsat[:, 0].clone(), done=done, next_tok=torch.gather(tok, 1, nxt), next_parent=torch.gather(beam_ix, 1, nxt)))
        if done:
            break
    n = int(fin_len[:, 0].max())
    return fin_seq[:, 0, :n]


def beam_sample_cases():
    """(geo, state dict, cases) of tests/golden/mid_generate_beam_sample.npz (tools/make_golden_generate_beam_sample.py): each case
    dict(ids, am, post_ids, kw, manual_seed, seed, tokens, fp32_stable, bf16_stable) -- kw = the generate() keywords of the call
    (num_beams among them), ``manual_seed`` what torch.manual_seed receives before it, ``seed`` the 64-bit seed the call then draws,
    tokens = the REAL reference's."""
    from conftest import load_npz, split_flat
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, decode_fixture_state_dict

    z = load_npz("mid_generate_beam_sample")
    geo = Geometry.from_dict(MID_GEOMETRY)
    sd = decode_fixture_state_dict(geo, int(z["seed_w"]))
    cases = []
    for n in range(int(z["n_cases"])):
        nb, new, min_len, top_k = (int(v) for v in z[f"c{n}_kw"])
        T, top_p, pen, lpen = (float(v) for v in z[f"c{n}_kwf"])
        cases.append(dict(ids=torch.from_numpy(z[f"c{n}_input_ids"]), am=torch.from_numpy(z[f"c{n}_attention_mask"]),
                          post_ids=split_flat(z[f"c{n}_post_ids_flat"], z[f"c{n}_post_lens"]), tokens=z[f"c{n}_tokens"],
                          manual_seed=int(z[f"c{n}_manual_seed"]), seed=int(z[f"c{n}_seed"]),
                          fp32_stable=bool(z["fp32_stable"][n]), bf16_stable=bool(z["bf16_stable"][n]),
                          kw=dict(num_beams=nb, max_new_tokens=new, min_length=min_len, top_k=top_k, temperature=T, top_p=top_p,
                                  repetition_penalty=pen, length_penalty=lpen)))
    return geo, sd, cases
