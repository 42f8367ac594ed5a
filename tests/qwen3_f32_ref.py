"""TEST HELPER (not a test, never shipped): the fp32 premise of tests/golden/mid_qwen3_generate.npz and what the fp32 tests of the
Qwen3 decoder share.  The fixture's tokens are the REAL reference's in fp32; the fp32 restatement (tests/qwen3_ref.py) reproduces
them on all cases and keeps them under N_JITTER runs with +-2e-5 relative logit noise (sample_ref.relative_jitter(100 n + j): the
documented agreement of the fp32 path with the reference), so the fp32 decode is asked for all of them token for token.  The
penalty and the sampled case are those of the fixture (pen_case / smp_case, chosen there for the bf16 restatement) with the fp32
restatement's tokens, computed here; both are jitter-stable in fp32 as well (tests/test_qwen3_fp32_cpu.py asserts it)."""
import dataclasses

import torch

import qwen3_ref as R
from penalty_ref import generate_penalised, prompt_embeddings, same
from sample_ref import draw_seed, generate_sampled, relative_jitter

N_JITTER = 8


def stable_tokens(gen, seed0):
    """(tokens of ``gen`` without noise, whether the N_JITTER noisy runs keep them); the noisy runs replay the recorded logits"""
    trace = []
    toks = gen(logits_trace=trace)
    for j in range(N_JITTER):
        tj = gen(logits_replay=trace, logit_jitter=relative_jitter(100 * seed0 + j))
        if tj is None:                                           # a beam left the recorded trajectory: decode for real
            tj = gen(logit_jitter=relative_jitter(100 * seed0 + j))
        if not same(tj, toks):
            return toks, False
    return toks, True


def case_tokens(sd, geo, c, n):
    """the fp32 restatement on fixture case n: (tokens, jitter-stable)"""
    gd = dataclasses.asdict(geo)
    with torch.no_grad():
        emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
        return stable_tokens(lambda **x: R.beam_search_generate(sd, emb, mask, gd, mode="fp32", **c["kw"], **x), n)


def knob_cases_fp32(sd, geo, cases):
    """(penalty case, sampled case, both jitter-stable): the fixture's two knob cases with the fp32 restatement's tokens"""
    pen, smp = R.knob_cases(cases)
    gd = dataclasses.asdict(geo)
    with torch.no_grad(), R.as_qwen3():
        emb, mask = prompt_embeddings(sd, geo, pen["ids"], pen["am"], pen["post_ids"], "fp32")
        tp, ok_p = stable_tokens(lambda **x: generate_penalised(sd, emb, mask, gd, mode="fp32", **pen["kw"], **x), 7000)
        emb, mask = prompt_embeddings(sd, geo, smp["ids"], smp["am"], smp["post_ids"], "fp32")
        T, top_k, top_p = smp["sampling"]
        seed = draw_seed(smp["manual_seed"])
        ts, ok_s = stable_tokens(lambda **x: generate_sampled(sd, emb, mask, gd, seed, max_new_tokens=smp["kw"]["max_new_tokens"],
                                                              min_length=smp["kw"]["min_length"], mode="fp32", temperature=T, top_k=top_k,
                                                              top_p=top_p, **x), 8000)
    return dict(pen, tokens=tp.numpy()), dict(smp, tokens=ts.numpy()), ok_p and ok_s


def decode_case_fp32(model, geo, c, graphs=None):
    """the product's fp32 decode loop on a fixture case (a penalty / sampled one included): numpy tokens"""
    from ps_slm_amd.decode import check_sampling
    from ps_slm_amd.decode_fp32 import beam_search_generate_fp32
    kw = dict(c["kw"])
    if "sampling" in c:
        kw["sampling"] = check_sampling(*c["sampling"])
        torch.manual_seed(c["manual_seed"])
    st = model.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    keep = model.decode_graphs
    if graphs is not None:
        model.decode_graphs = graphs
    try:
        return beam_search_generate_fp32(model, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw).numpy()
    finally:
        model.decode_graphs = keep
