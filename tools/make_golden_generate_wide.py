"""TEST INFRASTRUCTURE ONLY -- tests/golden/mid_generate_wide.npz: unfiltered random decode cases at the kernel-compatible "mid"
geometry with the REAL reference's ``generate(num_beams = 5 .. 16)`` tokens (fp32, the imported reference through
oracle/ref_import.py), following tools/make_golden_generate_penalty.py: one seeded draw per case, nothing rejected.

The cases cover num_beams in {5, 6, 7, 8, 10, 12, 16} (the 5-beam plans at repetition_penalty = 1.0: the unpenalised bf16 top-k at
k = 10), repetition_penalty in {1.0, 1.3, 0.8}, length_penalty in {0.6, 1.0, 2.0}, an active EOS ban (min_length = prompt length + 5),
B = 1..3 with left padding, max_new_tokens 8..40.  Per case the file also records
  * ``differs_from_nb4``: the reference decodes the case differently at num_beams = 4 (at least half must, or the fixture tests
    nothing the 4-beam fixtures do not);
  * ``bf16_stable``: the restatement tests/penalty_ref.py in bf16 mode reproduces the reference's tokens AND keeps them under
    N_JITTER runs with one-ulp flips on 15 % of every step's logits (oracle.tasu_oracle.bf16_ulp_jitter, the criterion of
    oracle/make_golden_generate_margin.py) -- decided by the restatement, never by the code under test.  The bf16 decode path is
    compared token for token on those cases only.  Two further conditions, neither of which looks at the code under test:
      - the bf16-mode restatement decoded once more with equal scores ordered as the device orders them (by beam, then token:
        ps_slm_amd.decode.BeamState on the restatement's network) must return the same tokens (``holds_under_the_device_tie_rule``).
        bf16 logits tie EXACTLY now and then; the restatement breaks such a tie as torch.topk happens to, and with 10-32 candidates
        per utterance and step a case whose tokens depend on one tie is common.  Stored in ``exact_tie_cases``.
      - as in oracle/make_golden_generate_margin.py, the product's host loop on the CPU double (tests/penalty_ops.py) is then run: a
        third bf16 evaluation of the same network, NOT a filter.  When it decodes other tokens the disagreement must be EXPLAINED
        as rounding (``explain_disagreement``: HF's update on the double's own candidates gives the double's tokens, on the
        restatement's penalised log-probs the reference's, and every candidate log-prob the double saw lies within two bf16 logit
        ulps of the restatement's) -- a near-tie the eight jitter runs missed, stored in ``near_tie_on_double`` -- or the generator
        exits non-zero: a bug in the product's host code.
    Such cases are stored as NOT stable; they stay in the file and in the fp32 comparison.
At least 10 cases must be stable, one of them with 8 beams, one with 16 and one penalised: further seeds are DRAWN (appended, none
rejected) until that holds, up to MAX_CASES.  The fp32-mode restatement must reproduce every case (asserted here).
Only prompts, posterior ids, kwargs and tokens are stored; the weights are regenerated from the seed.  Needs the reference's
source tree, which oracle/ref_import.py imports (it is not part of this repository), and transformers:
    python tools/make_golden_generate_wide.py"""
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import tasu_oracle as O  # noqa: E402
from oracle.make_golden import quiet  # noqa: E402
from oracle.make_golden_generate_margin import JITTER_PROB, MAX_LOGP_DIFF, N_JITTER, SEED_W, make_case  # noqa: E402
from oracle.ref_import import build_reference_model  # noqa: E402
from penalty_ref import generate_penalised, penalise, prompt_embeddings, same  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mid_generate_wide.npz")
N_CASES, MAX_CASES = 24, 60
# ``min_new``: min_length = embedded prompt length + min_new (HF counts the prompt), i.e. EOS banned for min_new positions
PLANS = [dict(num_beams=8, max_new_tokens=12), dict(num_beams=5, max_new_tokens=10),
         dict(num_beams=6, max_new_tokens=9, repetition_penalty=1.3), dict(num_beams=16, max_new_tokens=8),
         dict(num_beams=10, max_new_tokens=14, repetition_penalty=0.8), dict(num_beams=7, max_new_tokens=20, min_new=5),
         dict(num_beams=12, max_new_tokens=10, length_penalty=2.0), dict(num_beams=8, max_new_tokens=16, repetition_penalty=1.3, length_penalty=0.6),
         dict(num_beams=5, max_new_tokens=40, min_new=5), dict(num_beams=16, max_new_tokens=12, repetition_penalty=1.3),
         dict(num_beams=6, max_new_tokens=24, length_penalty=0.6), dict(num_beams=10, max_new_tokens=8, length_penalty=2.0, min_new=5)]
SEED0 = 93000


def decode_on_double(double, geo, ids, am, post_ids, kw, hook=None):
    from ps_slm_amd.decode import beam_search_generate
    st = double.prepare_text(ids, am, None, post_ids, None, None)
    double.forward_projector_text(st)
    orig = double.ops.beam_update
    if hook is not None:
        double.ops.beam_update = lambda vals, idx, bs, first: (hook(vals, idx, first), orig(vals, idx, bs, first))[1]
    try:
        return beam_search_generate(double, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **kw)
    finally:
        if hook is not None:
            del double.ops.beam_update


def holds_under_the_device_tie_rule(W, emb16, mask16, gd, kw, geo, t_ref):
    """The bf16-mode restatement decoded once more with equal scores ordered as the device orders them (by beam, then token: HF's
    update as ps_slm_amd.decode.BeamState makes it, on the network of tests/penalty_ref.py).  The restatement itself breaks a tie
    as torch.topk happens to; bf16 logits (8 significant bits) tie EXACTLY now and then, and with 10-32 candidates per utterance
    and step a case whose tokens depend on one tie is common -- a coin flip the one-ulp jitter only catches when a flip lands on
    it.  True when the tokens are the reference's."""
    from penalty_ref import _network
    from ps_slm_amd.decode import BeamState
    nb, new, p = kw["num_beams"], kw["max_new_tokens"], kw["repetition_penalty"]
    B, S, _ = emb16.shape
    K, min_new = 2 * nb, max(kw["min_length"] - S, 0)
    emb_b, mask_b = emb16.repeat_interleave(nb, 0), mask16.repeat_interleave(nb, 0)
    state = BeamState(B, nb, new, geo.eos_id, geo.eos_id, kw["length_penalty"], min_new)
    while not state.done:
        toks = torch.from_numpy(state.run_seq).view(B * nb, -1)[:, :state.cur]
        logp = penalise(torch.log_softmax(_network(W, gd, emb_b, mask_b, toks, "bf16"), -1), toks, p)
        if state.ban_eos():
            logp[:, geo.eos_id] = float("-inf")
        v, i = torch.sort(logp, dim=-1, descending=True, stable=True)
        state.update(v[:, :K].reshape(B, nb, K).numpy(), i[:, :K].reshape(B, nb, K).numpy().astype(np.int64))
    return same(state.result(), t_ref)


def explain_disagreement(double, geo, ids, am, post_ids, kw, S, trace, tc, t_ref):
    """oracle/make_golden_generate_margin.py::explain_disagreement with the repetition penalty where HF applies it (on the
    log-probs of the row's generated tokens, before the EOS ban); that HF's update on the restatement's log-probs gives the
    reference's tokens is holds_under_the_device_tie_rule's finding (a decode, where the original replays the recorded logits and
    loses them once two tied beams swap slots).  A description when the disagreement is ROUNDING, else None."""
    from ps_slm_amd.decode import BeamState
    nb, new, p = kw["num_beams"], kw["max_new_tokens"], kw["repetition_penalty"]
    K, B, min_new = 2 * nb, ids.shape[0], max(kw["min_length"] - S, 0)
    rec = []
    t2 = decode_on_double(double, geo, ids, am, post_ids, kw, hook=lambda vals, idx, first: rec.append((vals.clone().numpy(), idx.clone().numpy(), first)))
    if not same(t2, tc):
        return None                                                    # the double is not even repeatable
    mk = lambda: BeamState(B, nb, new, geo.eos_id, geo.eos_id, kw["length_penalty"], min_new)  # noqa: E731
    hd = mk()
    worst, same_prefix = 0.0, True
    for i, (dv, di, first) in enumerate(rec):
        if first:
            vv = np.full((B, nb, K), -1.0e9, np.float32)
            ii = np.zeros((B, nb, K), np.int64)
            vv[:, 0], ii[:, 0] = dv[:B], di[:B]
        else:
            vv, ii = dv.reshape(B, nb, K).astype(np.float32), di.reshape(B, nb, K).astype(np.int64)
        if i < len(trace) and same_prefix:
            logits, toks = trace[i]
            logp = penalise(torch.log_softmax(logits, -1), toks, p)
            if i < min_new:
                logp[:, geo.eos_id] = float("-inf")
            same_prefix = same_prefix and np.array_equal(hd.run_seq[:, :, :i], toks.view(B, nb, -1).numpy())
            if same_prefix:
                lp_rows = logp.view(B, nb, -1).numpy()
                for b in range(B):
                    for j in range(1 if first else nb):
                        ref_vals = lp_rows[b, j][ii[b, j]]
                        ok = np.isfinite(ref_vals) & (vv[b, j] > -1.0e8)
                        if ok.any():
                            worst = max(worst, float(np.abs(ref_vals[ok] - vv[b, j][ok]).max()))
        if not hd.done:
            hd.update(vv, ii)
    if not same(hd.result(), tc) or worst > MAX_LOGP_DIFF:
        return None
    return (f"bookkeeping identical (HF update on the double's candidates -> the double's tokens, on the restatement's network -> the "
            f"reference's tokens: holds_under_the_device_tie_rule), candidate log-probs within {worst:.3f} of the restatement's")


def main():
    from penalty_ops import PenaltyFakeOps
    from ps_slm_amd.model import Geometry, TasuModel
    from ps_slm_amd.synthetic import MID_GEOMETRY, decode_fixture_state_dict

    torch.set_num_threads(4)
    geo = Geometry.from_dict(MID_GEOMETRY)
    gd = dataclasses.asdict(geo)
    sd = decode_fixture_state_dict(geo, SEED_W)
    model = build_reference_model(gd, 0, dict(gt_emb=True, gt_emb_noise=False))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("encoder.") or k == "llm.lm_head.weight" for k in missing), (missing, unexpected)
    model.eval()
    double = TasuModel(geo, PenaltyFakeOps(), "cpu")
    double.load_reference_state_dict(sd)
    arrs, stable, differs, meta, near_ties, tie_cases = {}, [], [], [], [], []
    n = 0
    while True:
        plan = PLANS[n % len(PLANS)]
        nb, new, p = plan["num_beams"], plan["max_new_tokens"], plan.get("repetition_penalty", 1.0)
        seed = SEED0 + n                                               # ONE draw per case: nothing is rejected
        rng = np.random.default_rng(seed)
        ids, am, targets = make_case(geo, rng, 3)
        post_ids = [model.encoder_tokenizer.encode(t) for t in targets]
        emb, mask = prompt_embeddings(sd, geo, ids, am, post_ids, "fp32")
        S = emb.shape[1]
        min_length = S + plan["min_new"] if "min_new" in plan else 1
        kw = dict(max_new_tokens=new, min_length=min_length, length_penalty=plan.get("length_penalty", 1.0), repetition_penalty=p)
        ref = lambda beams: quiet(model.generate, input_ids=ids, input_features=torch.zeros(len(post_ids), 8, geo.feat_dim),  # noqa: E731
                                  attention_mask=am, input_feature_length=torch.full((len(post_ids),), 8), targets=targets,
                                  num_beams=beams, **kw)
        with torch.no_grad():
            toks = ref(nb)
            toks_nb4 = ref(4)
        kw["num_beams"] = nb
        t32 = generate_penalised(sd, emb, mask, gd, mode="fp32", **kw)
        assert same(t32, toks), (n, t32, toks)                       # the restatement IS the reference's loop
        emb16, mask16 = prompt_embeddings(sd, geo, ids, am, post_ids, "bf16")
        trace = []
        t16 = generate_penalised(sd, emb16, mask16, gd, mode="bf16", logits_trace=trace, **kw)
        ok = same(t16, toks)
        for j in range(N_JITTER if ok else 0):
            jit = lambda: O.bf16_ulp_jitter(100 * seed + j, JITTER_PROB)  # noqa: E731
            tj = generate_penalised(sd, emb16, mask16, gd, mode="bf16", logits_replay=trace, logit_jitter=jit(), **kw)
            if tj is None:                                               # a beam left the recorded trajectory: decode for real
                tj = generate_penalised(sd, emb16, mask16, gd, mode="bf16", logit_jitter=jit(), **kw)
            if not same(tj, toks):
                ok = False
                break
        if ok and not holds_under_the_device_tie_rule(sd, emb16, mask16, gd, kw, geo, t16):
            print(f"case {n}: hinges on an exact tie of bf16 scores (torch.topk's order against the device's): stored as not stable", flush=True)
            tie_cases.append(n)
            ok = False
        if ok:
            tc = decode_on_double(double, geo, ids, am, post_ids, kw)
            if not same(tc, toks):
                why = explain_disagreement(double, geo, ids, am, post_ids, kw, S, trace, tc, t16)
                if why is None:
                    raise SystemExit(f"the CPU double disagrees on case {n} (seed {seed}) and rounding does not explain it: double "
                                     f"{tc.tolist()} reference {toks.tolist()} -- fix the product's host code, do not drop the case")
                print(f"case {n}: a near-tie the jitter runs missed, stored as not stable: {why}; double {tc.tolist()}", flush=True)
                near_ties.append(n)
                ok = False
        stable.append(ok)
        differs.append(not same(toks, toks_nb4))
        meta.append((nb, p))
        arrs.update({f"c{n}_input_ids": ids.numpy(), f"c{n}_attention_mask": am.numpy(), f"c{n}_tokens": toks.numpy(),
                     f"c{n}_post_ids_flat": np.concatenate([np.asarray(q) for q in post_ids]),
                     f"c{n}_post_lens": np.asarray([len(q) for q in post_ids]), f"c{n}_kw": np.asarray([nb, new, min_length]),
                     f"c{n}_length_penalty": np.asarray(kw["length_penalty"]), f"c{n}_repetition_penalty": np.asarray(p),
                     f"c{n}_seed": np.asarray(seed)})
        print(f"case {n}: seed {seed} B={ids.shape[0]} S={S} nb={nb} new={new} p={p} lp={kw['length_penalty']} min_length={min_length} "
              f"stable={ok} differs_from_nb4={differs[-1]} tokens {toks.tolist()}", flush=True)
        n += 1
        enough = (sum(stable) >= 10 and all(any(s and b == w for s, (b, _) in zip(stable, meta)) for w in (8, 16))
                  and any(s and q != 1.0 for s, (_, q) in zip(stable, meta)))
        if n >= N_CASES and enough:
            break
        assert n < MAX_CASES, "no stable set within MAX_CASES draws"
    assert 2 * sum(differs) >= n, (sum(differs), n)                    # the wider beam must change what is decoded
    arrs["n_cases"] = np.asarray(n)
    arrs["bf16_stable"] = np.asarray(stable)
    arrs["differs_from_nb4"] = np.asarray(differs)
    arrs["near_tie_on_double"] = np.asarray(near_ties, dtype=np.int64)
    arrs["exact_tie_cases"] = np.asarray(tie_cases, dtype=np.int64)
    arrs["seed_w"] = np.asarray(SEED_W)
    np.savez_compressed(OUT, **arrs)
    print(n, "cases,", sum(stable), "bf16-stable,", len(tie_cases), "hinge on exact bf16 ties,", len(near_ties), "near-ties found on the double's evidence,", sum(differs), "decode differently at 4 beams;", f"{os.path.getsize(OUT) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
