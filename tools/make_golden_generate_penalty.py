"""TEST INFRASTRUCTURE ONLY -- tests/golden/mid_generate_penalty.npz: unfiltered random decode cases at the kernel-compatible "mid"
geometry with the REAL reference's ``generate(repetition_penalty = p)`` tokens (fp32, the imported reference through
oracle/ref_import.py), following oracle/make_golden_generate_fp32.py: one seeded draw per case, nothing rejected.

The cases cover num_beams 1..5 (1 = HF's greedy search: penalty on the raw logits; >= 2: on the log-probs), p in {1.1, 1.3, 2.0, 0.8}
(p < 1 boosts repeats), an active EOS ban (min_length = prompt length + 5 / + 8), length penalties, B = 1..3 with left padding,
max_new_tokens 8..30.  Per case the file also records
  * ``differs_from_p1``: the reference decodes the case differently at p = 1.0 (at least half must, or the fixture tests nothing);
  * ``bf16_stable``: the restatement tests/penalty_ref.py in bf16 mode reproduces the reference's tokens AND keeps them under
    N_JITTER runs with one-ulp flips on 15 % of every step's logits (oracle.tasu_oracle.bf16_ulp_jitter, the criterion of
    oracle/make_golden_generate_margin.py) -- decided by the restatement, never by the code under test.  The bf16 decode path is
    compared token for token on those cases only.
At least 10 cases must be stable, one of them with num_beams = 1 and one with p < 1: further seeds are DRAWN (appended, none
rejected) until that holds.  The fp32-mode restatement must reproduce every case (asserted here).
Only prompts, posterior ids, kwargs and tokens are stored; the weights are regenerated from the seed.  Run in the build container only:
    python tools/make_golden_generate_penalty.py"""
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
from oracle.make_golden_generate_margin import JITTER_PROB, N_JITTER, SEED_W, make_case  # noqa: E402
from oracle.ref_import import build_reference_model  # noqa: E402
from penalty_ref import generate_penalised, prompt_embeddings, same  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mid_generate_penalty.npz")
N_CASES, MAX_CASES = 24, 60
# ``min_new``: min_length = embedded prompt length + min_new (HF counts the prompt), i.e. EOS banned for min_new positions
PLANS = [dict(num_beams=4, max_new_tokens=12, repetition_penalty=1.3), dict(num_beams=1, max_new_tokens=10, repetition_penalty=1.3),
         dict(num_beams=2, max_new_tokens=9, repetition_penalty=2.0), dict(num_beams=3, max_new_tokens=14, repetition_penalty=0.8),
         dict(num_beams=5, max_new_tokens=8, repetition_penalty=1.1), dict(num_beams=4, max_new_tokens=20, repetition_penalty=1.1, min_new=5),
         dict(num_beams=1, max_new_tokens=16, repetition_penalty=0.8), dict(num_beams=3, max_new_tokens=10, repetition_penalty=1.3, length_penalty=2.0),
         dict(num_beams=5, max_new_tokens=12, repetition_penalty=2.0), dict(num_beams=2, max_new_tokens=30, repetition_penalty=1.3, min_new=8),
         dict(num_beams=4, max_new_tokens=8, repetition_penalty=0.8, length_penalty=0.5), dict(num_beams=1, max_new_tokens=24, repetition_penalty=2.0)]
SEED0 = 91000


def main():
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, decode_fixture_state_dict

    torch.set_num_threads(4)
    geo = Geometry.from_dict(MID_GEOMETRY)
    gd = dataclasses.asdict(geo)
    sd = decode_fixture_state_dict(geo, SEED_W)
    model = build_reference_model(gd, 0, dict(gt_emb=True, gt_emb_noise=False))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("encoder.") or k == "llm.lm_head.weight" for k in missing), (missing, unexpected)
    model.eval()
    arrs, stable, differs, meta = {}, [], [], []
    n = 0
    while True:
        plan = PLANS[n % len(PLANS)]
        nb, new, p = plan["num_beams"], plan["max_new_tokens"], plan["repetition_penalty"]
        seed = SEED0 + n                                               # ONE draw per case: nothing is rejected
        rng = np.random.default_rng(seed)
        ids, am, targets = make_case(geo, rng, 3)
        post_ids = [model.encoder_tokenizer.encode(t) for t in targets]
        emb, mask = prompt_embeddings(sd, geo, ids, am, post_ids, "fp32")
        S = emb.shape[1]
        min_length = S + plan["min_new"] if "min_new" in plan else 1
        kw = dict(num_beams=nb, max_new_tokens=new, min_length=min_length, length_penalty=plan.get("length_penalty", 1.0))
        ref = lambda **extra: quiet(model.generate, input_ids=ids, input_features=torch.zeros(len(post_ids), 8, geo.feat_dim),  # noqa: E731
                                    attention_mask=am, input_feature_length=torch.full((len(post_ids),), 8), targets=targets, **kw, **extra)
        with torch.no_grad():
            toks = ref(repetition_penalty=p)
            toks_p1 = ref()
        t32 = generate_penalised(sd, emb, mask, gd, repetition_penalty=p, mode="fp32", **kw)
        assert same(t32, toks), (n, t32, toks)                       # the restatement IS the reference's loop
        emb16, mask16 = prompt_embeddings(sd, geo, ids, am, post_ids, "bf16")
        trace = []
        t16 = generate_penalised(sd, emb16, mask16, gd, repetition_penalty=p, mode="bf16", logits_trace=trace, **kw)
        ok = same(t16, toks)
        for j in range(N_JITTER if ok else 0):
            jit = lambda: O.bf16_ulp_jitter(100 * seed + j, JITTER_PROB)  # noqa: E731
            tj = generate_penalised(sd, emb16, mask16, gd, repetition_penalty=p, mode="bf16", logits_replay=trace, logit_jitter=jit(), **kw)
            if tj is None:                                               # a beam left the recorded trajectory: decode for real
                tj = generate_penalised(sd, emb16, mask16, gd, repetition_penalty=p, mode="bf16", logit_jitter=jit(), **kw)
            if not same(tj, toks):
                ok = False
                break
        stable.append(ok)
        differs.append(not same(toks, toks_p1))
        meta.append((nb, p))
        arrs.update({f"c{n}_input_ids": ids.numpy(), f"c{n}_attention_mask": am.numpy(), f"c{n}_tokens": toks.numpy(),
                     f"c{n}_post_ids_flat": np.concatenate([np.asarray(q) for q in post_ids]),
                     f"c{n}_post_lens": np.asarray([len(q) for q in post_ids]), f"c{n}_kw": np.asarray([nb, new, min_length]),
                     f"c{n}_length_penalty": np.asarray(kw["length_penalty"]), f"c{n}_repetition_penalty": np.asarray(p),
                     f"c{n}_seed": np.asarray(seed)})
        print(f"case {n}: seed {seed} B={ids.shape[0]} S={S} nb={nb} new={new} p={p} min_length={min_length} stable={ok} "
              f"differs_from_p1={differs[-1]} tokens {toks.tolist()}", flush=True)
        n += 1
        enough = (sum(stable) >= 10 and any(s and b == 1 for s, (b, _) in zip(stable, meta))
                  and any(s and q < 1 for s, (_, q) in zip(stable, meta)))
        if n >= N_CASES and enough:
            break
        assert n < MAX_CASES, "no stable set within MAX_CASES draws"
    assert 2 * sum(differs) >= n, (sum(differs), n)                    # the penalty must change what is decoded
    arrs["n_cases"] = np.asarray(n)
    arrs["bf16_stable"] = np.asarray(stable)
    arrs["differs_from_p1"] = np.asarray(differs)
    arrs["seed_w"] = np.asarray(SEED_W)
    np.savez_compressed(OUT, **arrs)
    print(n, "cases,", sum(stable), "bf16-stable,", sum(differs), "decode differently at p = 1.0;", f"{os.path.getsize(OUT) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
