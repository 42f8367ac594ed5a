"""TEST INFRASTRUCTURE ONLY -- tests/golden/mid_generate_beam_sample.npz: unfiltered random decode cases at the kernel-compatible "mid"
geometry (V = 1000) with the REAL reference's ``generate(do_sample=True, num_beams=nb, ...)`` tokens (fp32, the imported reference
through oracle/ref_import.py), following tools/make_golden_generate_sample.py: one seeded draw per case, nothing rejected.

Everything HF does up to the draw is its own code: log_softmax, the processors and warpers (min_tokens_to_keep = 2), the accumulated
scores.  For the duration of the call ``torch.multinomial`` is replaced by the project's draw -- the 2 nb largest Gumbel keys of an
utterance's accumulated scores in key order, tests/beam_sample_ref64.py::draw_flat.  The draw needs the accumulated scores, not their
softmax, so ``torch.nn.functional.softmax`` records its last argument for the call (HF's ``_get_top_k_continuations`` forms the
multinomial argument with it); the stand-in asserts that the softmax of what was recorded IS what multinomial receives.  ``top_k``
reaches HF through the model's generation config, as in production.

The plans cover num_beams in {2, 4, 5, 6, 16}, top_k in {1, 2, 8, 50}, top_p in {1.0, 0.9, 0.5}, T in {0.7, 1.0, 1.5}, repetition
penalties {1.0, 1.3}, an active EOS ban (min_length = prompt length + min_new), length_penalty != 1, B = 1..3 with left padding,
max_new_tokens 4..12.  ``fp32_stable`` / ``bf16_stable`` are decided by the restatement tests/beam_sample_ref.py under jitter exactly
as tools/make_golden_generate_sample.py decides them.  The fp32-mode restatement must reproduce every case (asserted here).  At least
24 cases, 20 fp32-stable, 6 bf16-stable, among the bf16-stable ones one with num_beams >= 6 and one with a penalty: further seeds are
DRAWN (appended, none rejected) until that holds.  Only prompts, posterior ids, kwargs, seeds and tokens are stored.  Run in the build
container only:
    python tools/make_golden_generate_beam_sample.py"""
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
from beam_sample_ref import draw_seed, generate_beam_sampled, prompt_embeddings, relative_jitter, same  # noqa: E402
from beam_sample_ref64 import draw_flat  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mid_generate_beam_sample.npz")
N_CASES, MAX_CASES = 24, 96
N_JITTER_BF16 = 4 * N_JITTER
# ``min_new``: min_length = embedded prompt length + min_new, i.e. EOS banned for min_new positions.  bf16 rounding of the logits
# moves most long decodes over a wide support, so the plans that can be bf16-stable are narrow and short.
PLANS = [dict(num_beams=2, top_k=2, max_new_tokens=5), dict(num_beams=4, top_k=50, max_new_tokens=12, top_p=0.9, temperature=0.7),
         dict(num_beams=6, top_k=1, max_new_tokens=4, temperature=0.7), dict(num_beams=5, top_k=8, max_new_tokens=8, top_p=0.5, repetition_penalty=1.3),
         dict(num_beams=16, top_k=2, max_new_tokens=4, top_p=0.9), dict(num_beams=4, top_k=50, max_new_tokens=10, repetition_penalty=1.3, min_new=5),
         dict(num_beams=2, top_k=2, max_new_tokens=5, repetition_penalty=1.3, temperature=0.7), dict(num_beams=6, top_k=8, max_new_tokens=9, temperature=1.5, top_p=0.9, length_penalty=2.0),
         dict(num_beams=2, top_k=1, max_new_tokens=4, top_p=0.5, temperature=0.7, repetition_penalty=1.3), dict(num_beams=16, top_k=50, max_new_tokens=6, top_p=0.5),
         dict(num_beams=5, top_k=8, max_new_tokens=11, temperature=0.7, min_new=4, length_penalty=0.5), dict(num_beams=4, top_k=2, max_new_tokens=6, top_p=0.9, repetition_penalty=1.3)]
SEED0 = 97000


class Draw:
    """The stand-ins of one generate() call: ``softmax`` records what F.softmax last received, ``multinomial`` draws from it; position
    t = the number of multinomial calls so far."""

    def __init__(self, seed, softmax):
        self.seed, self.t, self.keep_softmax, self.last = seed, 0, softmax, None

    def softmax(self, input, *a, **k):
        self.last = input
        return self.keep_softmax(input, *a, **k)

    def multinomial(self, probs, num_samples, *a, **k):
        assert not a and not k and self.last is not None and self.last.shape == probs.shape
        acc = self.last.detach().float().cpu()
        assert torch.equal(self.keep_softmax(acc, dim=-1), probs.detach().float().cpu())        # the scores behind THESE probabilities
        ix = torch.from_numpy(draw_flat(acc.numpy(), self.seed, self.t, num_samples))
        self.t += 1
        return ix.to(probs.device)


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
    arrs, f32_stable, b16_stable, meta = {}, [], [], []
    n = 0
    while True:
        plan = PLANS[n % len(PLANS)]
        nb, top_k, new = plan["num_beams"], plan["top_k"], plan["max_new_tokens"]
        T, top_p, pen = plan.get("temperature", 1.0), plan.get("top_p", 1.0), plan.get("repetition_penalty", 1.0)
        lpen = plan.get("length_penalty", 1.0)
        manual_seed = SEED0 + n                                        # ONE draw per case: nothing is rejected
        rng = np.random.default_rng(manual_seed)
        ids, am, targets = make_case(geo, rng, 3)
        post_ids = [model.encoder_tokenizer.encode(t) for t in targets]
        emb, mask = prompt_embeddings(sd, geo, ids, am, post_ids, "fp32")
        S = emb.shape[1]
        min_length = S + plan["min_new"] if "min_new" in plan else 1
        seed = draw_seed(manual_seed)
        skw = dict(num_beams=nb, max_new_tokens=new, min_length=min_length, length_penalty=lpen, repetition_penalty=pen, temperature=T,
                   top_k=top_k, top_p=top_p)
        model.llm.generation_config.top_k = top_k                      # (the reference passes no top_k: HF reads the model's)
        keep = torch.multinomial, torch.nn.functional.softmax
        d = Draw(seed, keep[1])
        torch.multinomial, torch.nn.functional.softmax = d.multinomial, d.softmax
        try:
            with torch.no_grad():
                toks = quiet(model.generate, input_ids=ids, input_features=torch.zeros(len(post_ids), 8, geo.feat_dim), attention_mask=am,
                             input_feature_length=torch.full((len(post_ids),), 8), targets=targets, do_sample=True, num_beams=nb,
                             max_new_tokens=new, min_length=min_length, length_penalty=lpen, repetition_penalty=pen, temperature=T,
                             top_p=top_p)
        finally:
            torch.multinomial, torch.nn.functional.softmax = keep
        assert d.t >= toks.shape[1] >= 1, (d.t, toks.shape)             # one draw per position of the search
        t32 = generate_beam_sampled(sd, emb, mask, gd, seed, mode="fp32", **skw)
        assert same(t32, toks), (n, t32, toks)                        # the restatement IS the reference's loop
        trace = []
        generate_beam_sampled(sd, emb, mask, gd, seed, mode="fp32", logits_trace=trace, **skw)
        ok32 = True
        for j in range(N_JITTER):
            jit = lambda: relative_jitter(100 * manual_seed + j)  # noqa: E731
            tj = generate_beam_sampled(sd, emb, mask, gd, seed, mode="fp32", logits_replay=trace, logit_jitter=jit(), **skw)
            if tj is None:                                               # a beam left the recorded trajectory
                tj = generate_beam_sampled(sd, emb, mask, gd, seed, mode="fp32", logit_jitter=jit(), **skw)
            if not same(tj, toks):
                ok32 = False
                break
        emb16, mask16 = prompt_embeddings(sd, geo, ids, am, post_ids, "bf16")
        trace = []
        t16 = generate_beam_sampled(sd, emb16, mask16, gd, seed, mode="bf16", logits_trace=trace, **skw)
        ok16 = same(t16, toks)
        for j in range(N_JITTER_BF16 if ok16 else 0):
            jit = lambda: O.bf16_ulp_jitter(100 * manual_seed + j, JITTER_PROB)  # noqa: E731
            tj = generate_beam_sampled(sd, emb16, mask16, gd, seed, mode="bf16", logits_replay=trace, logit_jitter=jit(), **skw)
            if tj is None:
                tj = generate_beam_sampled(sd, emb16, mask16, gd, seed, mode="bf16", logit_jitter=jit(), **skw)
            if not same(tj, toks):
                ok16 = False
                break
        f32_stable.append(ok32)
        b16_stable.append(ok16)
        meta.append((nb, pen))
        arrs.update({f"c{n}_input_ids": ids.numpy(), f"c{n}_attention_mask": am.numpy(), f"c{n}_tokens": toks.numpy(),
                     f"c{n}_post_ids_flat": np.concatenate([np.asarray(q) for q in post_ids]),
                     f"c{n}_post_lens": np.asarray([len(q) for q in post_ids]), f"c{n}_kw": np.asarray([nb, new, min_length, top_k]),
                     f"c{n}_kwf": np.asarray([T, top_p, pen, lpen], dtype=np.float64), f"c{n}_manual_seed": np.asarray(manual_seed),
                     f"c{n}_seed": np.asarray(seed, dtype=np.int64)})
        print(f"case {n}: seed {manual_seed} B={ids.shape[0]} S={S} nb={nb} new={new} top_k={top_k} top_p={top_p} T={T} p={pen} lp={lpen} "
              f"min_length={min_length} fp32_stable={ok32} bf16_stable={ok16} tokens {toks.tolist()}", flush=True)
        n += 1
        s16 = [m for s, m in zip(b16_stable, meta) if s]
        enough = sum(f32_stable) >= 20 and len(s16) >= 6 and any(b >= 6 for b, _ in s16) and any(p != 1.0 for _, p in s16)
        if n >= N_CASES and enough:
            break
        assert n < MAX_CASES, "no stable set within MAX_CASES draws"
    arrs["n_cases"] = np.asarray(n)
    arrs["fp32_stable"] = np.asarray(f32_stable)
    arrs["bf16_stable"] = np.asarray(b16_stable)
    arrs["seed_w"] = np.asarray(SEED_W)
    np.savez_compressed(OUT, **arrs)
    print(n, "cases,", sum(f32_stable), "fp32-stable,", sum(b16_stable), "bf16-stable;", f"{os.path.getsize(OUT) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
