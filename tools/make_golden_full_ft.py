"""TEST INFRASTRUCTURE ONLY -- tests/golden/mid_text_full_ft.npz (tied head) and mid_text_full_ft_untied.npz: the REAL reference
model (imported through oracle/ref_import.py) at the "mid" geometry with what ``train_config.freeze_llm = false`` does to it
restated: every parameter of ``model.llm`` keeps ``requires_grad = True`` and the LLM is in training mode
(Multitask/model/ps-slm.py:105-108).  fp32, one text-branch training step on the seeds and batch of mid_text_lora
(oracle/make_golden_lora.py: seed_w 2026, seed_b 31): loss, accuracy, sampled logit columns and the lse, the projector's gradients
except ffn.0.weight, and for EVERY tensor of Qwen2ForCausalLM its full gradient norm (fp32, ``gnorm.<key>``) and values in fp16
scaled by a power of two (``g.<key>`` / ``gscale.<key>``): all of a 1-D tensor, every 4th row and column of a matrix, and for the
embedding table the rows the batch looks up plus 64 seeded others (``egrad_rows``, the use_emb fixtures' selection).

The generator asserts that no tensor's gradient norm is below 1e-3 of the largest, so that relative bars on every tensor mean
something.  Every tensor, the smallest included (the q / k biases, 0.4-3 % of the largest norm), clears the plain bf16 bar (cosine >
0.995) in the CPU double and on the HIP kernels -- lowest cosine 0.99980 in both -- so the tests use no wider bar for the small ones;
the bf16-mode oracle (oracle/tasu_oracle.py with the LLM made trainable) against these fp32 values: not measured.

Run where the reference tree is present (CPU, a few seconds):  python tools/make_golden_full_ft.py
Fixtures are data (seeds + the reference's outputs); weights come from ps_slm_amd.synthetic (seeded), nothing is copied.
"""
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.make_golden import quiet, save  # noqa: E402
from oracle.ref_import import build_reference_model  # noqa: E402


def main():
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, random_state_dict, synthetic_text_batch

    seed_w, seed_b = 2026, 31
    for name, tied in (("mid_text_full_ft", True), ("mid_text_full_ft_untied", False)):
        geo = Geometry.from_dict(dict(MID_GEOMETRY, tied=tied))
        gd = dataclasses.asdict(geo)
        sd = random_state_dict(geo, seed_w, with_encoder=True)
        batch = synthetic_text_batch(geo, 3, seed=seed_b, prompt_len=9, n_audio=21, target_len=17, speech_pos=4,
                                     feat_frames=12, noise=True, drop_prob=0.15, ragged=True)
        kept = [list(np.asarray(q)[np.asarray(k, dtype=bool)]) for q, k in zip(batch["post_ids"], batch["keeps"])]
        GT = [" ".join(map(str, k)) for k in kept]
        cols = torch.randperm(geo.llm_vocab, generator=torch.Generator().manual_seed(5))[:64].sort().values
        model = build_reference_model(gd, 0, dict(gt_emb=True, gt_emb_noise=False))
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected and set(missing) <= {"llm.lm_head.weight"}
        assert (model.llm.lm_head.weight is model.llm.get_input_embeddings().weight) == tied
        for q in model.llm.parameters():                                   # freeze_llm = false: ps-slm.py:105-108 freezes nothing
            q.requires_grad = True
        model.llm.train()
        out, acc = quiet(model, input_ids=batch["input_ids"], input_features=batch["input_features"],
                         attention_mask=batch["attention_mask"], input_feature_length=batch["input_feature_length"], GT=GT,
                         labels=batch["labels"])
        out.loss.backward()
        lg = out.logits.detach().float()
        ids, am = batch["input_ids"], batch["attention_mask"].bool()
        looked = torch.unique(ids[am & (ids != geo.speech_id)])
        perm = torch.randperm(geo.llm_vocab, generator=torch.Generator().manual_seed(6))
        others = perm[~torch.isin(perm, looked)][:64]
        erows = torch.cat([looked, others]).sort().values
        arrs = dict(seed_w=seed_w, seed_b=seed_b, tied=int(tied), loss=out.loss.detach().float(), acc=torch.as_tensor(acc).float(),
                    cols=cols, logits_cols=lg[:, :, cols], lse=torch.logsumexp(lg, -1), egrad_rows=erows)
        for n, prm in model.encoder_projector.named_parameters():
            if n != "ffn.0.weight":
                arrs["grad." + n] = prm.grad.clone()
        norms, n_par = {}, 0
        for n, prm in model.llm.named_parameters():                        # (a tied lm_head is the table: listed once)
            key, g = "llm." + n, prm.grad.detach().float()
            norms[key] = float(g.norm())
            n_par += g.numel()
            sub = g[erows] if n == "model.embed_tokens.weight" else (g if g.dim() == 1 else g[::4, ::4])
            scale = 2.0 ** int(np.floor(np.log2(1024.0 / float(sub.abs().max()))))   # fp16 keeps 11 bits at any magnitude then
            arrs["gnorm." + key] = np.float32(norms[key])
            arrs["gscale." + key] = np.float32(scale)
            arrs["g." + key] = (sub * scale).half()
        big = max(norms.values())
        low = sorted(norms.items(), key=lambda kv: kv[1])[:3]
        assert low[0][1] >= 1e-3 * big, low
        save(name, **arrs)
        print(name, "loss", f"{float(out.loss.detach()):.6f}", "acc", float(acc), "gradient tensors", len(norms), "parameters", n_par,
              "smallest norms / largest:", [(k, f"{v / big:.2e}") for k, v in low])


if __name__ == "__main__":
    main()
