"""TEST INFRASTRUCTURE ONLY -- tests/golden/mid_qwen3_full_ft.npz (tied head) and mid_qwen3_full_ft_untied.npz: the REAL reference
(the imported slam_model_asr through oracle/ref_import.py) with a seeded ``transformers.Qwen3ForCausalLM`` in place of its ``llm``
(tools/make_golden_qwen3.py: reference_with_qwen3) at the "mid" Qwen3 geometry, and what ``train_config.freeze_llm = false`` does
to it restated: every parameter of ``model.llm`` has ``requires_grad = True`` and the LLM is in training mode
(Multitask/model/ps-slm.py:105-108).  fp32, one text-branch training step on the seeds, weight scale and batch of mid_qwen3_step
(seed_w 2027, N(0, 0.15) linears, seed_b 31): loss, accuracy, sampled logit columns, the projector's gradients except ffn.0.weight,
and for EVERY tensor of Qwen3ForCausalLM -- the q_norm / k_norm weights [128] of every layer among them, no bias -- its full
gradient norm (fp32, ``gnorm.<key>``) and values in fp16 scaled by a power of two (``g.<key>`` / ``gscale.<key>``), on the sub-grids
of tools/make_golden_full_ft.py: all of a 1-D tensor, every 4th row and column of a matrix, and for the embedding table the rows
the batch looks up plus 64 seeded others (``egrad_rows``).

The generator asserts that no tensor's gradient norm is below 1e-3 of the largest, so that relative bars on every tensor mean
something; it prints the three smallest.

Run where the reference tree is present (CPU, a few seconds):  python tools/make_golden_qwen3_full_ft.py
Fixtures are data (seeds + the reference's outputs); weights come from ps_slm_amd.synthetic.qwen3_state_dict (seeded), nothing is
copied.
"""
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_qwen3 import SCALE_STEP, SEED_B, SEED_STEP, reference_with_qwen3  # noqa: E402
from oracle.make_golden import quiet, save  # noqa: E402


def main():
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, qwen3_state_dict, synthetic_text_batch

    for name, tied in (("mid_qwen3_full_ft", True), ("mid_qwen3_full_ft_untied", False)):
        geo = Geometry.from_dict(dict(MID_GEOMETRY, qk_norm=True, qkv_bias=False, tied=tied))
        gd = dataclasses.asdict(geo)
        sd = qwen3_state_dict(geo, SEED_STEP, with_encoder=True, scale=SCALE_STEP)
        batch = synthetic_text_batch(geo, 3, seed=SEED_B, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12,
                                     noise=False, ragged=True)
        GT = [" ".join(map(str, p)) for p in batch["post_ids"]]
        cols = torch.randperm(geo.llm_vocab, generator=torch.Generator().manual_seed(5))[:64].sort().values
        model = reference_with_qwen3(geo, gd, sd, dict(gt_emb=True, gt_emb_noise=False))
        assert (model.llm.lm_head.weight is model.llm.get_input_embeddings().weight) == tied
        assert tied or torch.equal(model.llm.lm_head.weight, sd["llm.lm_head.weight"])
        for q in model.llm.parameters():                                   # freeze_llm = false: ps-slm.py:105-108 freezes nothing
            q.requires_grad = True
        model.llm.train()                                                  # (no dropout anywhere: attention_dropout = 0)
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
        arrs = dict(seed_w=SEED_STEP, seed_b=SEED_B, scale=SCALE_STEP, tied=int(tied), loss=out.loss.detach().float(),
                    acc=torch.as_tensor(acc).float(), cols=cols, logits_cols=lg[:, :, cols], egrad_rows=erows)
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
        assert sum(k.endswith(("q_norm.weight", "k_norm.weight")) for k in norms) == 2 * geo.llm_layers and not any(k.endswith(".bias") for k in norms)
        big = max(norms.values())
        low = sorted(norms.items(), key=lambda kv: kv[1])[:3]
        assert low[0][1] >= 1e-3 * big, low
        save(name, **arrs)
        print(name, "loss", f"{float(out.loss.detach()):.6f}", "acc", float(acc), "gradient tensors", len(norms), "parameters", n_par,
              "smallest norms / largest:", [(k, f"{v / big:.2e}") for k, v in low])


if __name__ == "__main__":
    main()
