"""TEST INFRASTRUCTURE ONLY -- tests/golden/mid_text_lora_emb.npz (tied head) and mid_text_lora_emb_untied.npz: the REAL reference
model (imported through oracle/ref_import.py) at the "mid" geometry with the LoRA formula applied by hand (oracle/lora_oracle.py)
and ``train_config.use_emb``'s effect restated: ``requires_grad = True`` on every LLM parameter whose name contains ``embed_tokens``
(Multitask/model/ps-slm.py:119-123).  fp32, one text-branch training step on the seeds, batch and LoRA case of mid_text_lora
(oracle/make_golden_lora.py): loss, accuracy, sampled logit columns, the projector's and the adapters' gradients, and for the
embedding table the L2 norm of EVERY gradient row (fp32) plus, in fp16 (scaled by the power of two ``egrad_scale``), all rows the
batch looks up and 64 seeded other rows.

Run where the reference tree is present (CPU, a few seconds):  python tools/make_golden_use_emb.py
Expected: mid_text_lora_emb loss 7.367513 (1000 of 1000 rows non-zero), mid_text_lora_emb_untied loss 7.158842 (60 of 1000).
Fixtures are data (seeds + the reference's outputs); weights come from ps_slm_amd.synthetic (seeded), nothing is copied.
"""
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.lora_oracle import apply_hand_lora  # noqa: E402
from oracle.make_golden import quiet, save  # noqa: E402
from oracle.make_golden_lora import CASES  # noqa: E402
from oracle.ref_import import build_reference_model  # noqa: E402


def main():
    from ps_slm_amd.lora import LoraConfig
    from ps_slm_amd.model import Geometry
    from ps_slm_amd.synthetic import MID_GEOMETRY, random_lora_state_dict, random_state_dict, synthetic_text_batch

    seed_w, seed_b, seed_l = 2026, 31, 909
    r, alpha, targets, p, _ = CASES["mid_text_lora"]
    cfg = LoraConfig(r=r, lora_alpha=alpha, lora_dropout=p, target_modules=targets)
    for name, tied in (("mid_text_lora_emb", True), ("mid_text_lora_emb_untied", False)):
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
        lparams = apply_hand_lora(model.llm, random_lora_state_dict(geo, cfg, seed_l), targets, cfg.scaling, p, None)
        emb = [(n, q) for n, q in model.llm.named_parameters() if "embed_tokens" in n]         # ps-slm.py:119-123
        assert [n for n, _ in emb] == ["model.embed_tokens.weight"]
        assert (model.llm.lm_head.weight is model.llm.get_input_embeddings().weight) == tied
        table = emb[0][1]
        table.requires_grad = True
        out, acc = quiet(model, input_ids=batch["input_ids"], input_features=batch["input_features"],
                         attention_mask=batch["attention_mask"], input_feature_length=batch["input_feature_length"], GT=GT,
                         labels=batch["labels"])
        out.loss.backward()
        assert tied or model.llm.lm_head.weight.grad is None
        lg = out.logits.detach().float()
        eg = table.grad.detach().float()
        norms = eg.norm(dim=1)
        ids, am = batch["input_ids"], batch["attention_mask"].bool()
        looked = torch.unique(ids[am & (ids != geo.speech_id)])
        perm = torch.randperm(geo.llm_vocab, generator=torch.Generator().manual_seed(6))
        others = perm[~torch.isin(perm, looked)][:64]
        erows = torch.cat([looked, others]).sort().values
        escale = 2.0 ** int(np.floor(np.log2(1024.0 / float(eg[erows].abs().max()))))           # fp16 keeps 11 bits at any magnitude then
        arrs = dict(seed_w=seed_w, seed_b=seed_b, seed_l=seed_l, r=r, alpha=alpha, p=p, rng=np.asarray((0, 0)), tied=int(tied),
                    targets=np.asarray(",".join(targets)), loss=out.loss.detach().float(), acc=torch.as_tensor(acc).float(),
                    cols=cols, logits_cols=lg[:, :, cols], lse=torch.logsumexp(lg, -1),
                    egrad_norms=norms, egrad_rows=erows, egrad_scale=np.float32(escale), egrad=(eg[erows] * escale).half())
        for n, prm in model.encoder_projector.named_parameters():
            if n != "ffn.0.weight":
                arrs["grad." + n] = prm.grad.clone()
        for k, prm in lparams.items():
            arrs["lgrad." + k] = prm.grad.clone().half()
        save(name, **arrs)
        print(name, "loss", f"{float(out.loss.detach()):.6f}", "acc", float(acc), "non-zero table gradient rows", int((norms > 0).sum()),
              "of", geo.llm_vocab, "looked up", len(looked))


if __name__ == "__main__":
    main()
