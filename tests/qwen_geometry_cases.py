"""The Qwen2.5 head- and vocabulary-geometry fixtures (tests/golden/qwen15_geo.npz, qwen7_geo.npz; oracle/make_golden_qwen_geometry.py):
the decoder widths, heads, RoPE theta and vocabularies of Qwen2.5-1.5B (12 query / 2 KV heads, tied, V = 151,936) and Qwen2.5-7B
(28 / 4 heads, untied lm_head, V = 152,064) with fewer decoder layers, and the shipped linear-silu projector over the full CTC
vocabulary (K = 25,055).  Only seeds, prompts and the REAL reference's outputs are stored; weights and the training batch are
regenerated here from the seeds."""
import dataclasses

import numpy as np
import torch

from ps_slm_amd.model import Geometry
from ps_slm_amd.synthetic import random_state_dict, synthetic_text_batch

FIXTURES = {"qwen15_geo": ("qwen25_1p5b", 2), "qwen7_geo": ("qwen25_7b", 1)}
# ragged, right-padded text branch (the mid_text_clean recipe: the clean posterior of the ids the CPS drop keeps); S = 126 and 120, not a
# multiple of the attention tiles
BATCH = dict(prompt_len=24, n_audio=60, target_len=48, speech_pos=9, feat_frames=4, noise=True, drop_prob=0.15, ragged=True)
N_COLS = 64          # seeded logit columns kept per position
N_SAMPLE = 4096      # seeded elements kept of each projector weight gradient


def geometry(name):
    base, layers = FIXTURES[name]
    return dataclasses.replace(getattr(Geometry, base)(), llm_layers=layers)


def state_dict(geo, seed_w):
    return random_state_dict(geo, seed_w, with_encoder=False)


def text_batch(geo, seed_b):
    batch = synthetic_text_batch(geo, 3, seed=seed_b, **BATCH)
    batch["post_ids"] = [list(np.asarray(p)[np.asarray(k, dtype=bool)]) for p, k in zip(batch["post_ids"], batch["keeps"])]
    del batch["alphas"], batch["keeps"]
    return batch


def generate_cases(z):
    """[(input_ids, attention_mask, post_ids, reference tokens, smallest beam-score margin)] of a fixture."""
    from conftest import split_flat
    return [(torch.from_numpy(z[f"c{n}_input_ids"]), torch.from_numpy(z[f"c{n}_attention_mask"]),
             split_flat(z[f"c{n}_post_ids_flat"], z[f"c{n}_post_lens"]), z[f"c{n}_tokens"], float(z[f"c{n}_margin"]))
            for n in range(int(z["n_cases"]))]


def swap_kv_heads(sd, layer, geo):
    """The state dict with KV heads 0 and 1 of ``layer`` exchanged (k and v projections, weights and biases): a q -> kv head
    mapping error that a single-KV-head geometry cannot show."""
    out = dict(sd)
    hd = 128
    for n in ("k_proj", "v_proj"):
        for t in ("weight", "bias"):
            k = f"llm.model.layers.{layer}.self_attn.{n}.{t}"
            w = sd[k].clone()
            w[:hd], w[hd:2 * hd] = sd[k][hd:2 * hd], sd[k][:hd]
            out[k] = w
    assert geo.llm_kv_heads >= 2
    return out
