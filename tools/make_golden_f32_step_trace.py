"""TEST INFRASTRUCTURE ONLY -- tests/golden/f32_step_trace.txt: the operator calls of one fp32 training step (ps_slm_amd/train_fp32.py:
forward_train_fp32 + run_backward), per recipe, recorded on the CPU double tests/f32_step_ops.py.  The fp32 step's sums are
order-dependent by design (K ascending, slabs in ascending order), so the ORDER of its launches, their scalars and the buffer behind
every tensor argument fix the bits of the loss and the gradients; this file pins them (tests/test_f32_step_trace_cpu.py regenerates
the traces and compares them line for line).  The recorder, the line format, the ``=N`` encoding and the two batches are those of
tools/make_golden_step_trace.py; the names added here: ``f32.L<l>.<key>`` / ``f32.head`` for the fp32 weight set, ``f32t.`` for its
transposed copies, ``lora32[<l>,<target>].<copy>`` for LoraF32's working copies, ``merged32.`` for the merged fp32 set.

A change that moves a launch on purpose refreshes the file (python tools/make_golden_f32_step_trace.py) and shows the diff.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from f32_step_ops import F32StepOps, f32_step_model  # noqa: E402
from make_golden_step_trace import ALL7, BATCHES, Recorder, read_golden, write_golden  # noqa: E402,F401
from ps_slm_amd.lora import LoraConfig  # noqa: E402
from ps_slm_amd.model import Geometry  # noqa: E402
from ps_slm_amd.synthetic import MID_GEOMETRY, qwen3_state_dict, random_lora_state_dict, random_state_dict, synthetic_text_batch  # noqa: E402
from ps_slm_amd.train_fp32 import _transposed_weights, forward_train_fp32, lora_f32  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "f32_step_trace.txt")


class F32Recorder(Recorder):
    def start(self, model):
        """The base names, then the fp32 sets.  The transposed copies and the adapters' working copies are made by plain torch at
        their first use: they are made here, before the first recorded call, so that they have names."""
        super().start(model)
        m, named = model, []
        sets = [("f32.", m.llm.f32), ("f32t.", _transposed_weights(m)), ("merged32.", getattr(m.lora, "_merged32", None))]
        for tag, s in sets:
            if s:
                named += [(f"{tag}L{l}.{k}", t) for l, w in enumerate(s["layers"]) for k, t in w.items()] + [(tag + "head", s["head"])]
        if m.lora is not None:
            named += [(f"lora32[{l},{t}].{k}", v) for (l, t), w in lora_f32(m).weights().items() for k, v in w.items()]
        for n, t in named:
            if isinstance(t, torch.Tensor):
                self._own.setdefault(t.untyped_storage().data_ptr(), n)


LORA = dict(r16=dict(r=16, p=0.0), r16_drop=dict(r=16, p=0.1), r8_qvu=dict(r=8, targets=("q_proj", "v_proj", "up_proj")))


def recipes():
    """name -> keyword arguments of trace()"""
    out = {"frozen": dict(), "frozen_hook": dict(hook=True), "freeze_projector": dict(freeze_projector=True),
           "linear_k2": dict(projector="linear"), "cov1d_k2": dict(projector="cov1d-linear"), "cross_attention": dict(projector="cross-attention")}
    for n, kw in LORA.items():
        out["lora_" + n] = dict(lora=kw)
    out.update(lora_use_emb=dict(lora=LORA["r16"], use_emb=True), lora_use_emb_untied=dict(lora=LORA["r16"], use_emb=True, tied=False),
               full_ft=dict(full_ft=True), full_ft_untied=dict(full_ft=True, tied=False),
               full_ft_tn=dict(full_ft=True, f32_route="tn"), full_ft_composed=dict(full_ft=True, f32_route="composed"),
               qwen3=dict(qwen3=True), qwen3_full_ft=dict(qwen3=True, full_ft=True))
    return out


def geometry(projector="linear-silu", tied=True, qwen3=False):
    g = dict(MID_GEOMETRY, llm_layers=3, tied=tied, projector=projector)
    if projector in ("linear", "cov1d-linear"):
        g.update(projector_ds_rate=2)
    if qwen3:
        g.update(qk_norm=True, qkv_bias=False)
    return Geometry.from_dict(g)


def build(geo, lora=None, use_emb=False, full_ft=False, f32_route=None, freeze_projector=False):
    """(model on the bare double, state dict).  The capability probes look at the operator set's class, so the recorder goes in
    afterwards (step())."""
    sd = (qwen3_state_dict if geo.qk_norm else random_state_dict)(geo, 2026, with_encoder=False)
    m = f32_step_model(geo, sd, F32StepOps())
    if lora is not None:
        cfg = LoraConfig(r=lora["r"], lora_alpha=32, lora_dropout=lora.get("p", 0.0), target_modules=lora.get("targets", ALL7))
        m.enable_lora(cfg)
        m.lora.load_state_dict(random_lora_state_dict(geo, cfg, 7))
        if use_emb:
            m.enable_embedding_training()
        m.sync_projector_copies()
    if full_ft:
        m.enable_llm_training(sd)
        m.full_ft.f32_route = f32_route
    m.freeze_projector = freeze_projector
    return m, sd


def text_batch(geo, batch):
    """The bf16 tool's batch; a projector that joins k frames per row gets k times the frames, so that M is the batch's M."""
    return synthetic_text_batch(geo, batch["B"], seed=31, prompt_len=9, n_audio=batch["n_audio"] * geo.projector_ds_rate, target_len=17,
                                speech_pos=4, feat_frames=12, noise=False, ragged=batch["ragged"])


def step(m, b, hook=False, record=True):
    """One fp32 step; returns (state, the recorded lines or None)."""
    st = m.prepare_text(b["input_ids"], b["attention_mask"], b["labels"], b["post_ids"])
    ops = m.ops
    if record:
        m.ops = rec = F32Recorder(ops)
        rec.start(m)
    try:
        forward_train_fp32(m, st)
        m.run_backward(st, on_ready=(lambda lo, hi: rec.lines.append(f"on_ready {lo} {hi}")) if hook else None)
    finally:
        m.ops = ops
    return st, (rec.lines if record else None)


def trace(batch, hook=False, projector="linear-silu", tied=True, qwen3=False, **kw):
    geo = geometry(projector, tied, qwen3)
    m, _ = build(geo, **kw)
    st, lines = step(m, text_batch(geo, batch), hook)
    return st.M, lines


def generate():
    """The whole file as a list of lines: ``== recipe batch M=<rows> calls=<n>`` and the calls."""
    out = []
    for name, kw in recipes().items():
        for bname, batch in BATCHES:
            M, lines = trace(batch, **kw)
            assert (M % 64 == 0) == (bname == "M64"), (bname, M)
            out.append(f"== {name} {bname} M={M} calls={len(lines)}")
            out += lines
    return out


if __name__ == "__main__":
    lines = generate()
    write_golden(lines, GOLDEN)
    assert read_golden(GOLDEN) == lines
    print(GOLDEN, sum(l.startswith("==") for l in lines), "traces,", len(lines), "lines,", os.path.getsize(GOLDEN), "bytes")
