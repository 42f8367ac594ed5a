"""TEST INFRASTRUCTURE ONLY -- tests/golden/step_trace.txt: the operator calls of one bf16 training step of the decoder, per recipe,
recorded on the CPU double.  The step is replayed as a hipGraph on buffers that the layers alias on purpose, so the ORDER of the
launches and the IDENTITY of every buffer argument are part of its contract; this file pins both (tests/test_step_trace_cpu.py
regenerates the traces and compares them line for line).

The recorder forwards every call to the double (values stay real) and logs one line per call: the operator and every argument.
Scalars by repr; a tensor as ``name+offset(shape)`` (``+0`` left out) and, unless it is contiguous, ``(stride)``: ``name`` is its workspace buffer
(``model._ws``), else the tensor it is a view of among the model's own -- a layer weight ``L<l>.<key>``, ``wext`` / ``as`` / ``bts`` /
``at`` by their keys, ``proj.p`` / ``g`` / ``pb`` by offset (the weights of a fully fine-tuned decoder are such ranges).  The
gradient-exchange hook logs its ranges in place.  The recipes share most of their calls, so the file writes a call out once: a line
``=N`` stands for the text of line N of the file (write_golden / read_golden).

A change that moves a launch on purpose refreshes the file (python tools/make_golden_step_trace.py) and shows the diff.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from full_ft_ops import FullFtFakeOps  # noqa: E402
from ps_slm_amd.lora import LoraConfig, merged_llm  # noqa: E402
from ps_slm_amd.model import Geometry, TasuModel  # noqa: E402
from ps_slm_amd.synthetic import MID_GEOMETRY, random_lora_state_dict, random_state_dict, synthetic_text_batch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_trace.txt")


class GroupOps(FullFtFakeOps):
    """The double + the optional per-group entry points the host code looks for with hasattr (HipOps has them): member by member,
    as tests/lora_ref64.py runs them."""

    def gemm_rank_group(self, As, Bs, Cs, M, N, Ks):
        for a, b, c, K in zip(As, Bs, Cs, Ks):
            self.gemm_rank(a, b, c, M, N, K)

    def lora_apply_group(self, y, us, ws, M, N, R, sids, s=1.0, p=0.0, rng=None):
        for u, w, sid in zip(us, ws, sids):
            self.lora_apply(y, u, w, M, N, R, s=s, p=p, rng=rng, sid=sid)

    def lora_dropout_norm_group(self, x, w, rstd, dsts, M, D, p, rng, sids):
        for dst, sid in zip(dsts, sids):
            self.lora_dropout_norm(x, w, rstd, dst, M, D, p, rng, sid)


class Recorder:
    """Wraps an operator set: every call is forwarded and, while ``lines`` is a list, logged."""

    def __init__(self, ops):
        self._ops, self.lines, self.model, self._own = ops, None, None, {}

    def __getattr__(self, name):                           # (hasattr on the recorder answers for the wrapped set)
        f = getattr(self._ops, name)
        if not callable(f) or name == "alt_workspace":
            return f

        def call(*a, **k):
            if self.lines is not None:
                self.lines.append(" ".join([name] + [self.fmt(v) for v in a] + [f"{n}={self.fmt(v)}" for n, v in k.items()]))
            return f(*a, **k)
        return call

    def start(self, model):
        """Names of the model's own tensors by their storage, built once the model is complete."""
        self.model, self._own, m = model, {}, model
        named = [("proj." + n, t) for n, t in vars(m.proj).items()]        # the bucket (p, g, m, v, pb), then the projector's working copies
        for tag, llm in (("", m.llm), ("merged.", getattr(m.lora, "_merged", None))):
            if llm is not None:
                named += [(f"{tag}L{l}.{k}", t) for l, w in enumerate(llm.layers) for k, t in w.items()]
                named += [(tag + k, getattr(llm, k)) for k in ("embed", "head", "head_t", "norm")]
        if m.lora is not None:
            named.append(("lora.rng", m.lora.rng))
            for tag, d in (("wext", m.lora.wext), ("as", m.lora.as_), ("bts", m.lora.bts), ("at", m.lora.at)):
                named += [(f"{tag}[{k[0]},{k[1]}]", t) for k, t in d.items()]
        for n, t in named:
            if isinstance(t, torch.Tensor):
                self._own.setdefault(t.untyped_storage().data_ptr(), n)
        self.lines = []

    def fmt(self, v):
        if isinstance(v, (list, tuple)):
            return "[" + " ".join(self.fmt(x) for x in v) + "]"
        if not isinstance(v, torch.Tensor):
            return repr(v)
        base = v.untyped_storage().data_ptr()
        name = next((n for n, t in self.model._ws.items() if t.untyped_storage().data_ptr() == base), None) or self._own.get(base)
        if name is None:
            raise KeyError(f"a tensor argument {tuple(v.shape)} {v.dtype} that is neither a workspace buffer nor one of the model's")
        s = name + (f"+{v.storage_offset()}" if v.storage_offset() else "") + f"({','.join(map(str, v.shape))})"
        return s if v.is_contiguous() else s + f"({','.join(map(str, v.stride()))})"


BATCHES = (("M64", dict(B=2, n_audio=7, ragged=False)), ("M138", dict(B=3, n_audio=21, ragged=True)))     # M % 64 == 0, and not
ALL7 = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
LORA = dict(r16=dict(r=16, p=0.0), r16_drop=dict(r=16, p=0.1), r8_qvu=dict(r=8, targets=("q_proj", "v_proj", "up_proj")),
            r128_qkod=dict(r=128, targets=("q_proj", "k_proj", "o_proj", "down_proj")))


def recipes():
    """name -> keyword arguments of trace()"""
    out = {"frozen_tail": dict(keep_logits=False), "frozen_no_tail": dict(keep_logits=False, tail_rows=False),
           "frozen_keep_logits": dict(), "frozen_forward_only": dict(need_backward=False), "frozen_rows_none": dict(logits_rows="none")}
    for n, kw in LORA.items():
        out["lora_" + n] = dict(lora=kw)
        out["lora_" + n + "_grouped"] = dict(lora=kw, grouped=True)
    for n, kw in (("spans", dict(hook=True)), ("freeze_projector", dict(freeze_projector=True)), ("use_emb", dict(use_emb=True)),
                  ("use_emb_untied", dict(use_emb=True, tied=False)), ("merged_prefill", dict(merged=True, need_backward=False, logits_rows="none"))):
        out["lora_" + n] = dict(lora=LORA["r16_drop"], grouped=True, **kw)
    for n, kw in (("", {}), ("_untied", dict(tied=False))):
        out["full_ft" + n] = dict(full_ft=True, keep_logits=False, **kw)
        out["full_ft" + n + "_hook"] = dict(full_ft=True, keep_logits=False, hook=True, **kw)
    return out


def trace(batch, keep_logits=True, tail_rows=True, need_backward=True, logits_rows="all", lora=None, grouped=False, hook=False,
          freeze_projector=False, use_emb=False, tied=True, merged=False, full_ft=False):
    geo = Geometry.from_dict(dict(MID_GEOMETRY, llm_layers=3, tied=tied))
    sd = random_state_dict(geo, 2026, with_encoder=False)
    ops = Recorder(GroupOps() if grouped else FullFtFakeOps())
    m = TasuModel(geo, ops, "cpu", keep_logits=keep_logits)
    m.tail_rows = tail_rows
    m.load_reference_state_dict(sd)
    if lora is not None:
        cfg = LoraConfig(r=lora["r"], lora_alpha=32, lora_dropout=lora.get("p", 0.0), target_modules=lora.get("targets", ALL7))
        m.enable_lora(cfg)
        m.lora.load_state_dict(random_lora_state_dict(geo, cfg, 7))
        if use_emb:
            m.enable_embedding_training()
        m.sync_projector_copies()
    if full_ft:
        m.enable_llm_training(sd)
    m.freeze_projector = freeze_projector
    b = synthetic_text_batch(geo, batch["B"], seed=31, prompt_len=9, n_audio=batch["n_audio"], target_len=17, speech_pos=4, feat_frames=12,
                             noise=False, ragged=batch["ragged"])
    st = m.prepare_text(b["input_ids"], b["attention_mask"], b["labels"], b["post_ids"])
    m.forward_projector_text(st)
    if merged:                                             # the decode prefill: merged weights, no adapter runner (ps_slm_amd/decode.py)
        m.llm, m._lora_run = merged_llm(m), None
    ops.start(m)
    m.forward_llm(st, need_backward=need_backward, logits_rows=logits_rows, compute_loss=not merged)
    if need_backward and logits_rows != "none":
        if hook:
            m.run_backward(st, on_ready=lambda lo, hi: ops.lines.append(f"on_ready {lo} {hi}"), w1_chunks=2)
        else:
            m.backward(st)
    return st.M, ops.lines


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


def write_golden(lines, path=GOLDEN):
    first = {}
    with open(path, "w") as f:
        for n, line in enumerate(lines, 1):
            f.write((f"={first[line]}" if line in first else line) + "\n")
            first.setdefault(line, n)


def read_golden(path=GOLDEN):
    lines = open(path).read().splitlines()
    for n, line in enumerate(lines):
        if line.startswith("=") and not line.startswith("=="):
            lines[n] = lines[int(line[1:]) - 1]
    return lines


if __name__ == "__main__":
    lines = generate()
    write_golden(lines)
    assert read_golden() == lines
    print(GOLDEN, sum(l.startswith("==") for l in lines), "traces,", len(lines), "lines")
