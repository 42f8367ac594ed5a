"""Drop-in for the reference's model plugin ``model/ps-slm.py:model_factory`` (selected with
``++model_config.file=ps_slm_amd/ps_slm.py:model_factory``; contract: Multitask/model/ps-slm.py:130-181, loaded by
Multitask/utils/model_utils.py:9-33).  Same names, argument meaning and error behaviour; the arithmetic runs in
the HIP kernels of libtasu_hip.so through ps_slm_amd.model.TasuModel.

What callers get (Multitask/utils/deepspeed_utils.py:205-236, Multitask/inference_batch.py:139-151):
  model(**batch) -> (outputs, acc)   outputs.loss (0-dim fp32 device tensor with a grad_fn in training mode), outputs.logits [B,S,V] (bf16 view)
  model.generate(**batch) -> LongTensor [B, n_new]
  model.parameters() / named_parameters() / train() / eval() / state_dict() / load_state_dict(strict=False) with the
  reference's checkpoint keys ``encoder_projector.{norm,ffn.0,ffn.2}.{weight,bias}`` (Multitask/utils/checkpoint_handler.py:169-182)

Autograd glue (Multitask/finetune_deepspeed.py:127-149, Multitask/utils/deepspeed_utils.py:205-236): the model is not
an ``nn.Module`` (the frozen LLM and encoder weights live in kernel layouts and are not listed), but in training mode
``outputs.loss`` IS the result of a ``torch.autograd.Function`` over the trainable leaves ``parameters()`` lists (views of the flat
fp32 master buffer under the reference's names, the SAME objects on every call).  ``loss.backward()`` -- directly or through any
engine -- runs the hand-scheduled HIP backward (``TasuModel.run_backward``) once and hands each leaf its slice of the flat
gradient bucket, scaled by the incoming gradient; an optimizer built over ``model.parameters()`` then updates the masters in
place and the next ``forward`` / ``generate`` refreshes the bf16 working copies.  So the reference's loop body trains this plugin
with ``torch.optim.AdamW`` or DeepSpeed as it stands.  ``ps_slm_amd.engine.TasuEngine`` (the DeepSpeed engine's surface:
``backward(loss)`` / ``step()``) stays the FAST path: it ignores the graph, overlaps the gradient exchange with the backward and
runs the fused AdamW kernel.  A loss computed in eval mode has no saved activations behind it: it is an ``EngineLoss`` whose
``backward()`` raises and says so.
"""
import json
import logging
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import torch

# The reference loads a plugin with SourceFileLoader under the module name "<file name>", outside any package
# (Multitask/utils/dataset_utils.py:14-25), so this file cannot use package-relative imports: make the package importable
# by its absolute name from wherever the file lies, then import it like any other client would.
_PKG_PARENT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG_PARENT not in sys.path:
    sys.path.insert(0, _PKG_PARENT)

from ps_slm_amd.model import Geometry, TasuModel  # noqa: E402

logger = logging.getLogger(__name__)

# the LLM's input embedding table in a checkpoint (train_config.use_emb): peft's name under slam_model_asr.llm, the prefix of lora.key_of
EMBED_KEY = "llm.base_model.model.model.embed_tokens.weight"
from ps_slm_amd.full_ft import EMBED_KEY as FT_EMBED_KEY, is_llm_key  # noqa: E402  (a fully fine-tuned decoder: the reference's own module names)
DEFAULT_SPEECH_TOKEN = "<speech>"
DEFAULT_IGNORE_TOKEN = -100


# ------------------------------------------------------------------------------------------------ tokenizers
class SyntheticLLMTokenizer:
    """Stand-in used when ``llm_path`` holds no tokenizer files (the benchmark box has none): whitespace-separated
    integer strings <-> ids; any other word -> a deterministic ordinary id (so that cleaned training targets, which hold letters
    only -- speech_dataset_large.py:164 -- still have one token per word).  Exposes what the model and the entrypoints read
    (ps-slm.py:27,133-140,672-674)."""

    def __init__(self, geo: Geometry):
        self.eos_token_id = geo.eos_id
        self.pad_token_id = geo.eos_id
        self.bos_token_id = None
        self.default_speech_token = geo.speech_id
        self.default_ignore_token = DEFAULT_IGNORE_TOKEN
        self.vocab_size = geo.llm_vocab

    def encode(self, text):
        top = max(2, min(self.eos_token_id, self.vocab_size))          # ordinary ids: below the special tokens
        return [int(t) if t.lstrip("-").isdigit() else 1 + (sum((i + 1) * ord(c) for i, c in enumerate(t)) % (top - 1)) for t in text.split()]

    def batch_decode(self, ids, skip_special_tokens=True, **kw):
        out = []
        for row in ids.tolist() if isinstance(ids, torch.Tensor) else ids:
            toks = [t for t in row if not (skip_special_tokens and t in (self.eos_token_id, self.default_speech_token))]
            out.append(" ".join(map(str, toks)))
        return out


class SyntheticSentencePiece:
    """Stand-in for Multitask/model/tokenizer.py:SenseVoiceTokenizer when the BPE model file is absent:
    "12 7 3" -> [12, 7, 3]; any other word -> a deterministic id in [1, V)."""

    def __init__(self, vocab_size):
        self._v = vocab_size

    def encode(self, text):
        return [int(t) % self._v if t.isdigit() else 1 + sum(map(ord, t)) % (self._v - 1) for t in text.split()]

    @property
    def vocab_size(self):
        return self._v


def setup_tokenizer(train_config, model_config, geo, **kwargs):
    path = model_config.get("llm_path", None)
    if path and os.path.isfile(os.path.join(path, "tokenizer_config.json")):
        from transformers import AutoTokenizer
        tok = AutoTokenizer.from_pretrained(path)
        tok.pad_token_id = tok.eos_token_id
        tok.add_special_tokens({"additional_special_tokens": [DEFAULT_SPEECH_TOKEN]})
        tok.default_ignore_token = DEFAULT_IGNORE_TOKEN
        tok.default_speech_token = tok.convert_tokens_to_ids(DEFAULT_SPEECH_TOKEN)
        return tok
    return SyntheticLLMTokenizer(geo)


def setup_encoder_tokenizer(model_config, geo):
    path = model_config.get("encoder_path", None)
    if path and os.path.isfile(os.path.join(path, "chn_jpn_yue_eng_ko_spectok.bpe.model")):
        import sentencepiece as spm
        sp = spm.SentencePieceProcessor(model_file=os.path.join(path, "chn_jpn_yue_eng_ko_spectok.bpe.model"))
        return SimpleNamespace(encode=lambda t: sp.encode(t, out_type=int), vocab_size=sp.vocab_size())
    return SyntheticSentencePiece(geo.ctc_vocab)


# ------------------------------------------------------------------------------------------------ geometry / weights
def geometry_from_config(model_config, raw_features=False) -> Geometry:
    """HF config.json under llm_path when present; otherwise a named synthetic geometry
    (``llm_path = synthetic:qwen2.5-1.5b | synthetic:qwen2.5-7b | synthetic:mid | synthetic:mid-untied`` -- the last one is the mid
    geometry with an lm_head of its own, the 7B's layout -- ``| synthetic:mid-qwen3 | synthetic:qwen3-1.7b``: Qwen3 decoders, a
    per-head q/k RMSNorm and no q|k|v bias).  ``model_type == "qwen3"`` in the config.json selects the Qwen3 route; every other
    value (or none) takes the Qwen2 route as before, except "qwen3_moe", which is refused."""
    path = str(model_config.get("llm_path", "") or "")
    is_mid = path.lower() in ("synthetic:mid", "synthetic:mid-untied", "synthetic:mid-qwen3")    # the test geometry: encoder_dim / llm_dim overrides do not apply
    cfg_file = os.path.join(path, "config.json")
    if os.path.isfile(cfg_file):
        c = json.load(open(cfg_file))
        mt = str(c.get("model_type", "qwen2")).lower()
        if mt == "qwen3_moe":
            raise NotImplementedError("model_type 'qwen3_moe': the mixture-of-experts MLP is not built; the dense Qwen3 decoders "
                                      "(model_type 'qwen3') are served, the MoE ones are a follow-up")
        if mt == "qwen3" and c.get("use_sliding_window", False):
            raise NotImplementedError("use_sliding_window=true: the attention kernels are full-causal only; sliding-window attention "
                                      "is a follow-up")
        hd = c.get("head_dim", c["hidden_size"] // c["num_attention_heads"])
        if hd != 128:
            raise ValueError(f"head_dim {hd} is not supported by the gfx950 attention kernels (128 only)")
        if mt == "qwen3" and c["num_attention_heads"] * 128 != c["hidden_size"]:
            raise ValueError(f"model_type 'qwen3' with num_attention_heads * 128 = {c['num_attention_heads'] * 128} != hidden_size "
                             f"{c['hidden_size']} (Qwen3-0.6B / 4B / 32B): q|k|v widths other than heads * 128 == hidden are a follow-up; "
                             "Qwen3-1.7B / 8B / 14B are served")
        geo = Geometry(llm_vocab=c["vocab_size"], llm_dim=c["hidden_size"], llm_inter=c["intermediate_size"],
                       llm_layers=c["num_hidden_layers"], llm_heads=c["num_attention_heads"],
                       llm_kv_heads=c["num_key_value_heads"], rope_theta=float(c.get("rope_theta", 1e6)),
                       rms_eps=float(c.get("rms_norm_eps", 1e-6)), tied=bool(c.get("tie_word_embeddings", True)),
                       qk_norm=mt == "qwen3", qkv_bias=mt != "qwen3")          # (any other model_type: the Qwen2 route, as before)
        if mt == "qwen3" and c.get("attention_bias", False):
            raise NotImplementedError("model_type 'qwen3' with attention_bias=true: the Qwen3 route's q|k|v projection is a plain GEMM "
                                      "(no released Qwen3 checkpoint carries the bias)")
    elif path.startswith("synthetic:"):
        name = path.split(":", 1)[1].lower()
        if name in ("qwen2.5-1.5b", "1.5b"):
            geo = Geometry.qwen25_1p5b()
        elif name in ("qwen2.5-7b", "7b"):
            geo = Geometry.qwen25_7b()
        elif name in ("mid", "mid-untied"):
            from ps_slm_amd.synthetic import MID_GEOMETRY
            geo = Geometry.from_dict(dict(MID_GEOMETRY, tied=name == "mid"))
        elif name == "mid-qwen3":
            from ps_slm_amd.synthetic import MID_GEOMETRY
            geo = Geometry.from_dict(dict(MID_GEOMETRY, qk_norm=True, qkv_bias=False))
        elif name in ("qwen3-1.7b", "qwen3-1p7b"):
            geo = Geometry.qwen3_1p7b()
        else:
            raise ValueError(f"unknown synthetic geometry {name!r}")
    else:
        raise FileNotFoundError(f"model_config.llm_path={path!r}: no config.json there and not a 'synthetic:<name>' spec")
    apply_encoder_config(geo, model_config.get("encoder_path", None))
    if raw_features:
        # train_config.ctc_posterior=false (ps-slm.py:515-523): model_config.encoder_dim is the width of the encoder states the
        # projector reads; the CTC vocabulary (PSD still decides on the posterior) stays the encoder's own
        ed = model_config.get("encoder_dim", None)
        if ed not in (None, geo.enc_dim) and not is_mid:
            raise ValueError(f"ctc_posterior=false: model_config.encoder_dim={ed} must be the encoder's output size {geo.enc_dim}")
        geo.proj_in = geo.enc_dim
    elif model_config.get("encoder_dim", None) not in (None, geo.ctc_vocab) and not is_mid:
        geo.ctc_vocab = int(model_config.encoder_dim)
    if model_config.get("llm_dim", None) not in (None, geo.llm_dim):
        raise ValueError(f"model_config.llm_dim={model_config.llm_dim} does not match the LLM hidden size {geo.llm_dim}")
    return geo


def apply_encoder_config(geo: Geometry, encoder_path):
    """funasr ships the encoder geometry in ``<encoder_path>/config.yaml`` (``input_size`` + ``encoder_conf``: the file
    funasr's AutoModel builds SenseVoiceSmall from, Multitask/model/ps-slm.py:91-106); absent file = the published
    SenseVoiceSmall values already in ``Geometry``."""
    cfg_file = os.path.join(str(encoder_path or ""), "config.yaml")
    if not os.path.isfile(cfg_file):
        return
    import yaml
    c = yaml.safe_load(open(cfg_file)) or {}
    ec = c.get("encoder_conf", {}) or {}
    for key, field in (("output_size", "enc_dim"), ("attention_heads", "enc_heads"), ("linear_units", "enc_ffn"),
                       ("num_blocks", "enc_blocks"), ("tp_blocks", "enc_tp_blocks"), ("kernel_size", "enc_kernel")):
        if key in ec:
            setattr(geo, field, int(ec[key]))
    if "input_size" in c:
        geo.feat_dim = int(c["input_size"])
    if int(ec.get("sanm_shfit", 0)) != 0:
        raise NotImplementedError("sanm_shfit != 0 is not what SenseVoiceSmall ships (SenseVoice.py:209-228 path only)")


def load_hf_llm_state_dict(path):
    """Reads HF Qwen2 ``*.safetensors`` shards under ``path`` into reference-named (``llm.``-prefixed) CPU tensors."""
    from safetensors.torch import load_file
    sd = {}
    for fn in sorted(os.listdir(path)):
        if fn.endswith(".safetensors"):
            for k, v in load_file(os.path.join(path, fn)).items():
                sd["llm." + k] = v.float()
    if not sd:
        raise FileNotFoundError(f"no .safetensors shards under {path}")
    return sd


def model_factory(train_config, model_config, **kwargs):
    """Same contract as Multitask/model/ps-slm.py:130-181: returns (model, tokenizer).  train_config.use_fp16 selects the arithmetic
    for Qwen2 and Qwen3 decoders alike: true -> the bf16-autocast path, false (the reference's shipped scripts) -> the fp32 kernels
    for generate(), evaluation and, where train_fp32.py serves the recipe, the training step.  A Qwen3 decoder (per-head q/k
    RMSNorm) in fp32 needs an operator set whose class has f32_qk_norm_rope / f32_qk_norm_bwd / f32_gemm_qkv_norm_rope (HipOps
    has them); with freeze_llm=false it needs qk_norm_wgrad (bf16 step) / f32_qk_norm_wgrad (fp32 step); with use_peft=true it is
    refused on either path."""
    projector = model_config.get("encoder_projector", "linear-silu")
    if projector == "q-former":
        # FINDING: the reference cannot run its q-former either.  EncoderProjectorQFormer.forward(x, atts) (projector.py:91-100)
        # takes the attention mask as a second argument and has no `.k`, but every call site of slam_model_asr passes one argument
        # and divides the lengths by `.k` (ps-slm.py:482,488,505,522, :612-651) -- TypeError "missing 1 required positional
        # argument: 'atts'"; with cross_attn=true the embedding table lands in `atts` and the merge fails on the 64 query rows
        # (reproduced with the imported reference: tests/test_oracle_golden.py::test_reference_cannot_run_its_q_former).
        raise NotImplementedError("encoder_projector='q-former': the reference's slam_model_asr cannot call EncoderProjectorQFormer "
                                  "(Multitask/model/projector.py:91 needs `atts`, ps-slm.py:482 passes one argument and reads `.k`); "
                                  "there is no behaviour to reproduce")
    if projector not in ("linear-silu", "linear", "cov1d-linear", "cross-attention"):
        raise NotImplementedError(f"encoder_projector={projector!r}: the MI355X path serves 'linear-silu' (the shipped recipe, "
                                  "Multitask/scripts/finetune_deespeed_sensevoice.sh:25), 'linear' (EncoderProjectorConcat, "
                                  "Multitask/model/projector.py:28-49), 'cov1d-linear' (EncoderProjectorCov1d, :53-73) and "
                                  "'cross-attention' (EncoderProjectorCTCCA, :104-126); q-former / simple_linear are not built")
    # train_config.freeze_llm = false (the dataclass default, aispeech_asr_config.py:116): setup_llm leaves every decoder parameter
    # trainable (ps-slm.py:105-108).  With use_peft=true peft freezes the base weights itself (the knob's help text says so): the LoRA
    # recipe, as with freeze_llm=true.  Without it the whole decoder trains (ps_slm_amd/full_ft.py): on the bf16-autocast step with
    # use_fp16=true, on the fp32 step (csrc/wgrad_f32.hip) with use_fp16=false wherever the model's training arithmetic is fp32
    full_ft = not train_config.get("freeze_llm", True)
    if full_ft and train_config.get("use_peft", False):
        logger.warning("train_config.freeze_llm is false with use_peft=true: peft freezes the base weights itself -- the LoRA recipe, "
                       "exactly what freeze_llm=true builds")
        full_ft = False
    # the fp32 kernels run on the GPU only: device "cpu" / an operator set without the f32_* weight-gradient operators has none
    device = kwargs.get("device", None)
    if device is None:
        device = f"cuda:{int(os.environ.get('LOCAL_RANK', train_config.get('device', 0) or 0))}"
    f32_wgrads = not str(device).startswith("cpu") and (kwargs.get("ops", None) is None or hasattr(kwargs["ops"], "f32_gemm_tn"))
    if full_ft and not train_config.get("use_fp16", False):
        if not f32_wgrads:
            raise NotImplementedError("train_config.freeze_llm=false with use_fp16=false: the decoder's fp32 weight gradients need the GPU's "
                                      "fp32 operators, which this device / operator set does not have; there full fine-tuning of the LLM "
                                      "runs on the bf16-autocast step -- set use_fp16=true (or freeze_llm=true: "
                                      "Multitask/scripts/finetune_deespeed_sensevoice.sh:84)")
        if not train_config.get("ctc_posterior", True):
            raise NotImplementedError("train_config.freeze_llm=false with use_fp16=false on raw encoder features (ctc_posterior=false): the "
                                      "fp32 step's decoder weight gradients serve the CTC-posterior branch; set use_fp16=true")
        if projector != "linear-silu" and train_config.get("mixed_precision", True):
            raise NotImplementedError(f"train_config.freeze_llm=false with use_fp16=false and mixed_precision=true on the {projector} "
                                      "projector: the model would train on the bf16 step and evaluate in fp32 -- set mixed_precision=false "
                                      "(fp32 everywhere: the decoder trains on the fp32 step) or use_fp16=true")
    if train_config.get("quantization", False):
        raise NotImplementedError("train_config.quantization (ps-slm.py:101-102: bitsandbytes 8-bit weights) is not built")
    if kwargs.get("peft_ckpt", None):
        raise NotImplementedError("peft_ckpt (a peft adapter DIRECTORY, ps-slm.py:110-112): load the adapters from the training "
                                  "checkpoint with ckpt_path instead -- it holds them under the reference's own key names")
    fp32_mode = not train_config.get("use_fp16", False)
    raw = not train_config.get("ctc_posterior", True)
    use_peft = bool(train_config.get("use_peft", False))
    # by default the training step in fp32 (ps_slm_amd/train_fp32.py) is selected for the linear-silu projector without adapters;
    # generate() and the eval-mode forward in fp32 (ps_slm_amd/decode_fp32.py) serve every projector and LoRA on the CTC-posterior branch
    f32_train_served = projector == "linear-silu" and not use_peft
    f32_eval_served = f32_train_served or not raw
    # train_config.mixed_precision (aispeech_asr_config.py:90; default true) chooses the arithmetic of the recipes whose fp32 training
    # step is newer than their bf16 one: with use_fp16 = false, mixed_precision = false means "no bf16 anywhere" -- the alternate
    # projectors and the LoRA adapters train in fp32 as well, and a recipe without an fp32 step is refused here instead of training in bf16 behind a log line
    no_bf16 = fp32_mode and not train_config.get("mixed_precision", True)
    # train_config.use_emb ("For llm input_embs", finetune_deespeed_sensevoice.sh:29,86): with use_peft the reference gives
    # requires_grad = True to every LLM parameter whose name contains embed_tokens (ps-slm.py:119-123); the check sits inside the
    # `elif train_config.use_peft` branch, so without use_peft the knob is never looked at
    use_emb = bool(train_config.get("use_emb", False))
    if use_emb and not use_peft:
        logger.warning("train_config.use_emb is true but use_peft is false: the reference only looks at use_emb inside its use_peft "
                       "branch (ps-slm.py:114-123) and ignores it here -- the embedding table stays frozen")
        use_emb = False
    if use_emb and no_bf16 and not f32_wgrads:
        raise NotImplementedError("train_config.use_emb with use_fp16=false and mixed_precision=false: the fp32 step's backward into the "
                                  "embedding table needs the GPU's fp32 operators, which this device / operator set does not have; there "
                                  "use_emb trains on the bf16-autocast step (use_fp16=true, or mixed_precision=true)")
    if no_bf16 and not f32_train_served:
        what = f"{projector} projector" + (" with LoRA adapters" if use_peft else "") + (" on raw encoder features" if raw else "")
        if raw:
            raise NotImplementedError(f"use_fp16=false with mixed_precision=false asks for fp32 everywhere; the {what} has no fp32 path "
                                      "(ctc_posterior=false: the raw-feature branch runs on the bf16 kernels)")
        f32_train_served = True
        logger.warning("train_config.use_fp16 and mixed_precision are false: the reference's fp32 arithmetic everywhere -- generate(), "
                       "evaluation and the training step of the %s run on the fp32 kernels (correctness mode: the training step is "
                       "~10x slower than with use_fp16=true)", what)
    elif fp32_mode:
        # the reference computes in fp32 unless use_fp16 wraps the step in bf16 autocast (deepspeed_utils.py:160,205) and ALWAYS
        # decodes in fp32 (inference_batch.py:113-117).  use_fp16 = false therefore selects the fp32 kernels for generate(), the
        # eval-mode forward and -- where train_fp32.py serves the model -- the training step; use_fp16 = true selects bf16 autocast
        # semantics, the path the benchmarks measure
        what = f"{projector} projector" + (" with LoRA adapters" if use_peft else "") + (" on raw encoder features" if raw else "")
        if f32_train_served:
            logger.warning("train_config.use_fp16 is false: the reference's fp32 arithmetic -- generate(), evaluation and the training step "
                           "of the %s run on the fp32 kernels (correctness mode: the training step is ~10x slower than with "
                           "use_fp16=true, which selects the bf16-autocast path the benchmarks measure)", what)
        elif f32_eval_served:
            logger.warning("train_config.use_fp16 is false: generate() and evaluation of the %s run on the fp32 kernels (the reference's "
                           "arithmetic); its training step runs on the bf16-autocast path (the fp32 training step serves the "
                           "linear-silu projector without LoRA only)", what)
        else:
            logger.warning("train_config.use_fp16 is false: the %s has the bf16-autocast path only (generate(), evaluation and the "
                           "training step); the fp32 kernels serve the CTC-posterior branch", what)
    if raw and projector == "cross-attention":
        raise NotImplementedError("ctc_posterior=false with the cross-attention projector: the reference's raw-feature branch "
                                  "(ps-slm.py:515-523) calls the projector with one argument, EncoderProjectorCTCCA needs two")
    geo = geometry_from_config(model_config, raw_features=raw)
    if geo.qk_norm:
        # Qwen3 (per-head q/k RMSNorm, csrc/qk_norm.hip): served on the bf16-autocast path and, for an operator set whose class has
        # the fp32 head-norm operators (HipOps does), on the fp32 path; with freeze_llm=false for one whose class has the head norms'
        # weight gradient in the training arithmetic; everything else is refused here, before
        # any weight is built or any device work starts (the probe reads the operator set's CLASS, never the instance)
        if fp32_mode:
            from ps_slm_amd.model import f32_qk_norm_missing
            missing = f32_qk_norm_missing(kwargs.get("ops", None))
            if missing:
                raise NotImplementedError("a Qwen3 decoder with train_config.use_fp16=false: this operator set has no fp32 q/k head norm "
                                          f"(missing: {', '.join(missing)}) for generate(), evaluation and the training step in fp32 -- "
                                          "set use_fp16=true, or use the HIP operator set")
        if use_peft:
            raise NotImplementedError("a Qwen3 decoder with train_config.use_peft=true: the LoRA route's K-extended q|k|v GEMM carries "
                                      "the RoPE epilogue and cannot take the head norm -- LoRA on Qwen3 is a follow-up; set use_peft=false")
        if full_ft:
            from ps_slm_amd.model import qk_norm_wgrad_missing
            f32_step = fp32_mode and f32_train_served and not str(device).startswith("cpu")
            missing = qk_norm_wgrad_missing(kwargs.get("ops", None), "fp32" if f32_step else "bf16")
            if missing:
                raise NotImplementedError("a Qwen3 decoder with train_config.freeze_llm=false: this operator set has no weight gradient "
                                          f"of the q_norm / k_norm weights (missing: {missing}); set freeze_llm=true, or use the HIP "
                                          "operator set")
    geo.projector = projector
    geo.projector_ds_rate = int(model_config.get("encoder_projector_ds_rate", 1) or 1) if projector in ("linear", "cov1d-linear") else 1
    tokenizer = setup_tokenizer(train_config, model_config, geo, **kwargs)
    if not isinstance(tokenizer, SyntheticLLMTokenizer):
        geo.speech_id, geo.eos_id = tokenizer.default_speech_token, tokenizer.eos_token_id
    ops = kwargs.get("ops", None)
    if ops is None:
        from ps_slm_amd.ops import HipOps     # raises if libtasu_hip.so is missing or there is no GPU: no fallback
        ops = HipOps()
    core = TasuModel(geo, ops, device, keep_logits=bool(kwargs.get("keep_logits", True)))
    if fp32_mode and device != "cpu" and not str(device).startswith("cpu") and f32_eval_served:
        core.arith = "fp32"
        core.arith_train = "fp32" if f32_train_served else "bf16"
        core.llm.keep_f32 = True                       # fp32 copies of the frozen weights next to the bf16 ones (before loading)
    llm_path = str(model_config.get("llm_path", ""))
    need_encoder = not train_config.get("gt_emb", False) or raw or bool(kwargs.get("with_encoder", False))
    if llm_path.startswith("synthetic:"):
        core.init_random(seed=int(kwargs.get("init_seed", 1234)), with_encoder=need_encoder)
    else:
        sd = load_hf_llm_state_dict(llm_path)
        core.llm.load_reference_state_dict(sd)
        core.init_projector_default(seed=int(train_config.get("seed", 42)))
        enc_pt = os.path.join(str(model_config.get("encoder_path", "")), "model.pt")
        if need_encoder:
            core.load_encoder_checkpoint(enc_pt)
    # train_config.freeze_projector (the shipped script carries the knob, finetune_deespeed_sensevoice.sh:46,80): the reference
    # honours it for the linear-silu projector only (ps-slm.py:47-54) and then trains whatever else requires a gradient
    frozen_proj = bool(train_config.get("freeze_projector", False)) and projector == "linear-silu"
    if frozen_proj and not train_config.get("use_peft", False) and not full_ft:
        raise ValueError("freeze_projector=true with use_peft=false and freeze_llm=true leaves nothing to train (the encoder is frozen "
                         "here): the reference's optimizer would receive an empty parameter list")
    core.freeze_projector = frozen_proj
    if train_config.get("use_peft", False):
        from ps_slm_amd.lora import LoraConfig
        core.enable_lora(LoraConfig.from_peft_config(train_config.get("peft_config", {}) or {}), seed=int(train_config.get("seed", 42)) + 7)
        logger.info("LoRA: r=%d alpha=%g dropout=%g on %s: %d adapter parameters", core.lora.cfg.r, core.lora.cfg.lora_alpha,
                    core.lora.cfg.lora_dropout, ",".join(core.lora.cfg.target_modules), core.lora.num_parameters())
        if use_emb:
            core.enable_embedding_training()
            logger.info("use_emb: the LLM's input embedding table [%d, %d] trains%s", geo.llm_vocab, geo.llm_dim,
                        " (tied: it is the lm_head too)" if geo.tied else " (the untied lm_head stays frozen)")
    if full_ft:
        core.enable_llm_training(None if llm_path.startswith("synthetic:") else sd)
        logger.info("freeze_llm=false: the decoder's %d tensors (%d parameters with the embedding table) train%s",
                    len(core.full_ft.offsets), core.full_ft.num_parameters() + geo.llm_vocab * geo.llm_dim,
                    " next to the projector" if not frozen_proj else "; the projector is frozen")
    model = slam_model_asr(core, tokenizer, setup_encoder_tokenizer(model_config, geo), train_config, model_config, **kwargs)
    ckpt_path = kwargs.get("ckpt_path", None)
    if ckpt_path is not None:
        logger.info("loading other parts from: %s", ckpt_path)
        model.load_state_dict(torch.load(ckpt_path, map_location="cpu"), strict=False)
    return model, tokenizer


def default_top_k(model_config):
    """generate(do_sample=True) without ``top_k``: the reference never passes one, so HF takes it from the model's generation config
    -- ``top_k`` of <llm_path>/generation_config.json when that file has one, otherwise GenerationConfig's default 50."""
    path = os.path.join(str(model_config.get("llm_path", "") or ""), "generation_config.json")
    if os.path.isfile(path):
        import json
        with open(path) as f:
            top_k = json.load(f).get("top_k")
        if top_k is not None:
            return top_k
    return 50


# ------------------------------------------------------------------------------------------------ the model
NO_GRAPH_MSG = ("ps_slm_amd: this loss was computed in eval mode (model.eval() / need_backward=False): the step kept no activations "
                "for a backward pass.  Call model.train() before the forward whose loss you want to differentiate")


class EngineLoss(torch.Tensor):
    """``outputs.loss`` of an EVAL-mode forward: the 0-dim fp32 device tensor the step's CE kernel wrote.  It behaves like any
    tensor (``loss / k``, ``.detach().float()``, ``.item()`` of Multitask/utils/deepspeed_utils.py:283-293), results of arithmetic on
    it stay ``EngineLoss``, and ``backward()`` raises: no activations were saved.  (The TRAINING-mode loss is an ordinary tensor
    with a grad_fn: ``_HipStep`` below.)"""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t.detach(), False)

    def backward(self, *args, **kwargs):
        raise RuntimeError(NO_GRAPH_MSG)


class _HipStep(torch.autograd.Function):
    """The autograd node behind ``outputs.loss``: forward = the loss the HIP step already computed; backward = the hand-scheduled HIP
    backward of that step (``TasuModel.run_backward``: dgrad through the frozen decoder, wgrad of the projector / the adapters into
    the flat fp32 bucket ``core.proj.g``), each leaf receiving ``grad_output x`` its slice of the bucket.  Nothing of the arithmetic
    runs in torch; the Function only shuttles pointers (SURVEY 8b "Autograd glue")."""

    @staticmethod
    def forward(ctx, loss_dev, model, st, *leaves):
        ctx.model, ctx.st = model, st
        return loss_dev.detach().clone()

    @staticmethod
    def backward(ctx, grad_out):
        model, st = ctx.model, ctx.st
        if model.last_state is not st:
            raise RuntimeError("ps_slm_amd: loss.backward() of an OLDER step -- the activations of a forward pass live in the model's "
                               "workspace until the next forward; differentiate each loss before running the next batch")
        if getattr(st, "backward_ran", False):
            raise RuntimeError("ps_slm_amd: this step's backward has already run (the workspace does not keep a graph for a second pass)")
        model.core.run_backward(st)
        st.backward_ran = True
        model._masters_touched = True                   # an optimizer is about to write the masters: refresh the bf16 copies next forward
        g = model.core.proj.g
        scale = grad_out.to(g.dtype)
        return (None, None, None) + tuple(v * scale for _, v in model._trainable_views(g))


class CausalLMOutput:
    __slots__ = ("loss", "logits")

    def __init__(self, loss, logits):
        self.loss, self.logits = loss, logits


class slam_model_asr:
    """Mirror of the reference's ``slam_model_asr`` (Multitask/model/ps-slm.py:183-537) over TasuModel."""

    def __init__(self, core: TasuModel, tokenizer, encoder_tokenizer, train_config, model_config, **kwargs):
        self.core = core
        self.tokenizer = tokenizer
        self.encoder_tokenizer = encoder_tokenizer
        self.train_config, self.model_config = train_config, model_config
        self.metric = kwargs.get("metric", "acc")
        self.ctc_posterior = train_config.get("ctc_posterior", True)
        self.do_psd = train_config.get("do_psd", True)
        self.voca_trans = train_config.get("voca_trans", False)
        self.gt_emb = train_config.get("gt_emb", False)
        self.gt_emb_noise = train_config.get("gt_emb_noise", False)
        if self.voca_trans or train_config.get("top1_emb", False):
            # FINDING: the reference's own voca_trans branch cannot run -- forward (ps-slm.py:485-514) and generate (:614-640) read
            # `encoder_outs`, which is only assigned in the voca_trans == False branch (:457-471, :590-603), and raise
            # UnboundLocalError (reproduced with the imported reference); top1_emb lives inside that branch.  There is nothing to
            # pin an implementation against.
            raise NotImplementedError("voca_trans / top1_emb: the reference's branch (Multitask/model/ps-slm.py:485-514) reads an "
                                      "unassigned `encoder_outs` and raises UnboundLocalError as shipped; not built")
        if not self.ctc_posterior:
            # the raw-feature branch (ps-slm.py:515-523) never looks at gt_emb: the encoder always runs
            self.gt_emb = False
        # knobs of ctc_pseudo_posterior_noise (ps-slm.py:372-375), overridable as attributes like in the reference
        self.drop_prob, self.insert_prob, self.smooth_low, self.smooth_high = 0.05, 0.0, 0.0, 0.1
        self.training = True
        self.last_state = None
        self._leaves = None                            # (key, [(name, leaf)]): named_parameters()
        self._masters_touched = False                  # a foreign optimizer may have written the masters since the last refresh

    def _refresh_if_touched(self):
        if self._masters_touched:
            self.core.sync_projector_copies()          # masters -> bf16 working copies + their transposes (TasuEngine.step() does this itself)
            self._masters_touched = False

    # ---- nn.Module-like surface
    def train(self, mode=True):
        self.training = mode
        self.core.training = bool(mode)                # LoRA dropout is active in training mode only
        return self

    def eval(self):
        return self.train(False)

    def to(self, *a, **k):
        return self

    def _views(self, flat):
        """(name, view of ``flat``, trainable) for every tensor ``named_parameters()`` lists: ``flat`` is the fp32 master buffer or the
        gradient bucket (same layout); K padding is sliced off where that is a plain column slice."""
        pr = self.core.proj
        for n in pr.names:
            v = pr.view(flat, n)
            r = pr.real[n]
            if v.dim() == 1:
                v = v[: r[0]]
            elif v.dim() == 2 and len(r) == 2 and not (n == pr.n_w1 and pr.kin > 1):
                v = v[:, : r[1]]
            yield "encoder_projector." + n, v, not self.core.freeze_projector
        if self.core.lora is not None:                 # use_peft=true: lora_A / lora_B of every adapted Linear, peft's key names
            for key, k in self.core.lora.names():
                yield key, self.core.lora.view(flat, *k), True
        if self.core.full_ft is not None:              # freeze_llm=false: every tensor of Qwen2ForCausalLM, the reference's module names
            for key, v in self.core.full_ft.named_views(flat):
                yield key, v, True
            yield FT_EMBED_KEY, self.core.embed_view(flat), True
        elif self.core.embed_base is not None:         # use_emb: the decoder's input embedding table [V, D]
            yield EMBED_KEY, self.core.embed_view(flat), True

    def _trainable_views(self, flat):
        return [(n, v) for n, v, t in self._views(flat) if t]

    def named_parameters(self):
        """The trainable tensors under the reference's names (``encoder_projector.*``; what
        ``filter(lambda p: p.requires_grad, model.parameters())`` of Multitask/finetune_deepspeed.py:129 keeps): leaf views
        of the flat fp32 master buffer, ``requires_grad=True``, the SAME objects on every call (an optimizer built over them
        updates the masters in place; ``loss.backward()`` fills their ``.grad`` from the gradient bucket: ``_HipStep``)."""
        pr = self.core.proj
        key = (pr.p.data_ptr(), pr.p.numel(), self.core.lora is not None, bool(self.core.freeze_projector), self.core.embed_base,
               self.core.full_ft is not None)
        if self._leaves is None or self._leaves[0] != key:
            flat = pr.p.detach()
            self._leaves = (key, [(n, v.requires_grad_(t)) for n, v, t in self._views(flat)])
        return iter(self._leaves[1])

    def parameters(self):
        return (p for _, p in self.named_parameters())

    def state_dict(self):
        """The trainable tensors (what the reference's checkpoint keeps: checkpoint_handler.py:169-182 saves with
        exclude_frozen_parameters): the projector and, with use_peft, the adapters and -- use_emb -- the LLM's embedding table."""
        proj = {} if self.core.freeze_projector else self.core.projector_state_dict()
        if self.core.full_ft is not None:              # freeze_llm=false: checkpoint_handler.py:214 saves the LLM, fp32 masters
            return {**proj, **self.core.full_ft.state_dict(), FT_EMBED_KEY: self.core.llm.embed.detach().clone()}
        emb = {} if self.core.embed_base is None else {EMBED_KEY: self.core.llm.embed.detach().clone()}
        return {**proj, **self.core.lora_state_dict(), **emb}

    def load_state_dict(self, sd, strict=False):
        missing = []
        for n in self.core.proj.names:
            k = "encoder_projector." + n
            if k in sd:
                self.core.proj.load(n, sd[k].to(self.core.device, torch.float32))
            else:
                missing.append(k)
        known = set()
        if self.core.lora is not None:
            for key, k in self.core.lora.names():
                known.add(key)
                if key in sd:
                    self.core.lora.load(*k, sd[key])
                else:
                    missing.append(key)
        # the embedding table of a use_emb checkpoint is a value of the decoder: it loads into a model built without use_emb too
        if EMBED_KEY in sd:
            known.add(EMBED_KEY)
            self.core.load_embed(sd[EMBED_KEY])
        elif self.core.embed_base is not None and self.core.full_ft is None:
            missing.append(EMBED_KEY)
        # a fully fine-tuned decoder (freeze_llm=false): its tensors are values of the decoder too -- into the masters of a model that
        # trains them, or in place of the frozen weights of one that does not (with tied embeddings a lm_head key is ignored)
        llm_keys = [k for k in sd if is_llm_key(k)]
        known.update(llm_keys)
        ft = self.core.full_ft
        if ft is not None:
            have = set(llm_keys)
            for key, _ in ft.named_views(self.core.proj.p):
                if key in have:
                    ft.load(key, sd[key])
                else:
                    missing.append(key)
            if FT_EMBED_KEY in have:
                self.core.load_embed(sd[FT_EMBED_KEY])
            else:
                missing.append(FT_EMBED_KEY)
        elif llm_keys:
            self.core.load_llm_tensors({k: sd[k] for k in llm_keys})
        if strict and missing:
            raise KeyError(f"missing keys {missing}")
        self.core.sync_projector_copies()
        return missing, [k for k in sd if not k.startswith("encoder_projector.") and k not in known]

    # ---- CPS noise draws: same calls in the same order on the global CPU RNG as ps-slm.py:380-399
    def draw_noise(self, ids_list):
        """insert_prob == 0 (the shipped recipe): per utterance one uniform alpha, then one rand(len) keep mask."""
        if self.insert_prob != 0.0:
            raise ValueError("insert_prob != 0: use draw_noise_rows (insertions change the row sequence)")
        alphas, keeps = [], []
        for ids in ids_list:
            alphas.append(torch.empty(()).uniform_(self.smooth_low, self.smooth_high).item())
            keeps.append((torch.rand(len(ids)) > self.drop_prob).numpy())
        return alphas, keeps

    def draw_noise_rows(self, ids_list, blank_id=0):
        """The full CPS noise of ps-slm.py:360-409 as row descriptions: per utterance the final sequence of (id, alpha) after
        smoothing, drops and -- ``insert_prob`` > 0 -- int(len * insert_prob) insertions, each at randint(0, len + 1), each with
        probability 1/2 a copy of the row before it (same id, same alpha) and otherwise an exact one-hot blank row (alpha 0).
        Same calls in the same order on the global CPU RNG as the reference.  Returns (ids per utterance, alphas per row)."""
        out_ids, out_alpha = [], []
        for ids in ids_list:
            alpha = torch.empty(()).uniform_(self.smooth_low, self.smooth_high).item()
            keep = (torch.rand(len(ids)) > self.drop_prob).numpy()
            rows = [(int(i), alpha) for i, k in zip(ids, keep) if k]
            for _ in range(int(len(rows) * self.insert_prob)):
                pos = torch.randint(0, len(rows) + 1, (1,)).item()
                if bool(torch.rand(1) < 0.5) and len(rows) > 0:
                    rows.insert(pos, rows[pos - 1] if pos > 0 else rows[0])
                else:
                    rows.insert(pos, (int(blank_id), 0.0))
            out_ids.append([r[0] for r in rows])
            out_alpha.append([r[1] for r in rows])
        return out_ids, out_alpha

    # ---- forward (ps-slm.py:411-537)
    def forward(self, input_ids=None, input_features=None, attention_mask=None, input_feature_length=None, GT=None,
                labels=None, **unused):
        core = self.core
        self._refresh_if_touched()
        # use_fp16 = false outside training: the reference's fp32 arithmetic (evaluation(), deepspeed_utils.py:394-498, or any
        # model(**batch) under no autocast) -- fp32 projector / encoder / decoder / logits / CE (ps_slm_amd/decode_fp32.py)
        fp32_eval = core.arith == "fp32" and not self.training
        fp32_train = core.arith_train == "fp32" and self.training and labels is not None   # the shipped recipe trains in fp32 too (train_fp32.py)
        if self.gt_emb:
            ids_list = [self.encoder_tokenizer.encode(t) for t in GT]
            alphas = keeps = row_alphas = None
            if self.gt_emb_noise and self.insert_prob != 0.0:
                ids_list, row_alphas = self.draw_noise_rows(ids_list, core.geo.blank_id)
            elif self.gt_emb_noise:
                alphas, keeps = self.draw_noise(ids_list)
            st = core.prepare_text(input_ids, attention_mask, labels, ids_list, alphas, keeps, row_alphas=row_alphas)
            if not (fp32_eval or fp32_train):
                core.run_forward_text(st, compute_loss=labels is not None, need_backward=self.training)
        else:
            if input_features is None:
                raise ValueError("the audio branch needs input_features: dataset_config.text_only=true is only valid with "
                                 "train_config.gt_emb=true (text pseudo-posterior instead of the encoder)")
            st = core.prepare_audio(input_ids, attention_mask, labels, input_features, input_feature_length,
                                    do_psd=self.do_psd, fp32=fp32_eval or fp32_train)
            if not (fp32_eval or fp32_train):
                core.run_forward_llm(st, compute_loss=labels is not None, need_backward=self.training)
        if fp32_train:
            from ps_slm_amd.train_fp32 import forward_train_fp32
            forward_train_fp32(core, st)
        elif fp32_eval:
            from ps_slm_amd.decode_fp32 import forward_fp32
            forward_fp32(core, st, compute_loss=labels is not None)
        self.last_state = st
        if labels is None:
            return CausalLMOutput(None, core.logits_view(st)), -1
        res = st.dev["loss_out"]
        if self.training:
            leaves = [p for _, p in self.named_parameters() if p.requires_grad]
            loss = _HipStep.apply(res[0], self, st, *leaves)
        else:
            loss = EngineLoss(res[0])
        return CausalLMOutput(loss, core.logits_view(st)), (res[1] if self.metric else -1)

    __call__ = forward

    def prefetch(self, input_features=None, input_feature_length=None, **unused) -> bool:
        """Optional, audio branch only: start the frozen encoder pass of the NEXT batch now, on a side stream under the current
        batch's decoder step (TasuModel.prefetch_encoder).  Takes the collator's batch dict like forward(); the forward() of that
        very batch then skips its own encoder pass.  Results do not change; a batch that was not announced (or the text branch,
        or the CPU double) runs as before and the call returns False."""
        if self.gt_emb or input_features is None:
            return False
        return self.core.prefetch_encoder(input_features, input_feature_length)

    @torch.no_grad()
    def generate(self, input_ids=None, input_features=None, attention_mask=None, input_feature_length=None,
                 targets=None, **kwargs):
        from ps_slm_amd.decode import beam_search_generate
        core = self.core
        self._refresh_if_touched()
        # the decode loop is HF beam search / greedy with do_sample=False (ps-slm.py:660-675 defaults) or, with do_sample=True, HF multinomial
        # sampling (num_beams=1) and beam-search multinomial sampling (num_beams > 1, the reference's default 4 included:
        # csrc/sample.hip); repetition_penalty is served on all of them (ps_slm_amd/decode.py, HF's processor).  A sampling knob HF would
        # silently ignore (no do_sample) is rejected
        from ps_slm_amd.decode import check_repetition_penalty, check_sampling
        repetition_penalty = check_repetition_penalty(kwargs.get("repetition_penalty", 1.0))
        num_beams = kwargs.get("num_beams", 4)
        sampling = None
        if kwargs.get("do_sample", False) is True:
            sampling = check_sampling(kwargs.get("temperature", 1.0), kwargs.get("top_k", default_top_k(self.model_config)),
                                      kwargs.get("top_p", 1.0))
        else:
            for name, default in (("do_sample", False), ("top_p", 1.0), ("temperature", 1.0), ("top_k", None)):
                if kwargs.get(name, default) != default:
                    raise NotImplementedError(f"generate({name}={kwargs[name]!r}, num_beams={num_beams!r}): the MI355X decode loop serves "
                                              "the sampling knobs with do_sample=True only (Multitask/model/ps-slm.py:660-675); "
                                              f"{name} without do_sample=True would silently be ignored")
        if self.gt_emb:                                     # ps-slm.py:590-598
            texts = [re.sub(r"[^A-Za-z\s.,!?]+", "", t).lower().strip() for t in targets]
            ids_list = [self.encoder_tokenizer.encode(t) for t in texts]
            st = core.prepare_text(input_ids, attention_mask, None, ids_list, None, None)
            if core.arith != "fp32":                       # (the fp32 path runs its own fp32 projector)
                core.forward_projector_text(st)
        else:
            st = core.prepare_audio(input_ids, attention_mask, None, input_features, input_feature_length,
                                    do_psd=self.do_psd)
        if core.arith == "fp32":                           # use_fp16 = false: the reference's own decode arithmetic
            from ps_slm_amd.decode_fp32 import beam_search_generate_fp32 as beam_search_generate
        return beam_search_generate(core, st, num_beams=num_beams, sampling=sampling,
                                    max_new_tokens=kwargs.get("max_new_tokens", 200),
                                    min_length=kwargs.get("min_length", 1),
                                    length_penalty=kwargs.get("length_penalty", 1.0),
                                    repetition_penalty=repetition_penalty,
                                    eos_token_id=self.tokenizer.eos_token_id, pad_token_id=self.tokenizer.pad_token_id)
