"""TEST INFRASTRUCTURE ONLY -- tests/golden/qformer_finding.json: what the REAL reference (imported: oracle/ref_import.py) does
when its slam_model_asr is given an EncoderProjectorQFormer (encoder_projector="q-former") at the mid geometry: whether the
projector carries the `.k` every call site reads (Multitask/model/ps-slm.py:482), and the exception type and message of a forward
call with cross_attn off and on.  tests/test_oracle_golden.py::test_reference_cannot_run_its_q_former reads it.  Run in the build
container only."""
import contextlib
import dataclasses
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import Cfg, build_reference_model, load_reference  # noqa: E402
from ps_slm_amd.model import Geometry  # noqa: E402
from ps_slm_amd.synthetic import MID_GEOMETRY, synthetic_text_batch  # noqa: E402


def outcome(fn):
    try:
        fn()
    except Exception as e:                              # the finding IS the exception
        return {"raised": True, "type": type(e).__name__, "message": str(e)[:300]}
    return {"raised": False, "type": None, "message": None}


if __name__ == "__main__":
    _, _, proj = load_reference()
    geo = Geometry.from_dict(MID_GEOMETRY)
    model = build_reference_model(dataclasses.asdict(geo), 0, dict(gt_emb=True, gt_emb_noise=False))
    model.encoder_projector = proj.EncoderProjectorQFormer(Cfg(encoder_projector="q-former", encoder_dim=geo.ctc_vocab, llm_dim=geo.llm_dim,
                                                               qformer_layers=1, query_len=8))
    batch = synthetic_text_batch(geo, 2, seed=1, prompt_len=9, n_audio=21, target_len=17, speech_pos=4, feat_frames=12, noise=False)
    call = dict(input_ids=batch["input_ids"], input_features=batch["input_features"], attention_mask=batch["attention_mask"],
                input_feature_length=batch["input_feature_length"], GT=[" ".join(map(str, p)) for p in batch["post_ids"]],
                labels=batch["labels"])
    rec = {"has_k": hasattr(model.encoder_projector, "k")}
    with contextlib.redirect_stdout(io.StringIO()):
        for flag in (False, True):
            model.cross_attn = flag
            rec[f"cross_attn_{str(flag).lower()}"] = outcome(lambda: model(**call))
    with open(os.path.join(ROOT, "tests", "golden", "qformer_finding.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
