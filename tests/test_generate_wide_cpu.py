"""generate(num_beams = 5 .. 16) on the CPU: the fixture tests/golden/mid_generate_wide.npz (tools/make_golden_generate_wide.py), the
restatement tests/penalty_ref.py against the REAL reference's tokens on it, the argument check, the product's decode loop on the CPU
double, and the double's beam update against BeamState on the scripted streams the GPU test drives the kernel through."""
import dataclasses

import pytest

from conftest import load_npz

from penalty_ops import PenaltyFakeOps
from penalty_ref import generate_penalised, prompt_embeddings, same
from ps_slm_amd.decode import BEAM_MAX_NB, BeamState, beam_search_generate, generate_args
from ps_slm_amd.model import TasuModel
from wide_cases import EOS, KINDS, Script, check_against_beam_state, drive, wide_cases


@pytest.fixture(scope="module")
def fixture():
    geo, sd, cases = wide_cases()
    double = TasuModel(geo, PenaltyFakeOps(), "cpu")
    double.load_reference_state_dict(sd)
    return geo, sd, cases, double


def decode(double, geo, c, **over):
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    double.forward_projector_text(st)
    return beam_search_generate(double, st, eos_token_id=geo.eos_id, pad_token_id=geo.eos_id, **dict(c["kw"], **over)).numpy()


def test_fixture_covers_what_it_claims(fixture):
    _, _, cases, _ = fixture
    kws = [c["kw"] for c in cases]
    assert len(cases) >= 24 and {k["num_beams"] for k in kws} == {5, 6, 7, 8, 10, 12, 16}
    assert all(k["repetition_penalty"] == 1.0 for k in kws if k["num_beams"] == 5)        # the unpenalised top-k at k = 10
    assert {k["repetition_penalty"] for k in kws} == {1.0, 1.3, 0.8} and {k["length_penalty"] for k in kws} == {0.6, 1.0, 2.0}
    assert sum(k["min_length"] >= c["ids"].shape[1] + 5 for k, c in zip(kws, cases)) >= 4     # an active EOS ban (embedded prompt + 5)
    assert {c["ids"].shape[0] for c in cases} == {1, 2, 3} and all(8 <= k["max_new_tokens"] <= 40 for k in kws)
    assert {k["max_new_tokens"] for k in kws} >= {8, 40}
    assert 2 * sum(c["differs"] for c in cases) >= len(cases)
    stable = [c["kw"] for c in cases if c["bf16_stable"]]
    assert len(stable) >= 10 and {8, 16} <= {k["num_beams"] for k in stable} and any(k["repetition_penalty"] != 1.0 for k in stable)
    z = load_npz("mid_generate_wide")
    flagged = set(z["near_tie_on_double"].tolist()) | set(z["exact_tie_cases"].tolist())
    assert len(flagged) <= 2 and not any(cases[n]["bf16_stable"] for n in flagged)           # explained near-ties, kept in the file


def test_restatement_in_fp32_reproduces_the_reference_on_every_case(fixture):
    geo, sd, cases, _ = fixture
    gd = dataclasses.asdict(geo)
    bad = []
    for n, c in enumerate(cases):
        emb, mask = prompt_embeddings(sd, geo, c["ids"], c["am"], c["post_ids"], "fp32")
        t = generate_penalised(sd, emb, mask, gd, mode="fp32", **c["kw"])
        if not same(t, c["tokens"]):
            bad.append((n, t.tolist(), c["tokens"].tolist()))
    assert not bad, bad


def test_generate_args_accepts_16_beams_and_refuses_17(fixture):
    geo, _, cases, double = fixture
    c = cases[0]
    st = double.prepare_text(c["ids"], c["am"], None, c["post_ids"], None, None)
    assert BEAM_MAX_NB == 16
    for nb in (1, 5, 6, 16):
        assert generate_args(double, st, nb, 8, 1, None, None, 2048, "the cache attention's") == (0, geo.eos_id, geo.eos_id)
    for nb in (0, 17, 32):
        with pytest.raises(ValueError, match=rf"num_beams={nb}: the device beam search serves 1\.\.16 beams"):
            generate_args(double, st, nb, 8, 1, None, None, 2048, "the cache attention's")


def test_product_decode_loop_on_the_double_reproduces_the_stable_cases(fixture):
    """generate(num_beams = 5 .. 16) through the CPU double returns the reference's tokens on every bf16-stable case, 8 and 16 beams
    and a penalised one among them (on the parent: ValueError, 1..5 beams)."""
    geo, _, cases, double = fixture
    stable = [(n, c) for n, c in enumerate(cases) if c["bf16_stable"]]
    assert {8, 16} <= {c["kw"]["num_beams"] for _, c in stable}
    bad = [(n, c["kw"]) for n, c in stable if not same(decode(double, geo, c), c["tokens"])]
    assert not bad, bad


def test_wide_decode_differs_from_four_beams_where_the_reference_does(fixture):
    geo, _, cases, double = fixture
    n, c = next((n, c) for n, c in enumerate(cases) if c["bf16_stable"] and c["differs"] and c["kw"]["num_beams"] == 8)
    assert not same(decode(double, geo, c, num_beams=4), c["tokens"]), n


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("nb,B", [(6, 3), (16, 1), (8, 17), (4, 3)])
def test_double_beam_update_follows_beam_state_on_the_scripted_streams(kind, nb, B):
    """The streams of tests/test_gpu_generate_wide.py on the CPU double: after every step every state array equals BeamState's; the
    scripts do what their names say."""
    T, steps = 20, 22
    snaps, bs = drive(PenaltyFakeOps(), "cpu", Script(kind, B, nb, seed=nb), T, KINDS[kind], 2, steps)
    state = BeamState(B, nb, T, EOS, EOS, KINDS[kind], 2)
    n_steps = check_against_beam_state(snaps, state, Script(kind, B, nb, seed=nb), steps)
    assert same(bs.result(EOS).numpy(), state.result())
    if kind == "sparse":
        assert n_steps == T                                                   # max_new reached
    if kind == "allstop":
        assert n_steps == (12 if B == 1 else 14)                              # utterance 0 alone stops at step 11: the batch goes on
    if kind == "heavy":
        assert not state.unsat.any() and state.is_fin.all()                   # full heaps; the utterances stopped improving one by one
