"""The launch sequence of the fp32 training step, pinned (tools/make_golden_f32_step_trace.py -> tests/golden/f32_step_trace.txt): for
every recipe the operator calls of forward_train_fp32 + run_backward on the CPU double tests/f32_step_ops.py -- the same operators
in the same order, the same scalars, and behind every tensor argument the same buffer at the same offset, shape and stride -- equal
the stored trace line for line.  The fp32 step's sums are order-dependent by design, so a launch that moves changes the bits of the
loss and the gradients even where every tolerance test still passes.  And the double itself is held to the oracle's fp32 step at the
project's fp32 bars, so that what is traced is the step and not something that merely runs."""
import dataclasses
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_golden_f32_step_trace as T  # noqa: E402
from test_step_trace_cpu import sections  # noqa: E402


def test_fp32_step_traces_equal_the_golden_line_for_line():
    want, got = sections(T.read_golden(T.GOLDEN)), sections(T.generate())
    assert list(got) == list(want)
    for head in want:
        for n, (g, w) in enumerate(zip(got[head] + ["(end)"], want[head] + ["(end)"])):
            assert g == w, f"{head}, call {n}:\n  now    {g}\n  golden {w}"
        assert len(got[head]) == len(want[head])


def test_the_golden_covers_the_recipes_and_both_batches():
    heads = [h.split() for h in sections(T.read_golden(T.GOLDEN))]
    assert {h[0] for h in heads} == set(T.recipes()) and len(heads) == 2 * len(T.recipes())
    assert {int(h[1][1:]) % 64 == 0 for h in heads} == {True, False}
    size = lambda n: os.path.getsize(os.path.join(os.path.dirname(T.GOLDEN), n))
    assert size("f32_step_trace.txt") < size("step_trace.txt")


def test_the_double_has_the_step_operators_and_fakeops_has_none():
    from fake_ops import FakeOps
    from ps_slm_amd.model import f32_qk_norm_missing, qk_norm_wgrad_missing
    assert not [n for n in dir(FakeOps) if n.startswith("f32_")]
    ops = T.F32StepOps()
    assert f32_qk_norm_missing(ops) == () and not qk_norm_wgrad_missing(ops, "fp32")
    assert all(hasattr(ops, n) for n in ("f32_gemm_tn", "f32_rmsnorm_wgrad", "f32_colsum_split", "embed_bwd"))


@pytest.mark.parametrize("projector", ["linear-silu", "linear", "cov1d-linear"])
def test_the_double_runs_the_fp32_step_at_the_fp32_bars(projector):
    """M138 batch, mid geometry: |loss - oracle fp32 loss| <= 2e-5 and every projector gradient within 2e-4 relative L2 of the
    oracle's fp32 autograd (the bars of tests/test_gpu_model.py's fp32 step)."""
    import oracle.tasu_oracle as O
    geo = T.geometry(projector)
    m, sd = T.build(geo)
    batch = T.text_batch(geo, dict(T.BATCHES)["M138"])
    st, _ = T.step(m, batch, record=False)
    out, grads = O.loss_and_projector_grads(sd, batch, dataclasses.asdict(geo), "fp32")
    dloss = abs(float(st.dev["loss_out"][0]) - float(out["loss"].detach()))
    print(f"{projector}: |dloss| {dloss:.3e}")
    assert dloss <= 2e-5
    got = m.projector_grads()
    assert grads and set(grads) <= set(got)
    for k, g in grads.items():
        err = float((got[k].double() - g.double()).norm() / g.double().norm())
        print(f"{projector}: {k} relative L2 {err:.3e}")
        assert err <= 2e-4, (k, err)
