"""The launch sequence of the bf16 training step, pinned (tools/make_golden_step_trace.py -> tests/golden/step_trace.txt): for every
recipe the operator calls of one step on the CPU double -- the same operators in the same order, the same scalars, and behind every
tensor argument the same buffer at the same offset, shape and stride -- equal the stored trace line for line.  The step is replayed
as a hipGraph on buffers the layers alias on purpose; a launch that moves, or reads another buffer, is a change of behaviour even
where every tolerance test still passes.  A change that moves one on purpose refreshes the file with the tool and shows the diff."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_golden_step_trace as T  # noqa: E402


def sections(lines):
    out = {}
    for line in lines:
        if line.startswith("== "):
            cur = out.setdefault(" ".join(line.split()[1:3]), [])           # recipe and batch
        else:
            cur.append(line)
    return out


def test_step_traces_equal_the_golden_line_for_line():
    want, got = sections(T.read_golden()), sections(T.generate())
    assert list(got) == list(want)
    for head in want:
        for n, (g, w) in enumerate(zip(got[head] + ["(end)"], want[head] + ["(end)"])):
            assert g == w, f"{head}, call {n}:\n  now    {g}\n  golden {w}"
        assert len(got[head]) == len(want[head])


def test_the_golden_covers_the_recipes_and_both_batches():
    heads = [h.split() for h in sections(T.read_golden())]
    assert {h[0] for h in heads} == set(T.recipes()) and len(heads) == 2 * len(T.recipes())
    assert {int(h[1][1:]) % 64 == 0 for h in heads} == {True, False}
    size = lambda n: os.path.getsize(os.path.join(os.path.dirname(T.GOLDEN), n))
    assert size("step_trace.txt") < size("gemm_plan_grid.txt")
