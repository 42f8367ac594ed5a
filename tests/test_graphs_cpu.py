"""ps_slm_amd.graphs.GraphCache (the capture / replay rule of the training step, the encoder region and the decode step) on a
stand-in for torch.cuda's graph API: a capture records the work ``fn`` issues without running it, a replay runs the recorded work
once."""
import collections
import contextlib
from types import SimpleNamespace

import pytest

from ps_slm_amd import graphs
from ps_slm_amd.graphs import GraphCache


class FakeCuda:
    def __init__(self):
        self.capturing = None                        # the graph being captured
        self.captures = self.replays = 0
        self.calls = collections.Counter()           # work -> Python calls of its fn
        self.runs = collections.Counter()            # work -> executions (eager calls and replays)
        fake = self

        class Graph:
            def __init__(self):
                self.work = []

            def replay(self):
                fake.replays += 1
                fake.runs.update(self.work)

        @contextlib.contextmanager
        def capture(graph, capture_error_mode=None):
            assert capture_error_mode == "thread_local" and fake.capturing is None
            fake.capturing = graph
            try:
                yield
            finally:
                fake.capturing = None
            fake.captures += 1

        self.torch = SimpleNamespace(cuda=SimpleNamespace(CUDAGraph=Graph, graph=capture, synchronize=lambda: None))

    def work(self, name, dev=None, on_capture=None):
        """fn of a launch sequence called ``name``; publishes ``dev[name]`` like forward_llm publishes its views."""
        def fn():
            self.calls[name] += 1
            if dev is not None:
                dev[name] = "view of " + name
            if self.capturing is None:
                self.runs[name] += 1
                return
            self.capturing.work.append(name)
            if on_capture is not None:
                on_capture()
        return fn


@pytest.fixture
def fake(monkeypatch):
    f = FakeCuda()
    monkeypatch.setattr(graphs, "torch", f.torch)
    return f


def test_eager_then_capture_then_replays(fake):
    cache, gen = GraphCache(4), lambda: 0
    fn = fake.work("a")
    for _ in range(4):
        cache.run("a", fn, gen)
    assert fake.calls["a"] == 2 and fake.runs["a"] == 4          # eager, captured + replayed once, replayed, replayed
    assert fake.captures == 1 and fake.replays == 3
    assert len(cache) == 1 and "a" in cache and list(cache) == ["a"]


def test_lru_eviction_drops_the_warm_up_count(fake):
    cache, gen = GraphCache(2), lambda: 0
    for key in "abc":
        cache.run(key, fake.work(key), gen)
        cache.run(key, fake.work(key), gen)
    assert list(cache) == ["b", "c"] and fake.captures == 3       # "a" went when "c" came
    cache.run("b", fake.work("b"), gen)                          # replay: "b" is now the most recently used
    cache.run("a", fake.work("a"), gen)
    assert fake.calls["a"] == 3 and fake.captures == 3 and "a" not in cache    # eager again: its warm-up count went with it
    cache.run("a", fake.work("a"), gen)
    assert list(cache) == ["b", "a"] and fake.runs == {"a": 4, "b": 3, "c": 2}


def test_generation_change_restarts_the_stale_key_only(fake):
    now = [0]
    cache, gen = GraphCache(8), lambda: now[0]
    for key in ("a", "a", "b", "c", "c"):                        # a, c captured; b warmed up
        cache.run(key, fake.work(key), gen)
    assert list(cache) == ["a", "c"] and fake.captures == 2
    now[0] = 1                                                   # a workspace buffer moved
    cache.run("a", fake.work("a"), gen)
    assert len(cache) == 0 and fake.calls["a"] == 3 and fake.runs["a"] == 3 and fake.captures == 2    # stale hit: eager
    cache.run("a", fake.work("a"), gen)
    assert list(cache) == ["a"] and fake.captures == 3 and fake.runs["a"] == 4
    cache.run("b", fake.work("b"), gen)                          # the other keys' warm-up counts survive: captured at once
    cache.run("c", fake.work("c"), gen)
    assert list(cache) == ["a", "b", "c"] and fake.captures == 5 and fake.runs == {"a": 4, "b": 2, "c": 3}


def test_growth_during_capture_keeps_no_graph_and_runs_the_work_once(fake):
    now, grow = [0], [True]

    def grows():
        if grow[0]:
            now[0], grow[0] = now[0] + 1, False
    cache, gen = GraphCache(8), lambda: now[0]
    fn = fake.work("a", on_capture=grows)
    cache.run("a", fn, gen)
    cache.run("a", fn, gen)                                      # captured while a buffer grew
    assert fake.captures == 1 and len(cache) == 0 and fake.runs["a"] == 2
    cache.run("a", fn, gen)                                      # captured again, now kept
    cache.run("a", fn, gen)
    assert fake.captures == 2 and list(cache) == ["a"] and fake.runs["a"] == 4


def test_clear_and_drop_reset_the_warm_up_counts(fake):
    cache, gen = GraphCache(8), lambda: 0
    for key in (("region", 1), ("region", 1), ("fwd", 1), ("fwd", 1), ("bwd", 1)):
        cache.run(key, fake.work(key), gen)
    cache.drop(lambda k: k[0] == "region")
    assert list(cache) == [("fwd", 1)]
    cache.run(("region", 1), fake.work(("region", 1)), gen)
    assert ("region", 1) not in cache and fake.calls[("region", 1)] == 3      # eager again
    cache.clear()
    assert len(cache) == 0
    for key in (("fwd", 1), ("bwd", 1)):
        cache.run(key, fake.work(key), gen)
    assert len(cache) == 0 and fake.captures == 2 and fake.calls == {("region", 1): 3, ("fwd", 1): 3, ("bwd", 1): 2}


def test_replay_publishes_the_captured_views(fake):
    cache, gen = GraphCache(8), lambda: 0
    devs = [{}, {"kept": 1}, {}, {"a": "mine"}]
    for dev in devs:
        cache.run("a", fake.work("a", dev=dev), gen, dev)
    assert fake.calls["a"] == 2 and fake.replays == 3
    assert devs[2] == {"a": "view of a"}                         # published by the replay
    assert devs[3] == {"a": "mine"}                              # (setdefault: what the caller put there stays)
    cache.run("a", fake.work("a"), gen)                          # a caller without views
    assert fake.replays == 4
