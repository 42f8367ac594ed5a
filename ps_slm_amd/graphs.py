"""hipGraph capture and replay of launch sequences whose kernel arguments depend only on a key (shapes, scalars, switches) and on
the addresses of persistent workspace buffers: the training step's forward / backward and the encoder region (TasuModel._graphed),
and the decode step (ps_slm_amd/decode.py)."""
import collections
import gc
import traceback

import torch


class GraphCache:
    """Captured graphs by key, at most ``capacity`` of them (the least recently used goes first).  The first call of a key runs
    ``fn`` eagerly (it allocates the workspace and sets lazy kernel attributes), the second is captured and replayed once, later
    calls replay.  A graph is only valid for the buffers it was captured on: every graph keeps the workspace generation it was
    captured at."""

    def __init__(self, capacity):
        self.capacity = capacity
        self._graphs = collections.OrderedDict()     # key -> (graph, views its capture published into ``dev``, generation)
        self._seen = {}                              # key -> calls that found no graph to replay (the warm-up count)

    def __len__(self):
        return len(self._graphs)

    def __iter__(self):
        return iter(self._graphs)

    def __contains__(self, key):
        return key in self._graphs

    def clear(self):
        self._graphs.clear()
        self._seen.clear()

    def drop(self, pred):
        """Forgets the graphs whose key satisfies ``pred``, and their warm-up counts."""
        for key in [k for k in self._graphs if pred(k)]:
            del self._graphs[key]
            self._seen.pop(key, None)

    def run(self, key, fn, generation, dev=None):
        """Runs the launch sequence ``fn`` for ``key``.  ``generation()``: the caller's workspace generation (bumped whenever a
        named buffer is re-allocated: the same generation means the same addresses).  ``dev``: the dict ``fn`` publishes views into
        (StepState.dev); a replay publishes again the ones its capture added."""
        dev = {} if dev is None else dev
        gen = generation()
        entry = self._graphs.get(key)
        if entry is not None and entry[2] != gen:
            # a workspace buffer has grown since the capture (a larger batch shape came by): the graph holds freed addresses.
            # Drop every graph of another generation and start over for this key.
            for k in [k for k, e in self._graphs.items() if e[2] != gen]:
                del self._graphs[k]
            self._seen.pop(key, None)
            entry = None
        if entry is not None:
            self._graphs.move_to_end(key)
            entry[0].replay()
            for k, v in entry[1].items():
                dev.setdefault(k, v)
            return
        seen = self._seen.get(key, 0)
        self._seen[key] = seen + 1
        if seen < 1:
            fn()                                     # eager warm-up: buffer allocation, lazy kernel attributes
            return
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        before = set(dev)
        # The cyclic garbage collector must not run inside a capture: an unreachable CUDAGraph of an earlier model (a cycle freed
        # at a moment of the collector's choosing) would be destroyed while this stream is capturing -- hipGraphDestroy then fails
        # with "operation not permitted when stream is capturing" inside a destructor and takes the process down (seen in bench.py
        # between two legs).  torch.cuda.graph collects once before the capture begins; nothing may be collected until it ends.
        gc_was = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):   # other threads (RCCL watchdog) may call into HIP
                try:
                    fn()
                except BaseException:
                    # an exception that unwinds out of a capture takes the process down in ~CUDAGraph: say what it was first
                    traceback.print_exc()
                    raise
        finally:
            if gc_was:
                gc.enable()
        if generation() != gen:
            # a buffer grew DURING the capture: launches recorded before the growth hold its freed address, so the graph is not
            # kept.  They were only recorded, not run: this call's work runs eagerly instead, on the buffers as they are now.
            fn()
            return
        self._graphs[key] = (graph, {k: v for k, v in dev.items() if k not in before}, gen)
        while len(self._graphs) > self.capacity:
            old, _ = self._graphs.popitem(last=False)
            self._seen.pop(old, None)
        graph.replay()
