"""HIP graph capture with the cyclic garbage collector held off.

A collection that runs while a stream is capturing can free an unrelated, unreachable object
that owns a captured graph (an old agent's FusedPPO, a finished rollout): its destructor then
destroys a graph executable mid-capture, which the runtime refuses ("operation not permitted
when stream is capturing") and torch turns into an abort.  torch.cuda.graph no longer collects
before capturing (torch.compiler.config.force_cudagraph_gc is off by default), so this collects
first -- dead graphs are destroyed while nothing captures -- and holds the collector off for the
capture itself.  Captures happen once per argument key, so the collection's cost is off the
replayed path.
"""

from __future__ import annotations

import contextlib
import gc

import torch


@contextlib.contextmanager
def capture(graph: torch.cuda.CUDAGraph, stream=None, collect: bool = True, **kw):
    """torch.cuda.graph(graph, stream=stream, **kw), after a collection (collect=False: the
    caller has just collected, e.g. before a run of back-to-back captures) and with gc disabled
    inside."""
    if collect:
        gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=stream, **kw):
            yield graph
    finally:
        if was:
            gc.enable()


def run_or_replay(owner, use_graphs, key, steps, graph, gkey, seen, what):
    """The issue policy for a launch sequence `steps` (a rollout, ppo/rollout.py and
    ppo/group.py): replay the captured graph when its key repeats, run eagerly the first time a
    key is seen (allocations, argument tables), capture it the second time.  Counts what it did
    in owner.stats[f"{what}_replay" | "_eager" | "_capture"].  Returns the new (graph, graph
    key, seen key)."""
    if not use_graphs:
        steps()
        return graph, gkey, seen
    if graph is not None and key == gkey:
        owner.stats[f"{what}_replay"] += 1
        graph.replay()
        return graph, gkey, seen
    if key != seen:
        owner.stats[f"{what}_eager"] += 1
        steps()
        return graph, gkey, key
    owner.stats[f"{what}_capture"] += 1
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with capture(g, stream=s):
            steps()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    return g, key, seen


def run_or_replay_chunks(owner, use_graphs, key, chunks, steps, state):
    """run_or_replay per (t0, t1) chunk of a rollout, `steps(t0, t1)` issuing one chunk; state =
    one (graph, graph key, seen key) per chunk, or None."""
    if state is None or len(state) != len(chunks):
        state = [(None, None, None)] * len(chunks)
    return [run_or_replay(owner, use_graphs, key, lambda t0=t0, t1=t1: steps(t0, t1), *st,
                          "rollout")
            for (t0, t1), st in zip(chunks, state)]
