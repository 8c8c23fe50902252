"""HIP-graph capture for the agents: the one place that opens a capture (AgentPPO through ppo_update.py, AgentOffPolicy._run_update,
AgentTD3._capture_updates)."""
import torch

from .. import native


def capture_guard():
    """Every HIP-graph capture of the agents runs inside native.capture_guard: no cyclic garbage collection while the capture is
    open, and the library parks -- instead of hipFree-ing -- any device memory a handle releases meanwhile (a hipFree under stream
    capture aborts the process: seen once in tests/test_gpu_td3.py, "Garbage-collecting" in the fatal error's stack, when a cyclic
    collection finalised an earlier env handle inside torch.cuda.graph).  The guard also covers refcount-driven finalisation,
    which disabling the collector alone does not."""
    return native.capture_guard()


def capture(device, *thunks):
    """The launches of `thunks`, in order, on the current stream as one graph.  A refused capture raises RuntimeError."""
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    # thread_local: the RCCL watchdog thread of a data-parallel run may touch the HIP API meanwhile
    with capture_guard(), torch.cuda.graph(g, capture_error_mode="thread_local"):
        for thunk in thunks:
            thunk()
    return g


def collective_in_graph(agent):
    """Data parallel: are the all-reduces captured inside the graph?  (RCCL: yes; gloo, or a capture some rank refused: no.)"""
    return agent.dp is not None and agent.use_graph_collective and getattr(agent.dp, "graph_capturable", False)


def capture_on_every_rank(dp, device, *thunks):
    """capture() that does not raise: (graph, None), or (None, the RuntimeError) after a synchronise.  Under data parallelism (`dp`
    not None) the ranks must use the SAME launch form from here on (a rank replaying the collective from its graph while another
    issues it eagerly would still match up, but a rank-local failure must not go unnoticed): one MAX over the ranks decides for all
    of them, so the graph is also None -- with no error of this rank's own -- where another rank refused."""
    g = refused = None
    try:
        g = capture(device, *thunks)
    except RuntimeError as exc:
        refused = exc
    if dp is not None and dp.max_over_ranks(1.0 if refused is not None else 0.0) > 0.5:
        g = None
    if g is None:
        torch.cuda.synchronize(device)
    return g, refused
