"""HIP-graph replay of one U-Net evaluation (opt-in: PBE_GRAPH=1 or ``sampler.use_graph = True``).

One U-Net call is ~300 kernel launches.  The samplers call the network 51 times with identical shapes, the same context
tensor and only (x, t) changing, so the launch sequence can be captured ONCE per sampling run into a HIP graph
(``torch.cuda.CUDAGraph``: hipStreamBeginCapture on torch's capture stream - every libpbe_hip.so entry point takes the
stream, allocates nothing and never synchronises, so the C-ABI is capturable as it stands) and replayed with the inputs
copied into static buffers.  Results are bit-identical to eager launches (same kernels, same order;
``test_hip_graph_replay_is_bit_identical``).

Measured on MI355X (bench.py --batch 1, U-Net batch 2, ~16 us average kernel): 3.28 images/s replayed vs 3.36 eager.  The
host keeps ahead of the GPU even at batch 1 (~10 us of Python + ctypes per launch against >= 12 us of GPU time per
kernel including dispatch), so the small-batch regime is bound by per-kernel GPU fixed costs, not by the launch path,
and the capture pass costs one extra forward per run.  Hence off by default.
"""
from __future__ import annotations

import os

import torch


def graphs_enabled(unet_batch: int) -> bool:
    """PBE_GRAPH=1 enables replay for every batch size; default off (see the module docstring for the measurement)."""
    return os.environ.get("PBE_GRAPH", "0") == "1"


class GraphedUNet:
    def __init__(self, unet):
        self.unet = unet
        self.key = None
        self.graph = None
        self.replays = 0

    def __call__(self, x9: torch.Tensor, t: torch.Tensor, cond, paired: bool) -> torch.Tensor:
        """Same contract as ``unet.forward_nhwc(x9, t, cond.context, paired=paired, **cond.kwargs())`` for cond, an
        attention.Conditioning.  The graph is captured again when the shapes, ``paired`` or the conditioning (Conditioning.key)
        change.  The returned tensor is a static buffer that the next call overwrites (the samplers consume it before calling
        again).  With a collector (cond.maps) the captured launches add to its accumulators, which the eager pass put in place;
        every replay accumulates exactly as an eager call does, and tells the collector the launch counts the capture recorded."""
        key = (tuple(x9.shape), tuple(t.shape), bool(paired), cond.key())
        maps = cond.maps                               # (the collector itself: its accumulators are baked in)
        if key != self.key:
            self.sx, self.st, self.cond = x9.clone(), t.clone(), cond      # (cond: keeps the keyed tensors alive)
            kw = cond.kwargs()
            out = self.unet.forward_nhwc(self.sx, self.st, cond.context, paired=paired, **kw)     # eager: builds packs / caches / function attributes
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            if maps is not None:
                maps.begin_tape()                      # captured launches run at replay: counted there
            try:
                with torch.cuda.graph(g):
                    self.out = self.unet.forward_nhwc(self.sx, self.st, cond.context, paired=paired, **kw)
            finally:
                self.tape = maps.end_tape() if maps is not None else None
            self.graph, self.key = g, key
            return out
        self.sx.copy_(x9)
        self.st.copy_(t)
        self.graph.replay()
        if maps is not None:
            maps.replayed(self.tape)
        self.replays += 1
        return self.out
