"""Noise as a function of per-sample seeds: the stream plan over ops.randn_seeded (csrc/noise.hip).

THE FUNCTION.  Element e of sample b's flat fp32 array is Box-Muller on Philox4x32-10 (Salmon et al., SC'11; the Random123 constants):

    key     = (seed lo32, seed hi32)                         seeds[b] as an unsigned 64-bit value
    counter = (e // 4, sub[b], stream lo32, stream hi32)     one call gives x0 .. x3, elements 4q .. 4q + 3 come from it
    u = ((x0 >> 8) + 1) * 2^-24 in (0, 1],  v = (x1 >> 8) * 2^-24 in [0, 1),  r = sqrt(-2 ln u)
    elements 4q, 4q + 1 = r cos(2 pi v), r sin(2 pi v);  4q + 2, 4q + 3 the same from (x2, x3)

A value depends on (seed, sub, stream, e) and on nothing else: not on the batch size, the sample's place in the batch, how many holes
or chunks share a call, the device, or torch's generators.  There is no generator state to advance.

THE STREAM PLAN (part of the public contract: changing it changes every seeded picture).  `stream` names what a draw is for:

    STREAM_X_T      = 0         the start latent x_T of a sampler run, shape [B, 4, h, w]
    STREAM_POST_EPS = 1         the noise of the autoencoder's posterior sample of the masked picture, shape [B, 4, h, w]
    2 .. 15                     reserved
    STREAM_STEP0 + i, i >= 0    the i-th draw a sampler makes after x_T, in the order the sampler asks: the q_sample noise of the
                                mask / x0 blend (one per step, before the U-Net call) and the sigma_t noise of a DDIM step with eta > 0
                                (one per step, after the update).  A run with both alternates blend, step, blend, step ...

`sub` is a second, 31-bit name inside a seed.  pipeline.inpaint_holes with one seed per PICTURE gives each hole the picture's seed and
sub = the hole's first pixel index in raster order + 1 (the smallest label of its group, csrc/holes.hip), so a hole's noise is a function
of (picture seed, where the hole starts) and not of the other holes; everything else uses sub = 0.

One SeededNoise serves one sampler run: its step counter only grows, so a second run needs a new object (the samplers make their own).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .lib import PbeError

STREAM_X_T = 0
STREAM_POST_EPS = 1
STREAM_STEP0 = 16


class SeededNoise:
    """The draws of one run for a batch of seeds.  seeds: an int64 tensor [B] on the GPU or a sequence of Python ints in [0, 2^64);
    sub: None, an int32 tensor [B] or ints in [0, 2^31); device: where the draws are made (default: the seeds' device, or the current
    GPU).  Every method draws for all B samples; shape[0] must be B."""

    def __init__(self, seeds, sub=None, device=None):
        self.seeds = ops.seed_tensor(seeds, None, device)
        self.batch = int(self.seeds.numel())
        if self.batch < 1:
            raise PbeError("SeededNoise: no seeds")
        self.sub = ops.sub_tensor(sub, self.batch, self.seeds.device)
        self.device = self.seeds.device
        self.steps = 0                                   # draws made after x_T: the next one uses STREAM_STEP0 + steps

    def _shape(self, shape):
        shape = tuple(int(s) for s in shape)
        if len(shape) < 1 or shape[0] != self.batch:
            raise PbeError(f"SeededNoise: shape {shape} for {self.batch} seeds (the leading size is one sample per seed)")
        return shape

    def x_T(self, shape) -> torch.Tensor:
        return ops.randn_seeded(self.seeds, self._shape(shape), STREAM_X_T, sub=self.sub)

    def post_eps(self, shape) -> torch.Tensor:
        return ops.randn_seeded(self.seeds, self._shape(shape), STREAM_POST_EPS, sub=self.sub)

    def _next_stream(self) -> int:
        s = STREAM_STEP0 + self.steps
        self.steps += 1
        return s

    def noise_like(self, shape, device=None) -> torch.Tensor:
        """The i-th call in the object's life (add_noise_ counts too) draws stream STREAM_STEP0 + i.  `device` is the samplers'
        noise_like signature; the draw is made where the seeds live."""
        if device is not None and torch.device(device).type != self.device.type:
            raise PbeError(f"SeededNoise.noise_like: asked for {device}, the seeds live on {self.device}")
        return ops.randn_seeded(self.seeds, self._shape(shape), self._next_stream(), sub=self.sub)

    def add_noise_(self, img: torch.Tensor, scale: float) -> torch.Tensor:
        """img += scale * z in place, z the next step stream: one launch, no temporary (the bits of ops.axpy_ on noise_like's draw)."""
        return ops.randn_seeded(self.seeds, self._shape(img.shape), self._next_stream(), sub=self.sub, out=img, a=1.0, b=float(scale))
