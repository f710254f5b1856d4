"""PLMS (pseudo linear multistep) sampler for Paint-by-Example on MI355X — drop-in for
ldm/models/diffusion/plms.py:11-248 in zhanwenchen/pbe: ``PLMSSampler(model).sample(S, batch_size,
shape, conditioning, ..., unconditional_guidance_scale, unconditional_conditioning, x_T,
test_model_kwargs)`` -> ``(samples, {'x_inter', 'pred_x0'})``.

What differs from the reference loop (same arithmetic):
  * the schedule scalars never go to the device as tensors (the reference uploads four
    ``torch.full`` scalars per update, plms.py:204-207): they are kernel arguments,
  * per step ONE kernel builds the CFG-doubled 9-channel NHWC input (plms.py:185,225) and ONE
    kernel does the guidance combine, the Adams-Bashforth blend and the x_prev / pred_x0 update
    (plms.py:188-189, 202-219, 230-244); the state x stays fp32 NCHW like the reference's,
  * the U-Net is entered through its NHWC fast path, and the [uc | c] context is built once so
    the 16 cross-attention constants are computed once per run,
  * ``test_model_kwargs`` may use either key spelling (``inpaint_image``/``inpaint_mask`` from
    scripts/inference.py:320-332 or ``images_inpaint``/``images_mask`` from plms.py:221-222).
  * ``mask`` / ``x0`` (plms.py:150-153: img = q_sample(x0, ts) * mask + (1 - mask) * img before every step) and ``timesteps=``
    (plms.py:132-139: a prefix of the schedule) run as in the reference; the q_sample noise comes from ``self.noise_like``
    (default: the torch device generator, like the reference's randn_like - tests inject it).
Unsupported reference options (score_corrector, quantize_denoised, eta != 0 - the reference's PLMS asserts that too -,
noise_dropout, ddim_use_original_steps) raise instead of being silently ignored.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from pbe_amd import ops
from pbe_amd.graph import GraphedUNet, graphs_enabled
from pbe_amd.lib import PbeError
from ldm.modules.attention import Conditioning
from ldm.modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps

_AB = {0: (1.0,), 1: (3 / 2, -1 / 2), 2: (23 / 12, -16 / 12, 5 / 12), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


def inpaint_kwargs(kwargs):
    tmk = kwargs.get("test_model_kwargs")
    if tmk is None:
        raise PbeError("sample(): test_model_kwargs with the inpainting latent and mask is required (plms.py:220-222)")
    z = tmk.get("images_inpaint", tmk.get("inpaint_image"))
    m = tmk.get("images_mask", tmk.get("inpaint_mask"))
    if z is None or m is None:
        raise PbeError("test_model_kwargs needs images_inpaint/images_mask (or inpaint_image/inpaint_mask)")
    return z, m


def guidance_context(cond, uc, b, device):
    """The [uc | c] context of a guidance pair (plms.py:185-187) as fp16 [2b, K, D].  cond [b, K, D] may hold K >= 1 tokens per sample
    (several exemplars); a ONE-token uc is repeated to K tokens.  That is exact, not an approximation: K copies of one key give K equal
    scores, the softmax weights are 1/K each, and the weighted sum of K equal values is that value - attn2 of the repeated context is
    attn2 of the single token.  Any other difference in length is refused: samples with different exemplar counts are padded to one K
    and given per-sample weights (guidance_weights; pbe_amd.pipeline.pad_conditionings builds both)."""
    uc = uc.to(device)
    cond = cond.to(device)
    if uc.shape[0] != b:                           # scripts/inference.py:325 hands [1,1,768]; the test bench repeats it
        uc = uc.expand(b, *uc.shape[1:])
    if uc.dim() != 3 or cond.dim() != 3:
        raise PbeError(f"sampler: conditioning must be [B, K, D], got {tuple(cond.shape)} / {tuple(uc.shape)}")
    if uc.shape[1] != cond.shape[1]:
        if uc.shape[1] != 1:
            raise PbeError(f"sampler: unconditional_conditioning has {uc.shape[1]} tokens, conditioning {cond.shape[1]}: "
                           "only a one-token unconditional context can be repeated (per-sample exemplar counts go through "
                           "conditioning_weights, with weight 0 on the padding tokens)")
        uc = uc.expand(-1, cond.shape[1], -1)
    return torch.cat((uc.to(torch.float16), cond.to(torch.float16))).contiguous()


def _guidance_rows(v, cond, b, guided, name, extra, per):
    """The body of guidance_weights (extra = ()) and guidance_regions (extra = ("Hr", "Wr")): [b, K, *extra] -> fp64 on the host, with
    a leading half of ones under guidance."""
    if v is None:
        return None
    v = torch.as_tensor(v).detach().to("cpu", torch.float64)
    if v.dim() != 2 + len(extra) or tuple(v.shape[:2]) != (b, cond.shape[1]):
        want = ", ".join([str(b), str(cond.shape[1]), *extra])
        raise PbeError(f"sampler: {name} must be [{want}] ({per} per conditioning token), got {tuple(v.shape)}")
    return torch.cat((torch.ones_like(v), v)).contiguous() if guided else v.contiguous()


def guidance_weights(weights, cond, b, guided):
    """Exemplar weights of the context guidance_context builds: conditioning_weights [b, K] (>= 0, positive sum per sample, 0 = token
    absent) -> fp64 host tensor [2b, K] for a guidance pair (the unconditional half gets ones: on K copies of one token any weights
    with a positive sum give that token, for the reason above) or [b, K] unguided; None for None.  One tensor per run, so the U-Net's
    per-context cache sees one identity across the steps; validated where the operands are built (attention.prepare_context_weights)."""
    return _guidance_rows(weights, cond, b, guided, "conditioning_weights", (), "one")


def guidance_regions(regions, cond, b, guided):
    """Region maps of the context guidance_context builds: conditioning_regions [b, K, Hr, Wr] (>= 0; 1 = token j counts fully at that
    position) -> fp64 host tensor [2b, K, Hr, Wr] for a guidance pair (the unconditional half gets ones: uc is one token repeated K
    times, and any weights with a positive sum give that token) or [b, K, Hr, Wr] unguided; None for None.  One tensor per run, like
    guidance_weights; validated where the tables are built (attention.prepare_context_regions)."""
    return _guidance_rows(regions, cond, b, guided, "conditioning_regions", ("Hr", "Wr"), "one map")


def guidance_maps(maps, cond, b, device):
    """conditioning_maps (an attention.ContextMaps or None) bound to the run: b samples x cond's K tokens.  In a guidance batch
    cat([uc, c]) those are the LAST b samples - the conditional half; the unconditional half (one token repeated) is not collected."""
    if maps is None:
        return None
    if not all(hasattr(maps, a) for a in ("bind", "level", "note", "result")):
        raise PbeError("sampler: conditioning_maps must be an ldm.modules.attention.ContextMaps")
    return maps.bind(b, cond.shape[1], device)


class PLMSSampler(object):
    _seeded = None                    # a pbe_amd.noise.SeededNoise for the length of one sample(seeds=...) call, else None

    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.use_graph = None               # None = decide per run (pbe_amd.graph.graphs_enabled); True / False force
        self._graphed = None
        self.share_guidance_prefix = True   # evaluate the context-independent prefix of a guidance pair once (UNetModel.forward_nhwc paired=True)
        self.noise_like = lambda shape, device: torch.randn(shape, device=device)      # util.py:264-267 (q_sample / DDIM eta > 0 noise)
        self.require_gpu = True       # host-logic tests clear this and substitute the two element-wise kernels; the kernels themselves have no CPU path

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def _seed_run(self, seeds, seed_sub, x_T, shape):
        """sample(seeds=...): the start latent and, until the call returns, every noise draw come from one pbe_amd.noise.SeededNoise
        (sample i a function of seeds[i] alone; the stream plan is that module's docstring).  Without seeds: x_T as it came, no launch."""
        if seeds is None:
            if seed_sub is not None:
                raise PbeError("sample(): seed_sub names substreams of seeds, which are missing")
            return x_T
        if x_T is not None:
            raise PbeError("sample(): seeds and x_T both given - the start latent is either drawn from the seeds or handed in")
        from pbe_amd.noise import SeededNoise
        self._seeded = SeededNoise(seeds, seed_sub, device=self.model.betas.device)
        return self._seeded.x_T(shape)

    def _noise(self, shape, device):
        return self.noise_like(shape, device) if self._seeded is None else self._seeded.noise_like(shape, device)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        ac = self.model.alphas_cumprod.detach().float().cpu()
        assert ac.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        self.register_buffer("betas", self.model.betas)
        self.register_buffer("alphas_cumprod", self.model.alphas_cumprod)
        self.register_buffer("alphas_cumprod_prev", self.model.alphas_cumprod_prev)
        sig, a, a_prev = make_ddim_sampling_parameters(alphacums=ac.numpy(), ddim_timesteps=self.ddim_timesteps, eta=ddim_eta, verbose=verbose)
        self.register_buffer("ddim_sigmas", sig)
        self.register_buffer("ddim_alphas", a)                      # float32 numpy, selected from the fp32 buffer like the reference
        self.register_buffer("ddim_alphas_prev", a_prev)
        self.register_buffer("ddim_sqrt_one_minus_alphas", np.sqrt(1. - a))

    accepts_rest = False              # ddim.py:201-202's `rest=` spelling of the inpainting inputs: DDIMSampler and DPMSolverSampler take it
    blend_ref = "plms.py:150-153"     # where the reference blends mask / x0 (named when only one of them is given)

    def _own_options(self, conditioning, batch_size, eta, temperature, kwargs):
        """What the shared sample() leaves to each sampler: its own checks -> (the schedule's eta, its loop, the loop's further keywords)."""
        if conditioning.shape[0] != batch_size:
            print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
        return eta, self.plms_sampling, kwargs

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None, quantize_x0=False,
               eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, verbose=True,
               x_T=None, log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None, conditioning_weights=None,
               conditioning_regions=None, conditioning_maps=None, seeds=None, seed_sub=None, **kwargs):
        """The sample() of all three samplers; what is a sampler's own is in its _own_options (DDIMSampler: eta > 0 and temperature;
        DPMSolverSampler: order=).
        seeds: per-sample noise seeds (an int64 tensor [batch_size] on the GPU or ints in [0, 2^64)), seed_sub their substreams or
        None: x_T (which must then be None) and the q_sample noise are drawn by pbe_amd.noise.SeededNoise, sample i from seeds[i] alone.
        conditioning_weights: per-sample exemplar weights [batch_size, K] over conditioning's K tokens (>= 0, positive sum per sample;
        0 = token absent, so a ragged batch is padded to one K), or None: every token counts once.
        conditioning_regions: per-sample, per-token region maps [batch_size, K, Hr, Wr] >= 0 (regional exemplars: where each token
        applies; every transformer level's grid must divide Hr x Wr), or None: every token applies everywhere.
        conditioning_maps: an attention.ContextMaps or None.  It collects the attribution maps of the run - the share of cross-attention
        each conditioning token received at each position, from every U-Net call of the run (the probe call included); under guidance
        only the CONDITIONAL half is collected.  With it every level runs the fused cross-attention kernel: with regions the samples are
        those of the run without it bit for bit, without regions those of a run whose blocks have ctx_fused_max_width = 1280."""
        name = type(self).__name__
        if conditioning is None:
            raise PbeError(f"{name}.sample: conditioning is required")
        if quantize_x0 or score_corrector is not None or noise_dropout != 0.:
            raise PbeError(f"{name}: quantize_x0 / score_corrector / noise_dropout are not on the Paint-by-Example path")
        if (mask is None) != (x0 is None):
            raise PbeError(f"{name}: mask and x0 go together ({self.blend_ref})")
        eta, loop, kwargs = self._own_options(conditioning, batch_size, eta, temperature, kwargs)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        try:
            x_T = self._seed_run(seeds, seed_sub, x_T, (batch_size, C, H, W))
            return loop(conditioning, (batch_size, C, H, W), callback=callback, img_callback=img_callback, x_T=x_T, log_every_t=log_every_t,
                        unconditional_guidance_scale=unconditional_guidance_scale, unconditional_conditioning=unconditional_conditioning,
                        mask=mask, x0=x0, conditioning_weights=conditioning_weights, conditioning_regions=conditioning_regions,
                        conditioning_maps=conditioning_maps, **kwargs)
        finally:
            self._seeded = None

    # ---- one U-Net evaluation with guidance (plms.py:181-195) -----------------------------------
    def _eps(self, x, step, cond, z_inp, msk, dup):
        """cond: the run's attention.Conditioning.  A plain context hands the U-Net no keyword beyond paired= and step=."""
        b = x.shape[0]
        t = torch.full((dup * b,), int(step), device=x.device, dtype=torch.int64)
        unet = self.model.model.diffusion_model
        # cat([x]*2), cat([t]*2) (plms.py:183-184): both halves share x and t; the U-Net evaluates the common prefix once
        paired = dup == 2 and self.share_guidance_prefix
        x9 = ops.plms_pack_input(x, z_inp, msk, 1 if paired else dup)
        if (graphs_enabled(dup * b) if self.use_graph is None else self.use_graph) and x.is_cuda:      # launch-bound regime: one HIP graph per call
            if self._graphed is None or self._graphed.unet is not unet:
                self._graphed = GraphedUNet(unet)
            return self._graphed(x9, t, cond, paired)
        # every row of t is `step`: the embedding rows come from the per-value cache.  A collector covers the last b samples: the conditional half
        return unet.forward_nhwc(x9, t, cond.context, paired=paired, step=int(step), **cond.kwargs())

    def _coef(self, index, weights):
        a_t, a_prev = float(self.ddim_alphas[index]), float(self.ddim_alphas_prev[index])
        w = list(weights) + [0.0] * (4 - len(weights))
        return w + [float(self.ddim_sqrt_one_minus_alphas[index]), 1.0 / math.sqrt(a_t), math.sqrt(a_prev), math.sqrt(1.0 - a_prev)]

    def _schedule_subset(self, timesteps):
        """plms.py:132-139 / ddim.py:151-155: `timesteps` = how many of the schedule's steps to run (a prefix of ddim_timesteps)."""
        if timesteps is None:
            return self.ddim_timesteps
        n = self.ddim_timesteps.shape[0]
        subset_end = int(min(timesteps / n, 1) * n) - 1
        return self.ddim_timesteps[:subset_end]

    def _blend_known(self, img, x0, mask, step):
        """img_orig = q_sample(x0, ts); img = img_orig * mask + (1 - mask) * img (plms.py:150-153), one kernel."""
        ac = float(self.model.alphas_cumprod[int(step)])
        return ops.qsample_blend(x0, self._noise(tuple(x0.shape), x0.device).float(), mask, img, math.sqrt(ac), math.sqrt(1.0 - ac))

    # ---- the frame of a run: prelude and loop, shared by the three samplers; each hands the loop its update ------------------------
    def _begin_run(self, cond, shape, x_T, timesteps, unconditional_guidance_scale, unconditional_conditioning, mask, x0,
                   conditioning_weights, conditioning_regions, conditioning_maps, kwargs):
        """The state of one run: img (the start latent), z_inp / msk (the inpainting inputs), cond (the attention.Conditioning every
        U-Net call of the run gets: one object, so both per-conditioning caches see one identity across the steps), dup (2 = a
        guidance pair), scale, time_range (reversed; a prefix of the schedule for timesteps=), total, and mask / x0 on the device."""
        device = self.model.betas.device
        if self.require_gpu and device.type != "cuda":
            raise PbeError(f"{type(self).__name__}: the model must live on an MI355X (model.to('cuda')); there is no CPU path")
        b = shape[0]
        img = (torch.randn(shape, device=device) if x_T is None else x_T.to(device=device, dtype=torch.float32)).contiguous()
        if self.accepts_rest and "rest" in kwargs and "test_model_kwargs" not in kwargs:       # ddim.py:201-202: rest = cat(z_inpaint, mask)
            z_inp, msk = kwargs["rest"][:, :4], kwargs["rest"][:, 4:5]
        else:
            z_inp, msk = inpaint_kwargs(kwargs)
        z_inp = z_inp.to(device=device, dtype=torch.float32).contiguous()
        msk = msk.to(device=device, dtype=torch.float32).contiguous()
        cond = cond.to(device)
        guided = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
        if guided:
            ctx = guidance_context(cond, unconditional_conditioning, b, device)      # a one-token uc is repeated to cond's K tokens (exact)
        else:
            ctx = cond.to(torch.float16).contiguous()
        cond = Conditioning(ctx, guidance_weights(conditioning_weights, cond, b, guided), guidance_regions(conditioning_regions, cond, b, guided),
                            guidance_maps(conditioning_maps, cond, b, device))
        time_range = np.flip(self._schedule_subset(timesteps))
        if mask is not None:
            mask, x0 = mask.to(device=device, dtype=torch.float32), x0.to(device=device, dtype=torch.float32)
        return SimpleNamespace(img=img, z_inp=z_inp, msk=msk, cond=cond, dup=2 if guided else 1, scale=float(unconditional_guidance_scale),
                               time_range=time_range, total=time_range.shape[0], mask=mask, x0=x0)

    def _run_loop(self, run, update, callback, img_callback, log_every_t):
        """Per step: blend the known region in (mask / x0), evaluate the U-Net, update(i, index, img, eps) -> (img, pred_x0) - the
        sampler's own part -, then the callbacks and the log -> (img, {'x_inter', 'pred_x0'})."""
        img = run.img
        inter = {"x_inter": [img], "pred_x0": [img]}
        for i, step in enumerate(run.time_range):
            index = run.total - i - 1
            if run.mask is not None:
                img = self._blend_known(img, run.x0, run.mask, step)
            eps = self._eps(img, step, run.cond, run.z_inp, run.msk, run.dup)
            img, pred_x0 = update(i, index, img, eps)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == run.total - 1:
                inter["x_inter"].append(img)
                inter["pred_x0"].append(pred_x0)
        return img, inter

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, callback=None, timesteps=None, img_callback=None, log_every_t=100,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, mask=None, x0=None, conditioning_weights=None,
                      conditioning_regions=None, conditioning_maps=None, **kwargs):
        run = self._begin_run(cond, shape, x_T, timesteps, unconditional_guidance_scale, unconditional_conditioning, mask, x0,
                              conditioning_weights, conditioning_regions, conditioning_maps, kwargs)
        old = []                                                      # newest last, at most 3 (plms.py:163-165)

        def update(i, index, img, eps):
            if len(old) == 0:
                # pseudo improved Euler (plms.py:230-235): probe x_prev with e_t, re-evaluate at t_next, average
                x_probe, _, e_t = ops.plms_update(eps, run.dup, run.scale, img, [], self._coef(index, _AB[0]), want_pred=False)
                eps2 = self._eps(x_probe, run.time_range[min(i + 1, run.total - 1)], run.cond, run.z_inp, run.msk, run.dup)
                # e' = (e_t + e_next)/2 : c0 weights the fresh eps (= e_next), history slot 1 = e_t
                img, pred_x0, _ = ops.plms_update(eps2, run.dup, run.scale, img, [e_t], self._coef(index, (0.5, 0.5)), want_e_t=False)
            else:
                hist = old[::-1]
                img, pred_x0, e_t = ops.plms_update(eps, run.dup, run.scale, img, hist, self._coef(index, _AB[len(hist)]))
            old.append(e_t)
            if len(old) >= 4:
                old.pop(0)
            return img, pred_x0
        return self._run_loop(run, update, callback, img_callback, log_every_t)
