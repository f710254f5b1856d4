"""DDIM sampler for Paint-by-Example on MI355X — drop-in for ldm/models/diffusion/ddim.py:22-283 in
zhanwenchen/pbe (selected when ``--plms`` is absent, scripts/inference.py:277-280).  One U-Net
evaluation per step; the 9-channel concat (ddim.py:197-202, incl. the ``rest=`` spelling), guidance
combine and the x_prev / pred_x0 update (:222-241, pred_x0 from x[:, :4]) are the same two fused
kernels the PLMS sampler uses.  eta > 0 (scripts/inference.py:164 --ddim_eta): the direction term uses sqrt(1 - a_prev - sigma^2) and
sigma_t * noise * temperature is added by one more element-wise kernel (ddim.py:234-238); mask / x0 blending and timesteps= as in the
PLMS sampler.  The noise comes from ``self.noise_like`` (default: the torch device generator, like the reference)."""
import numpy as np
import torch

from pbe_amd import ops
from ldm.models.diffusion.plms import PLMSSampler


class DDIMSampler(PLMSSampler):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=0., verbose=verbose)
        if ddim_eta != 0:                                     # ddim.py:57-62 -> util.py:63-74
            from ldm.modules.diffusionmodules.util import make_ddim_sampling_parameters
            sig, _, _ = make_ddim_sampling_parameters(alphacums=self.model.alphas_cumprod.detach().float().cpu().numpy(), ddim_timesteps=self.ddim_timesteps,
                                                      eta=ddim_eta, verbose=verbose)
            self.register_buffer("ddim_sigmas", sig)

    accepts_rest = True
    blend_ref = "ddim.py:178-181"

    def _own_options(self, conditioning, batch_size, eta, temperature, kwargs):
        """eta > 0 is built here: with seeds the sigma_t term of each step is added by SeededNoise.add_noise_ (one launch, no temporary)."""
        return eta, self.ddim_sampling, dict(kwargs, temperature=temperature)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, callback=None, img_callback=None, log_every_t=100, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, timesteps=None, mask=None, x0=None, temperature=1., conditioning_weights=None,
                      conditioning_regions=None, conditioning_maps=None, **kwargs):
        run = self._begin_run(cond, shape, x_T, timesteps, unconditional_guidance_scale, unconditional_conditioning, mask, x0,
                              conditioning_weights, conditioning_regions, conditioning_maps, kwargs)

        def update(i, index, img, eps):
            coef = self._coef(index, (1.0,))
            sigma = float(self.ddim_sigmas[index])
            if sigma != 0.0:                                  # dir_xt = sqrt(1 - a_prev - sigma_t^2) e_t (ddim.py:234)
                coef[7] = float(np.sqrt(1.0 - float(self.ddim_alphas_prev[index]) - sigma * sigma))
            img, pred_x0, _ = ops.plms_update(eps, run.dup, run.scale, img, [], coef, want_e_t=False)
            if sigma != 0.0 and self._seeded is not None:     # the same term, drawn and added by one kernel
                self._seeded.add_noise_(img, sigma * float(temperature))
            elif sigma != 0.0:                                # + sigma_t * noise_like(...) * temperature (ddim.py:235-238)
                ops.axpy_(img, sigma * float(temperature), self.noise_like(tuple(img.shape), img.device).float().contiguous())
            return img, pred_x0
        return self._run_loop(run, update, callback, img_callback, log_every_t)
