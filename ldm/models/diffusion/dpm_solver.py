"""DPM-Solver++(2M) sampler for Paint-by-Example on MI355X: the second-order multistep solver in data-prediction form (Lu et al. 2022,
"DPM-Solver++", algorithm 2) that upstream Stable Diffusion ships as ``ldm.models.diffusion.dpm_solver.DPMSolverSampler`` /
``--dpm_solver``.  zhanwenchen/pbe has no such sampler: there is no reference code to pin it to, so its FIRST order is pinned to the
reference's DDIM (eta = 0), which it equals on the same grid, and its second order is shown on an analytic model.

``DPMSolverSampler(model).sample(S, batch_size, shape, conditioning, ..., order=2)`` -> ``(samples, {'x_inter', 'pred_x0'})`` with the
signature of DDIMSampler.sample.  S steps are S U-Net calls (PLMS: S + 1).  The grid is the DDIM grid of make_schedule: step index i
goes from a = ddim_alphas[i] to a' = ddim_alphas_prev[i] (cumulative alphas).  With alpha = sqrt(a), sigma = sqrt(1 - a),
lambda = ln(alpha / sigma), h = lambda' - lambda and x0 = (x - sigma e) / alpha the data prediction of the step:

    first order :  x' = (sigma'/sigma) x - alpha' expm1(-h) x0
    second order:  x' = (sigma'/sigma) x - alpha' expm1(-h) [(1 + 1/(2r)) x0 - 1/(2r) x0_previous],   r = h_previous / h

The first step of a run has no history and is first order; so is the last (the usual lower-order final step).  The coefficients are
fp64 host arithmetic (dpmpp_coefficients) handed to ONE kernel per step (pbe_dpmpp_update: guidance combine, x0, x'); the history is one
tensor, the previous x0.  Everything around the update is the other samplers' (PLMSSampler._eps: multi-exemplar contexts, weights,
regions, attribution maps, the shared guidance prefix, HIP graphs; _blend_known; _schedule_subset).  eta != 0 (the SDE variant) and
orders above 2 are not built and raise."""
import numpy as np
import torch

from pbe_amd import ops
from pbe_amd.lib import PbeError
from ldm.models.diffusion.plms import PLMSSampler, guidance_context, guidance_maps, guidance_regions, guidance_weights, inpaint_kwargs


def dpmpp_coefficients(alphas, alphas_prev, order=2):
    """The per-step scalars of a run over the grid rows i = n-1 .. 0 (row i: cumulative alpha alphas[i] -> alphas_prev[i]; the run
    STARTS at the last row, like the DDIM loop) -> float64 [n, 5] = {sigma_t, 1/alpha_t, kx, k0, k1} per row, the coef5 of
    pbe_dpmpp_update.  order 2: rows n-2 .. 1 are second order with r = h[i + 1] / h[i]; the first (n-1) and last (0) rows, and every
    row with order 1, are first order (k1 = 0).  Pure host arithmetic in fp64; a grid that does not move towards the data in every row
    (h <= 0: a repeated timestep, as the `quad` discretisation can produce) is refused."""
    if order not in (1, 2):
        raise PbeError(f"DPMSolverSampler: order must be 1 or 2, got {order!r}")
    a, ap = np.asarray(alphas, dtype=np.float64).reshape(-1), np.asarray(alphas_prev, dtype=np.float64).reshape(-1)
    if a.shape != ap.shape or a.size == 0 or not (np.all((a > 0) & (a < 1)) and np.all((ap > 0) & (ap < 1))):
        raise PbeError("DPMSolverSampler: the grid needs as many alphas as previous alphas, all inside (0, 1)")
    alpha, sigma, alpha_n, sigma_n = np.sqrt(a), np.sqrt(1.0 - a), np.sqrt(ap), np.sqrt(1.0 - ap)
    h = np.log(alpha_n / sigma_n) - np.log(alpha / sigma)
    if not np.all(h > 0):
        bad = int(np.flatnonzero(~(h > 0))[-1])
        raise PbeError(f"DPMSolverSampler: grid row {bad} does not move towards the data (h = {h[bad]:.3e} <= 0: a repeated or "
                       "increasing timestep); use a discretisation with distinct timesteps")
    phi = -np.expm1(-h)                                   # 1 - exp(-h)
    out = np.zeros((a.size, 5), dtype=np.float64)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = sigma, 1.0 / alpha, sigma_n / sigma, alpha_n * phi
    if order == 2:
        for i in range(1, a.size - 1):
            r = h[i + 1] / h[i]                           # the step before row i was row i + 1
            out[i, 3] = alpha_n[i] * phi[i] * (1.0 + 0.5 / r)
            out[i, 4] = -alpha_n[i] * phi[i] * (0.5 / r)
    return out


class DPMSolverSampler(PLMSSampler):
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None, quantize_x0=False,
               eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, verbose=True,
               x_T=None, log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None, disable_tqdm=True,
               conditioning_weights=None, conditioning_regions=None, conditioning_maps=None, order=2, seeds=None, seed_sub=None, **kwargs):
        """The arguments of DDIMSampler.sample (conditioning_weights / conditioning_regions / conditioning_maps / seeds / seed_sub as in
        PLMSSampler.sample) plus order: 2 = DPM-Solver++(2M), 1 = its first order, which is DDIM with eta = 0.  eta must be 0."""
        if conditioning is None:
            raise PbeError("DPMSolverSampler.sample: conditioning is required")
        if quantize_x0 or score_corrector is not None or noise_dropout != 0.:
            raise PbeError("DPMSolverSampler: quantize_x0 / score_corrector / noise_dropout are not on the Paint-by-Example path")
        if (mask is None) != (x0 is None):
            raise PbeError("DPMSolverSampler: mask and x0 go together (ddim.py:178-181)")
        if eta != 0:
            raise PbeError("DPMSolverSampler: eta must be 0 (the stochastic SDE-DPM-Solver++ variant is not built)")
        if order not in (1, 2):
            raise PbeError(f"DPMSolverSampler: order must be 1 or 2, got {order!r}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=0., verbose=verbose)
        C, H, W = shape
        try:
            x_T = self._seed_run(seeds, seed_sub, x_T, (batch_size, C, H, W))
            return self.dpm_sampling(conditioning, (batch_size, C, H, W), callback=callback, img_callback=img_callback, x_T=x_T,
                                     log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                     unconditional_conditioning=unconditional_conditioning, mask=mask, x0=x0,
                                     conditioning_weights=conditioning_weights, conditioning_regions=conditioning_regions,
                                     conditioning_maps=conditioning_maps, order=order, **kwargs)
        finally:
            self._seeded = None

    @torch.no_grad()
    def dpm_sampling(self, cond, shape, x_T=None, callback=None, img_callback=None, log_every_t=100, unconditional_guidance_scale=1.,
                     unconditional_conditioning=None, timesteps=None, mask=None, x0=None, conditioning_weights=None,
                     conditioning_regions=None, conditioning_maps=None, order=2, **kwargs):
        device = self.model.betas.device
        if self.require_gpu and device.type != "cuda":
            raise PbeError("DPMSolverSampler: the model must live on an MI355X; there is no CPU path")
        b = shape[0]
        img = (torch.randn(shape, device=device) if x_T is None else x_T.to(device=device, dtype=torch.float32)).contiguous()
        if "rest" in kwargs and "test_model_kwargs" not in kwargs:       # ddim.py:201-202: rest = cat(z_inpaint, mask)
            rest = kwargs["rest"]
            z_inp, msk = rest[:, :4], rest[:, 4:5]
        else:
            z_inp, msk = inpaint_kwargs(kwargs)
        z_inp = z_inp.to(device=device, dtype=torch.float32).contiguous()
        msk = msk.to(device=device, dtype=torch.float32).contiguous()
        guided = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
        if guided:
            ctx = guidance_context(cond, unconditional_conditioning, b, device)      # a one-token uc is repeated to cond's K tokens (exact: plms.py)
        else:
            ctx = cond.to(device=device, dtype=torch.float16).contiguous()
        dup = 2 if guided else 1
        ctx_w = guidance_weights(conditioning_weights, cond, b, guided)
        ctx_r = guidance_regions(conditioning_regions, cond, b, guided)
        ctx_m = guidance_maps(conditioning_maps, cond, b, device)
        scale = float(unconditional_guidance_scale)
        time_range = np.flip(self._schedule_subset(timesteps))
        total = time_range.shape[0]
        # the run covers grid rows total-1 .. 0: its first and last steps are first order whatever prefix `timesteps=` selects
        coef = dpmpp_coefficients(self.ddim_alphas[:total], self.ddim_alphas_prev[:total], order) if total else None
        if mask is not None:
            mask, x0 = mask.to(device=device, dtype=torch.float32), x0.to(device=device, dtype=torch.float32)
        inter = {"x_inter": [img], "pred_x0": [img]}
        x0_prev = None                                                    # the history: the previous step's data prediction
        for i, step in enumerate(time_range):
            index = total - i - 1
            if mask is not None:
                img = self._blend_known(img, x0, mask, step)
            eps = self._eps(img, step, ctx, z_inp, msk, dup, ctx_w, ctx_r, ctx_m)
            k = coef[index].tolist()
            img, pred_x0 = ops.dpmpp_update(eps, dup, scale, img, x0_prev if k[4] != 0.0 else None, k)
            x0_prev = pred_x0
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total - 1:
                inter["x_inter"].append(img)
                inter["pred_x0"].append(pred_x0)
        return img, inter
