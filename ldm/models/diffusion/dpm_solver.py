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
from ldm.models.diffusion.plms import PLMSSampler


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
    accepts_rest = True
    blend_ref = "ddim.py:178-181"

    def _own_options(self, conditioning, batch_size, eta, temperature, kwargs):
        """sample(order=): 2 = DPM-Solver++(2M), 1 = its first order, which is DDIM with eta = 0.  eta must be 0."""
        if eta != 0:
            raise PbeError("DPMSolverSampler: eta must be 0 (the stochastic SDE-DPM-Solver++ variant is not built)")
        if kwargs.get("order", 2) not in (1, 2):
            raise PbeError(f"DPMSolverSampler: order must be 1 or 2, got {kwargs['order']!r}")
        return 0., self.dpm_sampling, kwargs

    @torch.no_grad()
    def dpm_sampling(self, cond, shape, x_T=None, callback=None, img_callback=None, log_every_t=100, unconditional_guidance_scale=1.,
                     unconditional_conditioning=None, timesteps=None, mask=None, x0=None, conditioning_weights=None,
                     conditioning_regions=None, conditioning_maps=None, order=2, **kwargs):
        run = self._begin_run(cond, shape, x_T, timesteps, unconditional_guidance_scale, unconditional_conditioning, mask, x0,
                              conditioning_weights, conditioning_regions, conditioning_maps, kwargs)
        # the run covers grid rows total-1 .. 0: its first and last steps are first order whatever prefix `timesteps=` selects
        coef = dpmpp_coefficients(self.ddim_alphas[:run.total], self.ddim_alphas_prev[:run.total], order) if run.total else None
        x0_prev = None                                                    # the history: the previous step's data prediction

        def update(i, index, img, eps):
            nonlocal x0_prev
            k = coef[index].tolist()
            img, x0_prev = ops.dpmpp_update(eps, run.dup, run.scale, img, x0_prev if k[4] != 0.0 else None, k)
            return img, x0_prev
        return self._run_loop(run, update, callback, img_callback, log_every_t)
