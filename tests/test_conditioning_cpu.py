"""CPU suite: attention.Conditioning, the one value the samplers, GraphedUNet and the U-Net hand on.

  * key() - the identity both per-conditioning caches compare - is equal for the same tensors, differs after an in-place edit of the
    context, the weights or the regions, differs with and without a collector and between two collectors,
  * kwargs() names exactly what is present,
  * under each sampler a recording stub U-Net sees no keyword beyond paired= / step= for a plain context, and context_weights alone
    when only weights are given (the two element-wise ops are replaced by torch arithmetic IN THE TEST ONLY; no kernel is launched).
"""
import types

import pytest
import torch

from ldm.modules.attention import Conditioning, ContextMaps


def _parts():
    return torch.randn(2, 3, 8).half(), torch.tensor([[2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]).double(), torch.ones(2, 3, 4, 4).double()


def test_key_is_stable_and_follows_in_place_edits():
    ctx, w, r = _parts()
    cm = ContextMaps()
    full = Conditioning(ctx, w, r, cm)
    assert full.key() == Conditioning(ctx, w, r, cm).key() and Conditioning(ctx).key() == Conditioning(ctx).key()
    assert hash(full.key()) == hash(Conditioning(ctx, w, r, cm).key())                  # plain tuples: comparable and hashable
    for t in (ctx, w, r):
        before = full.key()
        t.mul_(1.0)                                                                       # same values, same storage: another _version
        assert full.key() != before
    # another storage with the same values is another conditioning; so is a list of other values
    assert Conditioning(ctx.clone(), w, r, cm).key() != full.key() and Conditioning(ctx, w.clone(), r, cm).key() != full.key()
    assert Conditioning(ctx, [[1.0, 1.0, 1.0]] * 2).key() == Conditioning(ctx, [[1.0, 1.0, 1.0]] * 2).key()
    assert Conditioning(ctx, [[1.0, 1.0, 1.0]] * 2).key() != Conditioning(ctx, [[1.0, 1.0, 2.0]] * 2).key()
    # each part has its own slot: weights are not mistaken for regions, nor a missing part for a present one
    keys = [Conditioning(ctx).key(), Conditioning(ctx, w).key(), Conditioning(ctx, None, r).key(), Conditioning(ctx, w, r).key()]
    assert len(set(keys)) == 4


def test_key_tells_collectors_apart():
    ctx, w, r = _parts()
    a, b = ContextMaps(), ContextMaps()
    none, ka, kb = Conditioning(ctx, w, r).key(), Conditioning(ctx, w, r, a).key(), Conditioning(ctx, w, r, b).key()
    assert none != ka and none != kb and ka != kb
    assert Conditioning(ctx, maps=a).key() == Conditioning(ctx, maps=a).key() != Conditioning(ctx).key()


def test_kwargs_names_exactly_what_is_present():
    ctx, w, r = _parts()
    cm = ContextMaps()
    names = ("context_weights", "context_regions", "context_maps")
    for present in [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]:
        vals = [v if i in present else None for i, v in enumerate((w, r, cm))]
        kw = Conditioning(ctx, *vals).kwargs()
        assert list(kw) == [names[i] for i in present]
        assert all(kw[names[i]] is vals[i] for i in present)


class _RecordingUNet:
    """model.model.diffusion_model: records the keywords of every call, eps = a fixed function of x."""

    def __init__(self):
        self.seen = []

    def forward_nhwc(self, x9, t, ctx, paired=False, step=None, **kw):
        assert step is not None and bool((t == int(step)).all()) and ctx.shape[0] == t.shape[0]
        self.seen.append(kw)
        if paired:
            x9 = torch.cat([x9, x9])
        return 0.1 * x9[..., :4].contiguous()


def _sampler(name, monkeypatch):
    from ldm.models.diffusion import ddim, dpm_solver, plms
    from ldm.models.diffusion.ddpm import DDPM

    def pack(x, z, m, dup):
        return torch.cat([torch.cat([x, z, m], 1).permute(0, 2, 3, 1)] * dup)

    def guided(eps, dup, scale):
        e = eps.float().permute(0, 3, 1, 2)
        return e if dup == 1 else e[:e.shape[0] // 2] + scale * (e[e.shape[0] // 2:] - e[:e.shape[0] // 2])

    def plms_update(eps, dup, scale, x, hist, coef, want_e_t=True, want_pred=True):
        e = guided(eps, dup, scale)
        ep = coef[0] * e + sum(c * h for h, c in zip(hist, coef[1:4]))
        px0 = (x - coef[4] * ep) * coef[5]
        return coef[6] * px0 + coef[7] * ep, px0, e

    def dpmpp_update(eps, dup, scale, x, x0_prev, k, want_pred=True):
        px0 = (x - k[0] * guided(eps, dup, scale)) * k[1]
        return k[2] * x + k[3] * px0 + (0.0 if x0_prev is None else k[4] * x0_prev), px0

    monkeypatch.setattr(plms.ops, "plms_pack_input", pack)
    monkeypatch.setattr(plms.ops, "plms_update", plms_update)
    monkeypatch.setattr(plms.ops, "dpmpp_update", dpmpp_update)
    m = DDPM.__new__(DDPM)
    torch.nn.Module.__init__(m)
    m.v_posterior = 0.0
    m.register_schedule(linear_start=0.00085, linear_end=0.0120, timesteps=1000)
    unet = _RecordingUNet()
    model = types.SimpleNamespace(num_timesteps=1000, betas=m.betas, alphas_cumprod=m.alphas_cumprod, alphas_cumprod_prev=m.alphas_cumprod_prev,
                                  model=types.SimpleNamespace(diffusion_model=unet))
    smp = {"plms": plms.PLMSSampler, "ddim": ddim.DDIMSampler, "dpm": dpm_solver.DPMSolverSampler}[name](model)
    smp.require_gpu = False
    return smp, unet


@pytest.mark.parametrize("name,calls", [("plms", 5), ("ddim", 4), ("dpm", 4)])
def test_samplers_pass_only_the_keywords_of_what_is_given(monkeypatch, name, calls):
    smp, unet = _sampler(name, monkeypatch)
    g = torch.Generator().manual_seed(3)
    kw = dict(S=4, batch_size=2, shape=[4, 4, 4], conditioning=torch.randn(2, 3, 8, generator=g), verbose=False, unconditional_guidance_scale=5.0,
              unconditional_conditioning=torch.randn(1, 1, 8, generator=g), x_T=torch.randn(2, 4, 4, 4, generator=g),
              test_model_kwargs={"inpaint_image": torch.randn(2, 4, 4, 4, generator=g), "inpaint_mask": torch.ones(2, 1, 4, 4)})
    with torch.no_grad():
        plain, _ = smp.sample(**kw)
    assert unet.seen == [{}] * calls                                   # PLMS: S + 1 calls (the probe), the others S
    del unet.seen[:]
    with torch.no_grad():
        smp.sample(conditioning_weights=[[2.0, 1.0, 0.0], [0.0, 0.0, 1.0]], **kw)
    assert len(unet.seen) == calls and all(list(s) == ["context_weights"] for s in unet.seen)
    w = unet.seen[0]["context_weights"]
    assert all(s["context_weights"] is w for s in unet.seen)           # one tensor per run: one cache identity across the steps
    assert w.tolist() == [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]      # [uc | c]: the unconditional half gets ones
    assert torch.isfinite(plain).all()
