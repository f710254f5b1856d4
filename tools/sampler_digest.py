"""One sha256 per sampler run over the conditioning / launch-path matrix, through the public sample() interface only - so the same
file runs in any tree, and two trees that print the same rows compute the same bits along the whole host path from sampler to block:

    python tools/sampler_digest.py > digests.txt       (it imports the ldm / pbe_amd / tests of the tree it lies in: copy it to compare trees)

Rows = {PLMS, DDIM eta 0, DDIM eta 0.5 with seeds, DPM-Solver++ order 2}
     x {one-token context, K = 3 with weights (one of them 0), K = 3 with regions, K = 3 with regions and a ContextMaps collector}
     x {eager paired, eager with share_guidance_prefix = False, use_graph = True}
on the narrow U-Net of the GPU tests (tests/cases.UNET_NARROW, name-seeded weights), 16 x 16 latents, batch 2, S = 6 (PLMS reaches its
three-deep history).  With a collector the row also carries the digest of ContextMaps.result((16, 16)) and the launch counts."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch                                                            # noqa: E402
import cases                                                            # noqa: E402
import modelbuild                                                       # noqa: E402
from ldm.models.diffusion.ddim import DDIMSampler                       # noqa: E402
from ldm.models.diffusion.dpm_solver import DPMSolverSampler            # noqa: E402
from ldm.models.diffusion.plms import PLMSSampler                       # noqa: E402
from ldm.modules.attention import ContextMaps                           # noqa: E402

B, K, S, GRID = 2, 3, 6, (16, 16)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(20240611)
    c3 = torch.randn(B, K, cases.UNET_NARROW["context_dim"], generator=g)
    regions = (torch.rand(B, K, *GRID, generator=g) > 0.4).double()
    regions[:, 0, :8] = 0.0                                             # token 0 absent from the upper half
    regions[:, 1:, 12:, 12:] = 0.0                                      # a corner only token 0 covers
    common = dict(batch_size=B, shape=[4, *GRID], verbose=False, unconditional_guidance_scale=5.0,
                  test_model_kwargs={"inpaint_image": torch.randn(B, 4, *GRID, generator=g).to(dev),
                                     "inpaint_mask": (torch.rand(B, 1, *GRID, generator=g) > 0.5).float().to(dev)})
    x_T = torch.randn(B, 4, *GRID, generator=g)
    samplers = {"plms": (PLMSSampler, dict(eta=0.0)), "ddim-eta0": (DDIMSampler, dict(eta=0.0)),
                "ddim-eta0.5-seeds": (DDIMSampler, dict(eta=0.5, seeds=[11, 2 ** 40 + 12])), "dpm-order2": (DPMSolverSampler, dict(order=2))}
    conds = {"k1": lambda: dict(conditioning=c3[:, :1]),
             "k3-weights": lambda: dict(conditioning=c3, conditioning_weights=[[2.0, 1.0, 0.0], [0.5, 0.0, 1.0]]),
             "k3-regions": lambda: dict(conditioning=c3, conditioning_regions=regions),
             "k3-regions-maps": lambda: dict(conditioning=c3, conditioning_regions=regions, conditioning_maps=ContextMaps())}
    modes = {"eager-paired": dict(), "eager-unshared": dict(share_guidance_prefix=False), "graph": dict(use_graph=True)}
    with torch.no_grad():
        model = modelbuild.narrow_model(dev)
        for sname, (cls, skw) in samplers.items():
            for cname, ckw in conds.items():
                for mname, attrs in modes.items():
                    smp = cls(model)
                    smp.use_graph = False
                    for k, v in attrs.items():
                        setattr(smp, k, v)
                    kw = dict(common, **skw, **ckw())
                    if "seeds" not in kw:
                        kw["x_T"] = x_T.clone().to(dev)
                    z, _ = smp.sample(S=S, unconditional_conditioning=model.learnable_vector, **kw)
                    row = f"{sname:18s} {cname:16s} {mname:15s} latent {sha(z)}"
                    cm = kw.get("conditioning_maps")
                    if cm is not None:
                        row += f"  maps {sha(cm.result(GRID))}  counts {sorted(cm.counts().items())}"
                    print(row, flush=True)


if __name__ == "__main__":
    main()
