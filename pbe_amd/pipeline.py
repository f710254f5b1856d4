"""End-to-end inpainting pass = the call order of scripts/inference.py:323-348 in zhanwenchen/pbe:
CLIP exemplar -> proj_out -> VAE encode of the masked image (posterior sample x 0.18215) ->
mask resize to the latent grid -> PLMS / DDIM sampling under classifier-free guidance ->
VAE decode -> clamp((x+1)/2, 0, 1).  Inputs are already pre-processed tensors
(pbe_amd.preprocess), outputs fp32 NCHW in [0,1]."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .lib import PbeError


def pad_conditionings(conds: Sequence[torch.Tensor], weights: Optional[Sequence] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A ragged batch of conditionings -> one padded context and its exemplar weights.  conds: per sample a tensor [k_i, D] (k_i >= 1
    exemplar tokens, one D and device for all); weights: per sample k_i non-negative weights, default ones.  Returns (context
    [B, K_max, D] in the dtype / on the device of conds[0], weights fp64 [B, K_max] on the host): the padding rows are COPIES of the
    sample's first token (finite, never uninitialised memory) and carry weight 0, which removes them from the softmax - pass the pair
    as conditioning / conditioning_weights to the samplers, or as context / context_weights to the U-Net."""
    if len(conds) == 0:
        raise PbeError("pad_conditionings: no conditionings")
    if any((not isinstance(c, torch.Tensor)) or c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != conds[0].shape[1] for c in conds):
        raise PbeError("pad_conditionings: every conditioning must be a [k_i >= 1, D] tensor with one D")
    if weights is not None and len(weights) != len(conds):
        raise PbeError(f"pad_conditionings: {len(weights)} weight rows for {len(conds)} conditionings")
    B, K = len(conds), max(int(c.shape[0]) for c in conds)
    ctx = torch.empty((B, K, conds[0].shape[1]), dtype=conds[0].dtype, device=conds[0].device)
    w = torch.zeros((B, K), dtype=torch.float64)
    for i, c in enumerate(conds):
        k = int(c.shape[0])
        ctx[i, :k] = c
        ctx[i, k:] = c[0]
        wi = torch.ones(k, dtype=torch.float64) if weights is None else torch.as_tensor(weights[i]).detach().to("cpu", torch.float64).reshape(-1)
        if wi.numel() != k:
            raise PbeError(f"pad_conditionings: sample {i} has {k} tokens and {wi.numel()} weights")
        if not bool(torch.isfinite(wi).all()) or bool((wi < 0).any()) or not float(wi.sum()) > 0.0:
            raise PbeError(f"pad_conditionings: the weights of sample {i} must be finite, >= 0 and have a positive sum")
        w[i, :k] = wi
    return ctx, w


def pad_regions(regions: Sequence, K_max: int) -> torch.Tensor:
    """The region maps of a ragged batch -> one padded tensor: regions holds per sample a [k_i, Hr, Wr] tensor (1 <= k_i <= K_max maps
    >= 0, one Hr x Wr for all), the result is fp64 [B, K_max, Hr, Wr] on the host with ZEROS on the padding tokens (absent everywhere,
    as their weight 0 from pad_conditionings already makes them) - pass it as conditioning_regions / context_regions beside the pair
    pad_conditionings returns."""
    if len(regions) == 0:
        raise PbeError("pad_regions: no regions")
    rs = [torch.as_tensor(r).detach().to("cpu", torch.float64) for r in regions]
    if any(r.dim() != 3 or r.shape[0] < 1 or r.shape[0] > K_max or tuple(r.shape[1:]) != tuple(rs[0].shape[1:]) for r in rs):
        raise PbeError(f"pad_regions: every sample needs a [k_i, Hr, Wr] tensor with 1 <= k_i <= {K_max} and one Hr x Wr")
    out = torch.zeros((len(rs), int(K_max), *rs[0].shape[1:]), dtype=torch.float64)
    for i, r in enumerate(rs):
        out[i, :r.shape[0]] = r
    return out


def resize_mask(mask: torch.Tensor, size, antialias: bool = True) -> torch.Tensor:
    """scripts/inference.py:332 ``Resize([h, w])(mask)``: bilinear, align_corners=False; the
    antialias default differs across torchvision versions -> exposed, default True.
    Pre-processing, once per image: the HIP kernel pbe_resize_bilinear_f32 (no torch fallback)."""
    return ops.resize_bilinear(mask.float(), size, antialias)


@torch.no_grad()
def inpaint(model, image: torch.Tensor, mask: torch.Tensor, ref: torch.Tensor, *, steps: int = 50, scale: float = 5.0,
            x_T: Optional[torch.Tensor] = None, post_eps: Optional[torch.Tensor] = None, sampler: str = "plms",
            antialias: bool = True, timings: Optional[Dict[str, float]] = None, ref_weights=None, ref_regions=None,
            return_ref_maps: bool = False, seeds=None, seed_sub=None) -> Dict[str, torch.Tensor]:
    """image [B,3,H,W] in [-1,1], mask [B,1,H,W] in {0,1} (1 = keep), ref [B,3,224,224] CLIP-normalised (or [B,K,3,224,224]: K
    exemplars per sample, with ref_weights [B, K] their non-negative weights or None and ref_regions [B, K, Hr, Wr] >= 0 where each of
    them applies - 1 = fully, 0 = not there; the latent grid and its halvings down to the coarsest attention level must divide
    Hr x Wr - or None); everything on the model's GPU.  Returns {'image' [B,3,H,W] in [0,1], 'latent', 'c', 'z_inpaint', 'mask_lat'}.
    sampler: "plms" (S + 1 U-Net calls), "dpm" (DPM-Solver++(2M), `steps` calls: about 20 do where the others take 50) or anything else: DDIM.
    return_ref_maps: also 'ref_maps' fp32 [B, K, h, w] on the latent grid - the share of cross-attention each exemplar received at each
    position, averaged over heads, blocks, sampler steps and levels (ldm.modules.attention.ContextMaps; K = 1: ones).  Collecting them
    sends every level through the fused cross-attention kernel: with ref_regions the picture is the one without return_ref_maps bit for
    bit; without regions (and K > 1) it is the picture of blocks with ctx_fused_max_width = 1280, within the sampler tolerance of the default.
    seeds: one noise seed per sample (an int64 tensor [B] on the GPU or ints in [0, 2^64)), seed_sub their substreams (int32 [B] / ints
    in [0, 2^31)) or None.  Then every draw of the call is made on the device by pbe_amd.noise (its docstring is the stream plan): the
    posterior noise from STREAM_POST_EPS - no CPU draw, no upload -, x_T and the samplers' own draws from the sampler's SeededNoise;
    sample i is a function of (seeds[i], seed_sub[i]) alone, whatever B is.  x_T and post_eps must then be None; the result gains 'seeds'
    (the int64 tensor).  Without seeds nothing changes: the draws are torch's, as in the reference."""
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.plms import PLMSSampler
    dev = model.device
    image, mask, ref = image.to(dev).float(), mask.to(dev).float(), ref.to(dev).float()
    B = image.shape[0]
    if seeds is None and seed_sub is not None:
        raise PbeError("inpaint: seed_sub names substreams of seeds, which are missing")
    if seeds is not None:
        if x_T is not None or post_eps is not None:
            raise PbeError("inpaint: seeds given together with x_T / post_eps - the noise is either drawn from the seeds or handed in")
        seeds, seed_sub = ops.seed_tensor(seeds, B, dev), ops.sub_tensor(seed_sub, B, dev)
    ev = None
    if timings is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
    c = model.proj_out(model.get_learned_conditioning(ref))                              # inference.py:326-327
    uc = model.learnable_vector if scale != 1.0 else None                                # inference.py:323-325
    if ev:
        ev[1].record()
    post = model.encode_first_stage(image * mask)                                        # inference.py:319,330
    if seeds is not None and hasattr(post, "parameters") and not post.deterministic:
        from .noise import SeededNoise
        pb, ph, pw, _ = post.parameters.shape
        post_eps = SeededNoise(seeds, seed_sub).post_eps((pb, post.z, ph, pw))
    z_inp = model.get_first_stage_encoding(post, noise=post_eps)                         # inference.py:331
    m_lat = resize_mask(mask, z_inp.shape[-2:], antialias)                               # inference.py:332
    if ev:
        ev[2].record()
    if sampler == "dpm":                                                                 # DPM-Solver++(2M): `steps` U-Net calls
        from ldm.models.diffusion.dpm_solver import DPMSolverSampler
        smp = DPMSolverSampler(model)
    else:
        smp = (PLMSSampler if sampler == "plms" else DDIMSampler)(model)
    more = {} if seeds is None else {"seeds": seeds, "seed_sub": seed_sub}
    cm = None
    if return_ref_maps:
        from ldm.modules.attention import ContextMaps
        cm = ContextMaps()
    z0, _ = smp.sample(S=steps, batch_size=B, shape=list(z_inp.shape[1:]), conditioning=c, verbose=False,
                       unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=0.0, x_T=x_T,
                       test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": m_lat}, conditioning_weights=ref_weights,
                       conditioning_regions=ref_regions, conditioning_maps=cm, **more)
    if ev:
        ev[3].record()
    img = ops.image_post(model.decode_first_stage_nhwc(z0))                              # inference.py:346-347
    if ev:
        ev[4].record()
        torch.cuda.synchronize()
        for k, i in (("clip_ms", 0), ("vae_encode_ms", 1), ("sampler_ms", 2), ("vae_decode_ms", 3)):
            timings[k] = timings.get(k, 0.0) + ev[i].elapsed_time(ev[i + 1])
    out = {"image": img, "latent": z0, "c": c, "z_inpaint": z_inp, "mask_lat": m_lat}
    if cm is not None:
        out["ref_maps"] = cm.result(z_inp.shape[-2:])
    if seeds is not None:
        out["seeds"] = seeds
    return out


def window_inputs(pictures: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], windows: Sequence, size) -> Dict[str, torch.Tensor]:
    """The stacked model inputs of inpaint_window: {'image' [B,3,H,W] in [-1,1], 'mask' [B,1,H,W] in {0,1}, 'inpaint' = image * mask},
    sample i from windows[i] of pictures[i] / masks[i] (ops.window_image, ops.window_mask, ops.mul_planes: HIP kernels only)."""
    B, (H, W), dev = len(pictures), (int(size[0]), int(size[1])), pictures[0].device
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    for i in range(B):
        ops.window_image(pictures[i], windows[i], (H, W), out=image[i])
        ops.window_mask(masks[i], windows[i], (H, W), out=mask[i])
    return {"image": image, "mask": mask, "inpaint": ops.mul_planes(image, mask)}


@torch.no_grad()
def inpaint_window(model, pictures: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], ref: torch.Tensor, *, size=(512, 512), context=0.5,
                   feather: int = 8, windows: Optional[Sequence] = None, mask_shape: Optional[dict] = None, tone: Optional[str] = None, tone_margin: int = 8,
                   tone_gain_limit: float = 1.25, tone_cell: int = 8, tone_field_limit: float = 0.125, **inpaint_kwargs) -> Dict[str, object]:
    """Inpaint a region of pictures of any size and paste it back in place.  pictures: per sample a uint8 [Hs, Ws, 3] tensor, masks: a
    uint8 [Hs, Ws] tensor of the same Hs x Ws (a byte >= 128 is the hole), both contiguous and on the model's GPU; the sizes may differ
    from sample to sample.  Per sample ONE window is planned around the hole (pbe_amd.window.plan_window with `size`, `context`,
    `feather`; or windows[i] = (y0, x0, wh, ww), validated), brought to the working size `size` = (H, W) (ops.window_image /
    ops.window_mask), and the stacked batch goes through the unchanged `inpaint`, which receives **inpaint_kwargs as they are (steps,
    scale, sampler, x_T, post_eps, ref_weights, ref_regions, return_ref_maps ...).  The result is resampled to the window and blended
    into a CLONE of each picture under alpha = ops.feather_alpha(mask, window, feather) by ops.paste_window: every byte with
    alpha == 0 - all of the picture farther than 2 feather from the hole - keeps its value, and with the planner's margin alpha is 0 on
    every window border inside the picture, so no seam shows.
    Returns inpaint's dict ('image', 'latent', ... at the working size) plus 'pictures' (list of uint8 [Hs, Ws, 3]), 'windows' (list of
    (y0, x0, wh, ww)), 'alphas' (list of fp32 [wh, ww]) and 'inputs' (window_inputs: what the model saw).  ref_regions and 'ref_maps' stay
    on the WINDOW's grid: a region map describes the window at the working size, not the picture, and the attribution maps come back on
    the window's latent grid.
    mask_shape: a dict of pbe_amd.window.shape_mask's keywords (open, close, grow, box, connectivity).  Each mask is then shaped once, on
    the device, and the shaped mask is THE mask from there on - planning, what the model sees, the blend - and the result gains 'masks',
    the list of shaped uint8 masks.  None (the default) takes the masks as they are.
    tone: "mean" or "affine" matches the pasted window's tone to the picture around the hole (match_tone below): each window is pasted
    through its own per-channel map gain * res + offset, and the result gains 'tone' (pbe_amd.window.fit_tone's list) and 'tone_stats'
    (the int64 [B, 3, 6] table).  'image' stays the uncorrected working-size result.  None (the default) adds no key and no launch.
    tone="field" follows a tone that varies across the window (match_tone_field below): each window is pasted with its own low-frequency
    difference field added, at `tone_cell` working pixels per cell, the cell means clamped to +-`tone_field_limit`.  The result gains 'tone'
    (pbe_amd.window.tone_field's summary list), 'tone_field' (fp32 [B, 3, Hc, Wc]) and 'tone_cells' (int32 [B, 4, Hc, Wc]), and no
    'tone_stats'.  tone_margin means what it means for the other modes; tone_gain_limit is ignored (the field is additive, gain 1)."""
    from . import window as _w
    B = len(pictures)
    shape = None if mask_shape is None else _w.shape_args(mask_shape)
    _check_tone("inpaint_window", tone)
    if B == 0 or len(masks) != B or (windows is not None and len(windows) != B):
        raise PbeError(f"inpaint_window: {B} pictures, {len(masks)} masks" + ("" if windows is None else f", {len(windows)} windows"))
    for i, (p, m) in enumerate(zip(pictures, masks)):
        if not isinstance(p, torch.Tensor) or not isinstance(m, torch.Tensor) or p.dim() != 3 or m.dim() != 2 or tuple(p.shape[:2]) != tuple(m.shape):
            raise PbeError(f"inpaint_window: sample {i} needs a uint8 [Hs, Ws, 3] picture and a uint8 [Hs, Ws] mask of one size")
    if shape is not None:
        masks = [_w.shape_mask(m, **shape) for m in masks]
    wins = [_w.plan_window(masks[i], size, context, feather, None if windows is None else windows[i]) for i in range(B)]
    inputs = window_inputs(pictures, masks, wins, size)
    out: Dict[str, object] = dict(inpaint(model, inputs["image"], inputs["mask"], ref, **inpaint_kwargs))
    alphas = [ops.feather_alpha(masks[i], wins[i], feather) for i in range(B)]
    result = out["image"].float().contiguous()
    maps = [{}] * B                                       # tone=None: the call it always was
    if tone == "field":
        out["tone"], out["tone_field"], out["tone_cells"] = match_tone_field(inputs["image"], result, masks, wins, size, tone_margin, tone_cell, tone_field_limit)
        maps = [{"field": out["tone_field"][i], "cell": tone_cell} for i in range(B)]
    elif tone is not None:
        out["tone"], out["tone_stats"] = match_tone(inputs["image"], result, masks, wins, size, tone, tone_margin, tone_gain_limit)
        maps = [{"tone": (f["gain"], f["offset"])} for f in out["tone"]]
    out["pictures"] = [ops.paste_window(result[i], alphas[i], pictures[i].clone(), wins[i], **maps[i]) for i in range(B)]
    out["windows"], out["alphas"], out["inputs"] = wins, alphas, inputs
    if shape is not None:
        out["masks"] = list(masks)
    return out


TONE_MODES = ("mean", "affine", "field")


def _check_tone(what: str, tone) -> None:
    if tone is not None and tone not in TONE_MODES:
        raise PbeError(f"{what}: tone must be None or one of {TONE_MODES}, got {tone!r}")


def match_tone(image: torch.Tensor, result: torch.Tensor, masks: Sequence[torch.Tensor], windows: Sequence, size, mode: str = "affine",
               margin: int = 8, gain_limit: float = 1.25):
    """The tone maps of a batch of windows: (pbe_amd.window.fit_tone's list, the int64 [B, 3, 6] table on the device).  image [B, 3, H, W]
    is what the model saw (window_inputs' 'image'), result [B, 3, H, W] what it returned (inpaint's 'image'), masks[i] / windows[i] the
    uint8 mask and the window of sample i.  sel = pbe_amd.window.tone_selection per window, stacked; ONE ops.tone_stats over the batch,
    one host read of the table, the fit on the host.  Known pixels come back from the autoencoder with a brightness and contrast of their
    own per channel; the map brings them back onto the original's, and the paste applies it to the whole window, hole included."""
    from . import window as _w
    _check_tone("match_tone", mode)
    if mode == "field":
        raise PbeError("match_tone: mode 'field' has no map per window: match_tone_field makes the difference field")
    B, (H, W) = len(windows), (int(size[0]), int(size[1]))
    sel = torch.empty((B, 1, H, W), dtype=torch.float32, device=image.device)
    for i in range(B):
        _w.tone_selection(masks[i], windows[i], (H, W), margin, out=sel[i])
    stats = ops.tone_stats(image.contiguous(), result.contiguous(), sel)
    return _w.fit_tone(stats.cpu(), mode, gain_limit), stats


def match_tone_field(image: torch.Tensor, result: torch.Tensor, masks: Sequence[torch.Tensor], windows: Sequence, size, margin: int = 8, cell: int = 8,
                     limit: float = 0.125):
    """The difference fields of a batch of windows: pbe_amd.window.tone_field's (summary list, field fp32 [B, 3, Hc, Wc], cells int32
    [B, 4, Hc, Wc]) over the selection match_tone takes (pbe_amd.window.tone_selection per window, stacked).  One ops.tone_cells and one
    ops.tone_field over the batch, one small host read for the summary."""
    from . import window as _w
    B, (H, W) = len(windows), (int(size[0]), int(size[1]))
    sel = torch.empty((B, 1, H, W), dtype=torch.float32, device=image.device)
    for i in range(B):
        _w.tone_selection(masks[i], windows[i], (H, W), margin, out=sel[i])
    field, cells, summary = _w.tone_field(image.contiguous(), result.contiguous(), sel, cell, limit)
    return summary, field, cells


PER_WINDOW_KWARGS = ("x_T", "post_eps", "ref_weights", "ref_regions", "seeds", "seed_sub")       # the arguments of inpaint with a leading batch dimension


@torch.no_grad()
def inpaint_holes(model, pictures: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], ref: torch.Tensor, *, size=(512, 512), context=0.5,
                  feather: int = 8, connectivity: int = 8, max_holes: int = 16, batch: Optional[int] = None, mask_shape: Optional[dict] = None,
                  tone: Optional[str] = None, tone_margin: int = 8, tone_gain_limit: float = 1.25, tone_cell: int = 8, tone_field_limit: float = 0.125,
                  hole_seeds: Optional[Dict[int, int]] = None, **inpaint_kwargs) -> Dict[str, object]:
    """Inpaint every hole of a picture in a window of its own and paste them all back into one picture.  pictures / masks: as in
    inpaint_window (B samples).  Per sample the mask is labelled on the device (ops.mask_components at `connectivity`), the component
    boxes come back in one small read (ops.component_boxes) and pbe_amd.window.plan_holes groups the components whose blend zones could
    touch and plans one window per group: N windows over the B samples, ordered by sample, then by the raster order of each group's
    first pixel.  More than `max_holes` groups in a sample, or a mask without a hole, raise PbeError.

    DECISION: window g is built from g's OWN mask, ops.select_components of g's labels - both what the model sees (ops.window_mask) and
    the blend (ops.feather_alpha).  Another group's hole that falls into g's window shows its original pixels there and is not blended
    by g: each hole is edited as if it were the only one.  Groups lie farther apart than 4 feather + 2, so their alpha supports are
    disjoint and the order of pasting does not matter.

    ref: [B, ...] (each sample's exemplars serve all its holes) or [N, ...] (one per window); where B == N that is the same thing.  The
    per-window arguments of inpaint (x_T, post_eps, ref_weights, ref_regions) have leading size N.  The windows go through the unchanged
    `inpaint` in chunks of at most `batch` (default: all N at once); everything else in **inpaint_kwargs passes as it is.
    Returns inpaint's tensors concatenated over the chunks, plus 'pictures' (per sample a uint8 [Hs, Ws, 3] clone with every hole pasted),
    'holes' (per window a dict: 'sample', 'labels', 'box' (ya, yb, xa, xb), 'window' (y0, x0, wh, ww), 'area' in pixels), 'alphas' (per
    window fp32 [wh, ww]) and 'inputs' (window_inputs over the N windows).
    mask_shape: as in inpaint_window - each mask is shaped once (pbe_amd.window.shape_mask) before it is labelled, the holes are those
    of the shaped mask, and the result gains 'masks'.  `connectivity` here is the labelling's; the box stage has its own key.
    seeds (through **inpaint_kwargs): B noise seeds, one per PICTURE - window g then draws with its picture's seed and sub = the raster
    index of its group's first pixel + 1 (min(holes[g]['labels']) + 1: the labels of csrc/holes.hip), so a hole's noise is a function of
    (picture seed, where the hole starts) and does not change with the other holes, with `batch` or with `max_holes` - or N seeds, one
    per window, with sub = 0 (where B == N the seeds count per picture).  hole_seeds {g: seed} then gives window g a seed of its own with
    sub = 0 - one hole re-rolled, the others keep their noise.  seed_sub is not an argument here.  Each holes[g] gains 'seed' and 'sub',
    and the result 'seeds' as from inpaint.
    tone: as in inpaint_window, one map (or, with "field", one difference field: tone_cell, tone_field_limit) per WINDOW ('tone' and
    'tone_stats', or 'tone_field' and 'tone_cells', have N entries / rows, concatenated over the chunks; "field" ignores
    tone_gain_limit).  The selection comes from each window's OWN mask, as alpha does: another group's hole inside the window was a known pixel for the model
    and counts as one."""
    from . import window as _w
    B = len(pictures)
    shape = None if mask_shape is None else _w.shape_args(mask_shape)
    _check_tone("inpaint_holes", tone)
    if B == 0 or len(masks) != B:
        raise PbeError(f"inpaint_holes: {B} pictures, {len(masks)} masks")
    for i, (p, m) in enumerate(zip(pictures, masks)):
        if not isinstance(p, torch.Tensor) or not isinstance(m, torch.Tensor) or p.dim() != 3 or m.dim() != 2 or tuple(p.shape[:2]) != tuple(m.shape):
            raise PbeError(f"inpaint_holes: sample {i} needs a uint8 [Hs, Ws, 3] picture and a uint8 [Hs, Ws] mask of one size")
    if shape is not None:
        masks = [_w.shape_mask(m, **shape) for m in masks]
    holes, own_masks = [], []
    for i in range(B):
        labels = ops.mask_components(masks[i], connectivity)
        _, table = ops.component_boxes(labels)
        area = {int(row[0]): int(row[5]) for row in table}
        for ls, box, win in _w.plan_holes(table, masks[i].shape, size, context, feather, max_holes):
            holes.append({"sample": i, "labels": ls, "box": box, "window": win, "area": sum(area[l] for l in ls)})
            own_masks.append(ops.select_components(labels, ls))
    N = len(holes)
    lead = int(ref.shape[0])
    if lead == B:
        ref = ref if N == B and all(h["sample"] == k for k, h in enumerate(holes)) else ref[[h["sample"] for h in holes]]
    elif lead != N:
        raise PbeError(f"inpaint_holes: ref has leading size {lead}; expected {B} (one per sample) or {N} (one per hole)")
    if inpaint_kwargs.get("seed_sub") is not None:
        raise PbeError("inpaint_holes: seed_sub is derived from the holes (one seed per picture) or 0 (one seed per hole); do not pass it")
    if hole_seeds and inpaint_kwargs.get("seeds") is None:
        raise PbeError("inpaint_holes: hole_seeds overrides single holes of a seeded run; seeds is missing")
    if inpaint_kwargs.get("seeds") is not None:
        inpaint_kwargs = dict(inpaint_kwargs)
        sd = inpaint_kwargs["seeds"]
        sd = ops.seed_tensor(sd, None).tolist() if isinstance(sd, torch.Tensor) else ops.seed_words(sd)      # the int64 values (one small read)
        if len(sd) == B:
            sd, subs = [sd[h["sample"]] for h in holes], [min(h["labels"]) + 1 for h in holes]
        elif len(sd) == N:
            subs = [0] * N
        else:
            raise PbeError(f"inpaint_holes: {len(sd)} seeds; expected {B} (one per picture) or {N} (one per hole)")
        for g, s_ in (hole_seeds or {}).items():
            if isinstance(g, bool) or not isinstance(g, int) or not 0 <= g < N:
                raise PbeError(f"inpaint_holes: hole_seeds names hole {g!r}; the mask has holes 0 .. {N - 1}")
            sd[g], subs[g] = ops.seed_words([s_])[0], 0
        for h, s_, u_ in zip(holes, sd, subs):
            h["seed"], h["sub"] = s_ & ((1 << 64) - 1), u_
        dev = pictures[0].device
        inpaint_kwargs["seeds"] = torch.tensor(sd, dtype=torch.int64, device=dev)
        inpaint_kwargs["seed_sub"] = torch.tensor(subs, dtype=torch.int32, device=dev)
    for k in PER_WINDOW_KWARGS:
        v = inpaint_kwargs.get(k)
        if v is not None and len(v) != N:
            raise PbeError(f"inpaint_holes: {k} has leading size {len(v)}, expected {N} (one per hole)")
    step = N if batch is None else int(batch)
    if step < 1:
        raise PbeError(f"inpaint_holes: batch {batch!r} must be a positive integer")
    wins = [h["window"] for h in holes]
    inputs = window_inputs([pictures[h["sample"]] for h in holes], own_masks, wins, size)
    chunks = []
    for a in range(0, N, step):
        kw = {k: (v[a:a + step] if k in PER_WINDOW_KWARGS and v is not None else v) for k, v in inpaint_kwargs.items()}
        chunks.append(inpaint(model, inputs["image"][a:a + step], inputs["mask"][a:a + step], ref[a:a + step], **kw))
    out: Dict[str, object] = {k: (torch.cat([c[k] for c in chunks]) if len(chunks) > 1 else chunks[0][k]) for k in chunks[0]}
    alphas = [ops.feather_alpha(own_masks[n], wins[n], feather) for n in range(N)]
    result = out["image"].float().contiguous()
    pasted = [p.clone() for p in pictures]
    maps = [{}] * N                                       # tone=None: the call it always was
    if tone == "field":
        out["tone"], out["tone_field"], out["tone_cells"] = match_tone_field(inputs["image"], result, own_masks, wins, size, tone_margin, tone_cell, tone_field_limit)
        maps = [{"field": out["tone_field"][n], "cell": tone_cell} for n in range(N)]
    elif tone is not None:
        out["tone"], out["tone_stats"] = match_tone(inputs["image"], result, own_masks, wins, size, tone, tone_margin, tone_gain_limit)
        maps = [{"tone": (f["gain"], f["offset"])} for f in out["tone"]]
    for n, h in enumerate(holes):
        ops.paste_window(result[n], alphas[n], pasted[h["sample"]], wins[n], **maps[n])
    out["pictures"], out["holes"], out["alphas"], out["inputs"] = pasted, holes, alphas, inputs
    if shape is not None:
        out["masks"] = list(masks)
    return out


def ref_maps_u8(ref_maps: torch.Tensor, size, antialias: bool = True) -> torch.Tensor:
    """Attribution maps fp32 [B, K, h, w] in [0, 1] -> uint8 [B, K, H, W] at the picture size `size` = (H, W): resized on the device
    (pbe_resize_bilinear_f32, as the mask is) and quantised as round(255 * map).  What --save_reference_maps writes, one PNG per plane."""
    B, K, h, w = ref_maps.shape
    big = ops.resize_bilinear(ref_maps.float().reshape(B * K, 1, h, w).contiguous(), size, antialias)
    return (big * 255.0).round_().clamp_(0.0, 255.0).to(torch.uint8).view(B, K, int(size[0]), int(size[1]))
