#!/usr/bin/env python3
"""Single-triple inpainting CLI — counterpart of scripts/inference.py:127-402 in zhanwenchen/pbe with
the same flags and defaults, the same call order (CLIP -> proj_out -> VAE encode -> mask resize ->
sampler -> decode -> clamp) and the same output tree, running on the MI355X HIP path.

    python scripts/inference.py --plms --outdir results --config configs/v1.yaml --ckpt checkpoints/model.ckpt \
        --image_path examples/image/example_1.png --mask_path examples/mask/example_1.png \
        --reference_path examples/reference/example_1.jpg --seed 321 --scale 5

`--dpm_solver` (upstream Stable Diffusion's flag, not in the reference; excludes `--plms`) samples with DPM-Solver++(2M): `--ddim_steps`
U-Net calls, so `--ddim_steps 20` is 20 calls where `--plms` makes 51 at its default.
`--reference_path` may name several images (not in the reference): each becomes one context token of the sample.
`--reference_weight w1 w2 ...` gives each of them a non-negative weight (default: all 1): its share of the cross-attention is
proportional to w exp(score), so `2 1` equals naming the first image twice and `1 0` equals naming the first image alone.
`--reference_region a.png b.png` gives each of them a grayscale image of where it applies (white = there, black = not there; grey
in between): it is resized to the latent grid and every position of the picture attends to the exemplars whose region covers it,
weighted by region x weight; a position that no region covers blends them by their weights alone.
`--save_reference_maps` writes, beside the result, one 8-bit grayscale PNG per reference into `<outdir>/reference_maps/`, named after
the result file with `_ref<j>`: the share of cross-attention that reference received at each position of the picture (white = all of
it), averaged over heads, blocks, sampler steps and levels - whether a region "took", which exemplar wins where.
`--paste_back` (not in the reference) lets `--image_path` / `--mask_path` be a picture of ANY size: one window around the hole (the
hole's box plus `--context` of its size and the feather's width on each side, at the aspect of `--H` x `--W`, never smaller than
`--H` x `--W` where the picture allows) is brought to `--H` x `--W` on the device and goes through the model; `source/`, `results/`
and `grid/` show that window as before, and `pasted/<stem>_<seed>.png` is the whole picture with the result blended in under a mask
feathered over `--feather` pixels (default 8): every pixel farther than 2 x feather from the hole keeps its bytes.  `--reference_region`
images are then picture-sized and cropped to the window; the attribution maps stay on the window.
`--per_hole` (with `--paste_back`; not in the reference) gives every hole of the mask a window of its own (pipeline.inpaint_holes: the
mask's connected components, grouped where their blend zones could touch; each window sees its own hole alone) and
`pasted/<stem>_<seed>.png` holds all of them; `source/`, `results/` and `grid/` get one set of files per hole, named
`<stem>_hole<i>_<seed>...`, holes in raster order of their first pixel.  With `--reference_per_hole` the i-th `--reference_path` is the
exemplar of the i-th hole (as many paths as holes); without it every hole gets all of them.  The start code (with `--fixed_code`) and the
posterior noise of the windows come from generators seeded with `--seed`, so a run is reproducible from its arguments.
`--mask_open PX`, `--mask_close PX`, `--mask_grow PX` and `--mask_box` (not in the reference) shape the mask on the device before anything
else sees it (pbe_amd.window.shape_mask, in that order): open removes specks narrower than a disc of radius PX, close fills gaps narrower
than it, grow grows the hole by that disc (a negative PX shrinks it), box replaces every hole by its bounding box.  They work with and
without `--paste_back` / `--per_hole`; `source/<stem>_<seed>_mask.png` then shows the shaped mask.
`--match_tone {mean,affine}` (with `--paste_back`, with or without `--per_hole`; not in the reference) matches the pasted window's tone
to the picture around the hole: per window and channel an offset (`mean`) or a gain and an offset (`affine`) is fitted on the known
pixels farther than `--tone_margin PX` (default 8) working pixels from the hole, so that the result's known pixels fall back onto the
original's, and the whole window is pasted through that map.  A line per window reports gains, offsets, the rms difference before and
after in grey levels and the pixel count; `pasted/<stem>_<seed>.tone.json` holds the same (pbe_amd.window.fit_tone's list).  `results/`
keeps the uncorrected window.  `--match_tone field` follows a tone that VARIES across the window (a vignette, a gradient the decoder
flattens): the difference between the original's and the result's known pixels is summed per cell of `--tone_cell PX` (4, 8, 16, 32 or
64; default 8) working pixels, filled in over the hole by a pull-push pyramid, clamped to +-`--tone_field_limit V` (default 0.125 of
full scale) and added to the pasted window.  The line per window reports the pixel count, the grid and the field's range in grey
levels; the `.tone.json` holds pbe_amd.window.tone_field's summary.
`--reference_on_device` (not in the reference) cuts the exemplar on the device: PIL only decodes `--reference_path`, its full-size bytes
travel, and Pillow's own resize to 224 x 224 runs as HIP kernels (pbe_amd.exemplar) - the picture is the default path's bit for bit.
`--reference_box X0 Y0 X1 Y1` (four numbers per `--reference_path`, Pillow's box, fractions allowed) takes that part of the reference as
the exemplar; `--reference_mask PATH ...` (one per reference, of its size, white = the object) takes the object's bounding box instead;
`--reference_pad F` grows the box by F of its size on each side, `--reference_square` makes it square about its centre (both inside
the picture: shifted at a border, not shrunk), `--reference_fill R G B` (with `--reference_mask`) paints everything off the object in that
colour before the resize.  Any of them implies the device path.  The cut exemplars are written to
`<outdir>/reference_crops/<stem>_ref<k>.png`.  All of it works with several references, `--reference_per_hole`, `--paste_back` and every
sampler.

`--seeds S [S ...]` (not in the reference) makes every picture a function of its own seed: all noise - the start code, the posterior
noise, the samplers' own draws - comes from pbe_amd.noise (Philox4x32-10 keyed by the seed, drawn on the device), so a seed gives the
same noise in any batch, on any device and with any torch.  A plain or `--paste_back` run becomes ONE batch with one variant of the
triple per seed and writes the usual output tree once per seed, that seed in every file name.  With `--per_hole` each seed is one
pipeline.inpaint_holes call with it as the picture's seed: a hole's noise is then a function of (seed, where the hole starts), and
`--hole_seed INDEX SEED` (repeatable) re-rolls hole INDEX alone - the others keep their noise; a line per hole prints its (seed, sub).
`--seeds` excludes `--fixed_code` and `--n_samples` above 1; `--seed` still seeds torch's generators and nothing else.
Without `--seeds` every run writes the files it always wrote.

Differences, all deliberate: the safety checker and the invisible watermark are dropped (the
reference overwrites the checker's result, :350-351; both need hub downloads); `--ckpt ""` or
`--random_weights` runs with name-seeded random weights (no checkpoint exists offline);
`--precision` is accepted for compatibility (the HIP path is always fp16 storage / fp32 accumulate).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--outdir", type=str, nargs="?", default="outputs/txt2img-samples")
    p.add_argument("--skip_grid", action="store_true")
    p.add_argument("--skip_save", action="store_true")
    p.add_argument("--ddim_steps", type=int, default=50)
    p.add_argument("--plms", action="store_true")
    p.add_argument("--dpm_solver", action="store_true", help="(upstream Stable Diffusion's flag, not in the reference) sample with "
                   "DPM-Solver++(2M): --ddim_steps U-Net calls, about 20 where PLMS / DDIM take 50; excludes --plms")
    p.add_argument("--fixed_code", action="store_true")
    p.add_argument("--ddim_eta", type=float, default=0.0)
    p.add_argument("--n_iter", type=int, default=2)
    p.add_argument("--H", type=int, default=512)
    p.add_argument("--W", type=int, default=512)
    p.add_argument("--n_imgs", type=int, default=100)
    p.add_argument("--C", type=int, default=4)
    p.add_argument("--f", type=int, default=8)
    p.add_argument("--n_samples", type=int, default=1)
    p.add_argument("--n_rows", type=int, default=0)
    p.add_argument("--scale", type=float, default=1)
    p.add_argument("--config", type=str, default="")
    p.add_argument("--ckpt", type=str, default="")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--precision", type=str, choices=["full", "autocast"], default="autocast")
    p.add_argument("--image_path", type=str, default="")
    p.add_argument("--mask_path", type=str, default="")
    p.add_argument("--reference_path", type=str, nargs="+", default=[""], help="one exemplar image as in the reference, or several: they "
                   "become the context tokens of the sample")
    p.add_argument("--reference_weight", type=float, nargs="+", default=None, help="(not in the reference) one non-negative weight per "
                   "--reference_path, default all 1; at least one must be positive")
    p.add_argument("--reference_region", type=str, nargs="+", default=None, help="(not in the reference) one grayscale image per "
                   "--reference_path: white where that exemplar applies")
    p.add_argument("--save_reference_maps", action="store_true", help="(not in the reference) write one grayscale attribution map per "
                   "--reference_path into <outdir>/reference_maps/: where the picture attended to that exemplar")
    p.add_argument("--paste_back", action="store_true", help="(not in the reference) --image_path / --mask_path of any size: inpaint a "
                   "window around the hole at --H x --W and write the whole picture, the result blended in, to <outdir>/pasted/")
    p.add_argument("--context", type=float, default=0.5, help="with --paste_back: the window holds the hole's box plus this fraction of its size on each side")
    p.add_argument("--feather", type=int, default=8, help="with --paste_back: the blend mask falls off over 2 x this many picture pixels around the hole")
    p.add_argument("--per_hole", action="store_true", help="with --paste_back: every hole of the mask (connected components, grouped where their "
                   "blend zones could touch) gets a window of its own; pasted/ holds all of them")
    p.add_argument("--reference_per_hole", action="store_true", help="with --per_hole: the i-th --reference_path is the exemplar of the i-th hole, "
                   "holes in raster order of their first pixel")
    p.add_argument("--match_tone", choices=("mean", "affine", "field"), default=None, help="with --paste_back: match the pasted window's tone to the "
                   "picture around the hole - per window and channel an offset (mean) or a gain and an offset (affine) fitted on the known pixels, "
                   "or a low-frequency difference field that follows a tone varying across the window (field); "
                   "pasted/<stem>_<seed>.tone.json holds the fit")
    p.add_argument("--tone_cell", type=int, default=8, choices=(4, 8, 16, 32, 64), metavar="PX", help="with --match_tone field: the cell of the "
                   "difference field in working pixels (4, 8, 16, 32 or 64)")
    p.add_argument("--tone_field_limit", type=float, default=0.125, metavar="V", help="with --match_tone field: the field is clamped to +-V of full "
                   "scale (0.125 = 32 grey levels)")
    p.add_argument("--tone_margin", type=int, default=8, metavar="PX", help="with --match_tone: known pixels nearer to the hole than this many "
                   "working pixels are left out of the fit")
    p.add_argument("--max_holes", type=int, default=16, help="with --per_hole: more separate holes than this is an error")
    p.add_argument("--mask_grow", type=float, default=0.0, metavar="PX", help="(not in the reference) grow the hole by a disc of this radius in "
                   "mask pixels before anything else sees the mask; negative shrinks it")
    p.add_argument("--mask_close", type=float, default=0.0, metavar="PX", help="(not in the reference) fill gaps of the hole narrower than a disc of this radius")
    p.add_argument("--mask_open", type=float, default=0.0, metavar="PX", help="(not in the reference) remove specks of the hole narrower than a disc of this radius")
    p.add_argument("--mask_box", action="store_true", help="(not in the reference) replace every hole by its bounding box; applied after "
                   "--mask_open, --mask_close and --mask_grow, in that order")
    p.add_argument("--reference_on_device", action="store_true", help="(not in the reference) resize the exemplar on the device: the same picture "
                   "as the default path, bit for bit, from the reference's full-size bytes")
    p.add_argument("--reference_box", type=float, nargs="+", default=None, metavar="N", help="(not in the reference) X0 Y0 X1 Y1 per --reference_path: "
                   "the part of that image to take as the exemplar (Pillow's box, fractions allowed)")
    p.add_argument("--reference_mask", type=str, nargs="+", default=None, metavar="PATH", help="(not in the reference) one image per --reference_path, "
                   "of its size, white = the object: the exemplar is the object's bounding box")
    p.add_argument("--reference_pad", type=float, default=0.0, metavar="F", help="with --reference_box / --reference_mask: grow the box by this "
                   "fraction of its size on each side")
    p.add_argument("--reference_square", action="store_true", help="with --reference_box / --reference_mask: grow the box's shorter side to the longer")
    p.add_argument("--reference_fill", type=int, nargs=3, default=None, metavar=("R", "G", "B"), help="with --reference_mask: the colour of "
                   "everything off the object")
    p.add_argument("--seeds", type=int, nargs="+", default=None, metavar="S", help="(not in the reference) one variant of the triple per seed, in one "
                   "batch, all noise drawn on the device as a function of that seed (pbe_amd.noise); the output tree is written once per seed")
    p.add_argument("--hole_seed", type=int, nargs=2, action="append", default=None, metavar=("INDEX", "SEED"), help="with --per_hole --seeds "
                   "(repeatable): hole INDEX draws from SEED instead; the other holes keep their noise")
    p.add_argument("--random_weights", action="store_true", help="name-seeded random weights instead of --ckpt")
    p.add_argument("--dump_tensors", type=str, default="", help="(not in the reference) save the start code, the posterior noise and the "
                   "intermediate tensors of this run to an .npz: what a CPU replay needs to reproduce the run without the device RNG")
    opt = p.parse_args(argv)
    if opt.plms and opt.dpm_solver:
        p.error("--plms and --dpm_solver are mutually exclusive: name one sampler")
    if opt.dpm_solver and opt.ddim_eta != 0.0:
        p.error("--dpm_solver runs with --ddim_eta 0 (the stochastic variant is not built)")
    if opt.seeds is not None:
        if opt.fixed_code:
            raise SystemExit("--seeds draws the start code from each seed: --fixed_code has nothing to fix")
        if opt.n_samples != 1:
            raise SystemExit(f"--seeds runs one sample per seed: --n_samples {opt.n_samples} is not 1")
        if any(not 0 <= v < 1 << 64 for v in opt.seeds) or len(set(opt.seeds)) != len(opt.seeds):
            p.error("--seeds: distinct integers in [0, 2^64)")
    if opt.hole_seed is not None:
        if opt.seeds is None or not opt.per_hole:
            raise SystemExit("--hole_seed re-rolls one hole of a --per_hole --seeds run")
        if any(i < 0 or not 0 <= v < 1 << 64 for i, v in opt.hole_seed) or len({i for i, _ in opt.hole_seed}) != len(opt.hole_seed):
            p.error("--hole_seed: INDEX >= 0 (each hole once) and SEED in [0, 2^64)")
    if opt.reference_weight is not None:
        w, refs = opt.reference_weight, opt.reference_path if isinstance(opt.reference_path, (list, tuple)) else [opt.reference_path]
        if len(w) != len(refs):
            p.error(f"--reference_weight: {len(w)} weights for {len(refs)} --reference_path images")
        if any(not (x >= 0.0) or x == float("inf") for x in w) or not sum(w) > 0.0:
            p.error("--reference_weight: weights must be finite and >= 0 with a positive sum")
    refs = opt.reference_path if isinstance(opt.reference_path, (list, tuple)) else [opt.reference_path]
    if opt.reference_box is not None and len(opt.reference_box) != 4 * len(refs):
        p.error(f"--reference_box: {len(opt.reference_box)} numbers for {len(refs)} --reference_path images (X0 Y0 X1 Y1 each)")
    if opt.reference_mask is not None and len(opt.reference_mask) != len(refs):
        p.error(f"--reference_mask: {len(opt.reference_mask)} masks for {len(refs)} --reference_path images")
    if opt.reference_box is not None and opt.reference_mask is not None and opt.reference_fill is None:
        p.error("--reference_box and --reference_mask both place the crop: name one (with --reference_fill the mask paints the background and goes with a box)")
    if opt.reference_fill is not None and (opt.reference_mask is None or any(not 0 <= v <= 255 for v in opt.reference_fill)):
        p.error("--reference_fill: three bytes R G B, with --reference_mask (it colours what is off the object)")
    if not (0.0 <= opt.reference_pad < float("inf")):
        p.error("--reference_pad must be finite and >= 0")
    if (opt.reference_pad != 0.0 or opt.reference_square) and opt.reference_box is None and opt.reference_mask is None:
        p.error("--reference_pad / --reference_square grow a box: they need --reference_box or --reference_mask")
    if not (opt.context >= 0.0) or opt.context == float("inf") or opt.feather < 0 or opt.feather > 2047:
        p.error("--context must be finite and >= 0, --feather an integer in 0 .. 2047")
    if not (-2047.0 <= opt.mask_grow <= 2047.0) or not (0.0 <= opt.mask_close <= 2047.0) or not (0.0 <= opt.mask_open <= 2047.0):
        p.error("--mask_grow must lie in -2047 .. 2047, --mask_close and --mask_open in 0 .. 2047")
    if (opt.match_tone is not None or opt.tone_margin != 8) and not opt.paste_back:
        raise SystemExit("--match_tone / --tone_margin need --paste_back: the tone is matched where the window is pasted into the picture")
    if opt.tone_margin < 0:
        p.error("--tone_margin must be an integer >= 0")
    if (opt.tone_cell != 8 or opt.tone_field_limit != 0.125) and opt.match_tone != "field":
        raise SystemExit("--tone_cell / --tone_field_limit need --match_tone field: the other modes fit one map per window")
    if not (0.0 < opt.tone_field_limit < float("inf")):
        p.error("--tone_field_limit must be finite and > 0")
    if opt.per_hole:
        if not opt.paste_back:
            raise SystemExit("--per_hole needs --paste_back: the holes are pasted back into the one picture")
        if opt.n_samples != 1:
            raise SystemExit(f"--per_hole runs one sample per hole: --n_samples {opt.n_samples} is not 1")
        if opt.dump_tensors:
            raise SystemExit("--per_hole does not write --dump_tensors (the dump describes one window)")
        if opt.reference_region is not None or opt.save_reference_maps or opt.ddim_eta != 0.0:
            raise SystemExit("--per_hole is not built for --reference_region, --save_reference_maps or a --ddim_eta other than 0")
        if opt.reference_per_hole and opt.reference_weight is not None:
            raise SystemExit("--reference_per_hole gives each hole one exemplar: --reference_weight has nothing to weigh")
    elif opt.reference_per_hole:
        raise SystemExit("--reference_per_hole needs --per_hole")
    if opt.reference_region is not None:
        refs = opt.reference_path if isinstance(opt.reference_path, (list, tuple)) else [opt.reference_path]
        if len(opt.reference_region) != len(refs):
            p.error(f"--reference_region: {len(opt.reference_region)} region images for {len(refs)} --reference_path images")
    return opt


def mask_shape_of(opt):
    """The --mask_* flags as the keywords of pbe_amd.window.shape_mask, or None when none of them is given."""
    if opt.mask_open == 0.0 and opt.mask_close == 0.0 and opt.mask_grow == 0.0 and not opt.mask_box:
        return None
    return {"open": opt.mask_open, "close": opt.mask_close, "grow": opt.mask_grow, "box": bool(opt.mask_box)}


def load_regions(paths, size, device, window=None):
    """One grayscale image per exemplar -> region maps fp32 [1, K, h, w] in [0, 1] on `device`: decoded to uint8 (with --paste_back:
    cropped on the host to `window` = (y0, x0, wh, ww) of the picture, which the region images then have the size of), scaled to [0, 1],
    resized on the device to the latent grid `size` (pipeline.resize_mask: antialiased bilinear, a convex combination, so the values
    stay in [0, 1] up to the rounding of the fp32 filter sums; no threshold).  The clamp takes that rounding away: a sum of -1e-8
    where the image is black would otherwise be refused as a negative region."""
    import numpy as np
    from PIL import Image
    from pbe_amd import pipeline
    maps = []
    for path in paths:
        img = Image.open(path).convert("L")
        if window is not None:
            y0, x0, wh, ww = window
            img = img.crop((x0, y0, x0 + ww, y0 + wh))
        u8 = torch.from_numpy(np.array(img, dtype=np.uint8)).to(device)
        maps.append(pipeline.resize_mask(u8.float()[None, None] / 255.0, size))
    return torch.cat(maps, 1).clamp_(0.0, 1.0)


def reference_on_device(opt) -> bool:
    """True when the exemplar is to be cut on the device: --reference_on_device, or any flag that crops it."""
    return bool(opt.reference_on_device or opt.reference_box is not None or opt.reference_mask is not None or opt.reference_pad != 0.0
                or opt.reference_square or opt.reference_fill is not None)


def cut_references(opt, refs, device):
    """The exemplars of the --reference_* flags: one fp32 [1, 3, 224, 224] per --reference_path, cut on the device
    (pbe_amd.preprocess.load_reference_device), and <outdir>/reference_crops/<stem>_ref<k>.png with the bytes of each.  None on the
    default path, which then runs as it always did."""
    if not reference_on_device(opt):
        return None
    from PIL import Image
    from pbe_amd import preprocess
    d, stem = os.path.join(opt.outdir, "reference_crops"), os.path.basename(opt.image_path)[:-4]
    os.makedirs(d, exist_ok=True)
    planes = []
    for k, path in enumerate(refs):
        box = None if opt.reference_box is None else tuple(opt.reference_box[4 * k:4 * k + 4])
        e = preprocess.load_reference_device(path, device, box=box, mask_path=None if opt.reference_mask is None else opt.reference_mask[k],
                                             pad=opt.reference_pad, square=opt.reference_square, fill=opt.reference_fill)
        Image.fromarray(e["u8"].cpu().numpy()).save(os.path.join(d, f"{stem}_ref{k}.png"))
        print(f"reference {k}: box (x0, y0, x1, y1) = {e['box']} of {path}")
        planes.append(e["ref"])
    return planes


def save_reference_maps(outdir, stem, seed, ref_maps, H, W):
    """ref_maps fp32 [B, K, h, w] (ContextMaps.result) -> <outdir>/reference_maps/<stem>_<seed>[_<i>]_ref<j>.png, 8-bit grayscale
    round(255 * map) at the picture size (pipeline.ref_maps_u8: resized on the device).  Returns the paths, sample-major."""
    from PIL import Image
    from pbe_amd import pipeline
    d = os.path.join(outdir, "reference_maps")
    os.makedirs(d, exist_ok=True)
    u8 = pipeline.ref_maps_u8(ref_maps, (H, W)).cpu().numpy()
    paths = []
    for i in range(u8.shape[0]):
        tag = f"{stem}_{seed}" if u8.shape[0] == 1 else f"{stem}_{seed}_{i}"
        for j in range(u8.shape[1]):
            paths.append(os.path.join(d, f"{tag}_ref{j}.png"))
            Image.fromarray(u8[i, j], mode="L").save(paths[-1])
    return paths


def report_tone(outdir, stem, seed, fits):
    """--match_tone: a line per window and pasted/<stem>_<seed>.tone.json with pbe_amd.window.fit_tone's list (tone_field's summary in the
    field mode)."""
    import json
    fmt = lambda v, spec: "(" + ", ".join(format(x, spec) for x in v) + ")"      # noqa: E731
    for i, f in enumerate(fits):
        if f.get("mode") == "field":
            print(f"tone of window {i}: field over n = {f['n']} pixels, grid {f['grid'][0]} x {f['grid'][1]} cells of {f['cell']} ({f['levels']} levels), range "
                  f"{fmt(f['field_min'], '+.2f')} .. {fmt(f['field_max'], '+.2f')} grey levels, whole-window offset {fmt(f['offset'], '+.4f')}"
                  + (" (identity)" if f["identity"] else ""))
            continue
        print(f"tone of window {i}: gain {fmt(f['gain'], '.4f')}, offset {fmt(f['offset'], '+.4f')}, rms {fmt(f['rms_before'], '.2f')} -> "
              f"{fmt(f['rms_after'], '.2f')} grey levels over n = {f['n']} pixels" + (" (identity)" if f["identity"] else ""))
    with open(os.path.join(outdir, "pasted", f"{stem}_{seed}.tone.json"), "w") as fh:
        json.dump(fits, fh, indent=1)


def run_per_hole(opt, model, device, refs):
    """--paste_back --per_hole: pipeline.inpaint_holes on the picture, one set of source / results / grid files per hole and the picture
    with every hole pasted.  Returns the windows' results [N, 3, H, W] on the host."""
    from PIL import Image
    from pbe_amd import ops, pipeline, preprocess
    from pbe_amd import window as pbe_window
    u8 = preprocess.load_triple_u8(opt.image_path, opt.mask_path, refs[0])
    if u8["image"].shape[:2] != u8["mask"].shape:
        raise SystemExit(f"--paste_back: the image is {u8['image'].shape[:2]}, the mask {u8['mask'].shape}")
    picture, picture_mask = torch.from_numpy(u8["image"]).to(device), torch.from_numpy(u8["mask"]).to(device)
    if mask_shape_of(opt) is not None:                                                 # shaped once, here: inpaint_holes gets the shaped mask
        picture_mask = pbe_window.shape_mask(picture_mask, **mask_shape_of(opt))
    size = (opt.H, opt.W)
    _, table = ops.component_boxes(ops.mask_components(picture_mask))
    N = len(pbe_window.plan_holes(table, picture_mask.shape, size, opt.context, opt.feather, opt.max_holes))
    if opt.reference_per_hole and len(refs) != N:
        raise SystemExit(f"--reference_per_hole: {len(refs)} --reference_path images for {N} holes")
    cut = cut_references(opt, refs, device)
    if cut is not None:
        planes = [c[0] for c in cut]
    else:
        planes = [preprocess.load_triple_device(opt.image_path, opt.mask_path, r, device)["ref"][0] for r in refs]    # each [3, 224, 224]
    kw = {}
    if opt.reference_per_hole:
        ref = torch.stack(planes)                                                      # [N, 3, 224, 224]: exemplar i for hole i
    else:
        ref = torch.stack(planes)[None] if len(planes) > 1 else planes[0][None]        # the sample's exemplars, for every hole
        if opt.reference_weight is not None:
            kw["ref_weights"] = torch.tensor([opt.reference_weight], dtype=torch.float64).expand(N, -1).contiguous()
    shape = (N, opt.C, opt.H // opt.f, opt.W // opt.f)
    if opt.seeds is not None:                                                          # one call per seed, all noise from pbe_amd.noise
        if any(i >= N for i, _ in opt.hole_seed or []):
            raise SystemExit(f"--hole_seed: the mask has holes 0 .. {N - 1}")
        return torch.cat([_per_hole_call(opt, model, picture, picture_mask, ref, planes, N, s,
                                         dict(kw, seeds=[s], hole_seeds={i: v for i, v in opt.hole_seed or []})) for s in opt.seeds])
    if opt.fixed_code:
        kw["x_T"] = torch.randn(shape, device=device, generator=torch.Generator(device=device).manual_seed(opt.seed))
    kw["post_eps"] = torch.randn(shape, generator=torch.Generator().manual_seed(opt.seed)).to(device)
    return _per_hole_call(opt, model, picture, picture_mask, ref, planes, N, opt.seed, kw)


def _per_hole_call(opt, model, picture, picture_mask, ref, planes, N, tag, kw):
    """One pipeline.inpaint_holes call of run_per_hole and its files, `tag` (the seed) in every name."""
    from PIL import Image
    from pbe_amd import pipeline, preprocess
    size = (opt.H, opt.W)
    out = pipeline.inpaint_holes(model, [picture], [picture_mask], ref, size=size, context=opt.context, feather=opt.feather, max_holes=opt.max_holes,
                                 steps=opt.ddim_steps, scale=opt.scale, sampler="dpm" if opt.dpm_solver else ("plms" if opt.plms else "ddim"),
                                 **({} if opt.match_tone is None else {"tone": opt.match_tone, "tone_margin": opt.tone_margin}),
                                 **({"tone_cell": opt.tone_cell, "tone_field_limit": opt.tone_field_limit} if opt.match_tone == "field" else {}), **kw)
    stem = os.path.basename(opt.image_path)[:-4]
    if not opt.skip_save:
        for i in range(N):
            t = {k: out["inputs"][k][i:i + 1] for k in ("image", "mask", "inpaint")}
            t["ref"] = (ref[i] if opt.reference_per_hole else planes[0])[None]
            preprocess.save_outputs_device(opt.outdir, f"{stem}_hole{i}", tag, t, out["image"][i], opt.H, opt.W)
    os.makedirs(os.path.join(opt.outdir, "pasted"), exist_ok=True)
    Image.fromarray(out["pictures"][0].cpu().numpy()).save(os.path.join(opt.outdir, "pasted", f"{stem}_{tag}.png"))
    if opt.match_tone is not None:
        report_tone(opt.outdir, stem, tag, out["tone"])
    for i, h in enumerate(out["holes"]):
        print(f"hole {i}: {h['area']} pixels in rows {h['box'][0]} .. {h['box'][1]}, columns {h['box'][2]} .. {h['box'][3]}; window {h['window']}"
              + (f"; noise (seed, sub) = ({h['seed']}, {h['sub']})" if "seed" in h else ""))
    return out["image"].cpu()


def seed_everything(seed):
    import random
    import numpy as np
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def main(argv=None):
    opt = parse(argv)
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.ddpm import load_model_from_config
    from ldm.models.diffusion.plms import PLMSSampler
    from ldm.util import load_yaml_config
    from pbe_amd import ops, pipeline, preprocess, weights

    seed_everything(opt.seed)
    if not torch.cuda.is_available():
        raise SystemExit("scripts/inference.py needs an MI355X: the HIP path has no CPU fallback")
    device = torch.device("cuda")
    config = load_yaml_config(opt.config or os.path.join(ROOT, "configs", "v1.yaml"))
    if opt.ckpt and not opt.random_weights:
        model = load_model_from_config(config, opt.ckpt, device=device)
    else:
        print("no --ckpt: running with name-seeded random weights")
        model = load_model_from_config(config, None, device="cpu")
        weights.fill_latent_diffusion_(model, seed=0)
        model = model.to(device).eval()
    if opt.dpm_solver:
        from ldm.models.diffusion.dpm_solver import DPMSolverSampler
        sampler = DPMSolverSampler(model)
    else:
        sampler = PLMSSampler(model) if opt.plms else DDIMSampler(model)

    start_code = None
    if opt.fixed_code:
        start_code = torch.randn([opt.n_samples, opt.C, opt.H // opt.f, opt.W // opt.f], device=device)

    with torch.no_grad(), model.ema_scope():
        refs = list(opt.reference_path) if isinstance(opt.reference_path, (list, tuple)) else [opt.reference_path]
        if opt.per_hole:                                                               # one window per hole: its own path, the rest is unchanged
            x = run_per_hole(opt, model, device, refs)
            print(f"Your samples are ready and waiting for you here: \n{opt.outdir} \n \nEnjoy.")
            return x
        win, mask_shape = None, mask_shape_of(opt)
        if opt.paste_back:                                                             # a picture of any size: one window of it at H x W
            from pbe_amd import window as pbe_window
            u8 = preprocess.load_triple_u8(opt.image_path, opt.mask_path, refs[0])
            if u8["image"].shape[:2] != u8["mask"].shape:
                raise SystemExit(f"--paste_back: the image is {u8['image'].shape[:2]}, the mask {u8['mask'].shape}")
            picture, picture_mask = torch.from_numpy(u8["image"]).to(device), torch.from_numpy(u8["mask"]).to(device)
            if mask_shape is not None:
                picture_mask = pbe_window.shape_mask(picture_mask, **mask_shape)
            win = pbe_window.plan_window(u8["mask"] if mask_shape is None else picture_mask, (opt.H, opt.W), opt.context, opt.feather)
            t = pipeline.window_inputs([picture], [picture_mask], [win], (opt.H, opt.W))
            t["ref"] = ops.u8_to_planes(torch.from_numpy(u8["ref"]).to(device)[None], preprocess.CLIP_MEAN, preprocess.CLIP_STD)
        else:
            t = preprocess.load_triple_device(opt.image_path, opt.mask_path, refs[0], device, mask_shape=mask_shape)   # uint8 up, arithmetic on the GPU
        filename = os.path.basename(opt.image_path)
        test_model_kwargs = {"inpaint_mask": t["mask"], "inpaint_image": t["inpaint"]}
        cut = cut_references(opt, refs, device)                                        # None on the default path
        if cut is not None:
            t["ref"] = cut[0]                                                          # (the triple loader's host-resized exemplar is dropped)
        ref = t["ref"]
        if len(refs) > 1:                                                              # several exemplars: [1, K, 3, 224, 224] -> K context tokens
            more = cut[1:] if cut is not None else [preprocess.load_triple_device(opt.image_path, opt.mask_path, r, device)["ref"] for r in refs[1:]]
            ref = torch.stack([ref] + more, 1)
        uc = model.learnable_vector if opt.scale != 1.0 else None
        c = model.proj_out(model.get_learned_conditioning(ref))                      # scripts/inference.py:326-327
        nb = opt.n_samples
        if opt.seeds is not None:                                                      # one variant per seed: the triple's tensors, repeated
            nb = len(opt.seeds)
            c = c.expand(nb, -1, -1).contiguous()
        cw = None
        if opt.reference_weight is not None:                                           # one weight per exemplar token, the same for every sample
            cw = torch.tensor([opt.reference_weight], dtype=torch.float64).expand(c.shape[0], -1).contiguous()
        post = model.encode_first_stage(test_model_kwargs["inpaint_image"])
        pb, ph, pw, _ = post.parameters.shape
        post_eps = torch.randn((pb, post.z, ph, pw)) if opt.dump_tensors else None   # the CPU draw DiagonalGaussianDistribution.sample() makes itself
        if opt.seeds is not None:                                                      # encoded once; each variant samples the posterior with its own noise
            from pbe_amd.noise import SeededNoise
            post = type(post)(post.parameters.expand(nb, -1, -1, -1).contiguous(), post.deterministic)
            eps = SeededNoise(opt.seeds, device=device).post_eps((nb, post.z, ph, pw))
            post_eps = eps.cpu() if opt.dump_tensors else None
            z_inpaint = model.get_first_stage_encoding(post, noise=eps)
        else:
            z_inpaint = model.get_first_stage_encoding(post, noise=None if post_eps is None else post_eps.to(device))
        test_model_kwargs["inpaint_image"] = z_inpaint
        test_model_kwargs["inpaint_mask"] = pipeline.resize_mask(test_model_kwargs["inpaint_mask"], z_inpaint.shape[-2:])
        if opt.seeds is not None:
            test_model_kwargs["inpaint_mask"] = test_model_kwargs["inpaint_mask"].expand(nb, -1, -1, -1).contiguous()
            extra_seeds = {"seeds": list(opt.seeds)}
        else:
            extra_seeds = {}
        cr = None
        if opt.reference_region is not None:                                           # one map per exemplar token, the same for every sample
            cr = load_regions(opt.reference_region, z_inpaint.shape[-2:], device, win).expand(c.shape[0], -1, -1, -1).contiguous()
        cm = None
        if opt.save_reference_maps:
            from ldm.modules.attention import ContextMaps
            cm = ContextMaps()
        shape = [opt.C, opt.H // opt.f, opt.W // opt.f]
        samples, _ = sampler.sample(S=opt.ddim_steps, conditioning=c, batch_size=nb, shape=shape, verbose=False,
                                    unconditional_guidance_scale=opt.scale, unconditional_conditioning=uc, eta=opt.ddim_eta,
                                    x_T=start_code, test_model_kwargs=test_model_kwargs, conditioning_weights=cw, conditioning_regions=cr,
                                    conditioning_maps=cm, **extra_seeds)
        xd = ops.image_post(model.decode_first_stage_nhwc(samples))                  # clamp((x+1)/2, 0, 1), still on the GPU
        tags = [opt.seed] * xd.shape[0] if opt.seeds is None else list(opt.seeds)      # what names sample i's files
        if not opt.skip_save:
            for i in range(xd.shape[0]):
                paths = preprocess.save_outputs_device(opt.outdir, filename[:-4], tags[i], t, xd[i], opt.H, opt.W)
        if win is not None:                                                            # (an explicit request: written with --skip_save too)
            from PIL import Image
            os.makedirs(os.path.join(opt.outdir, "pasted"), exist_ok=True)
            alpha = ops.feather_alpha(picture_mask, win, opt.feather)
            maps = [None] * xd.shape[0]
            fields = None
            if opt.match_tone == "field":                                              # per saved sample against the one window the model saw
                n = xd.shape[0]
                fits, fields, _ = pipeline.match_tone_field(t["image"].expand(n, -1, -1, -1), xd, [picture_mask] * n, [win] * n, (opt.H, opt.W), opt.tone_margin,
                                                            opt.tone_cell, opt.tone_field_limit)
            elif opt.match_tone is not None:
                n = xd.shape[0]
                fits, _ = pipeline.match_tone(t["image"].expand(n, -1, -1, -1), xd, [picture_mask] * n, [win] * n, (opt.H, opt.W), opt.match_tone,
                                              opt.tone_margin)
                maps = [(f["gain"], f["offset"]) for f in fits]
            for i in range(xd.shape[0]):
                if fields is not None:
                    pasted = ops.paste_window(xd[i].contiguous(), alpha, picture.clone(), win, field=fields[i], cell=opt.tone_cell)
                else:
                    pasted = ops.paste_window(xd[i].contiguous(), alpha, picture.clone(), win, tone=maps[i])
                Image.fromarray(pasted.cpu().numpy()).save(os.path.join(opt.outdir, "pasted", f"{filename[:-4]}_{tags[i]}.png"))
            if opt.match_tone is not None and opt.seeds is None:
                report_tone(opt.outdir, filename[:-4], opt.seed, fits)
            elif opt.match_tone is not None:
                for i, s_ in enumerate(tags):
                    report_tone(opt.outdir, filename[:-4], s_, fits[i:i + 1])
        ref_maps = None
        if cm is not None:                                                             # (an explicit request: written with --skip_save too)
            ref_maps = cm.result(z_inpaint.shape[-2:])
            if opt.seeds is None:
                save_reference_maps(opt.outdir, filename[:-4], opt.seed, ref_maps, opt.H, opt.W)
            else:
                for i, s_ in enumerate(tags):
                    save_reference_maps(opt.outdir, filename[:-4], s_, ref_maps[i:i + 1], opt.H, opt.W)
        x = xd.cpu()
        if opt.dump_tensors:
            import numpy as np
            if opt.seeds is not None:                                                  # the start code the sampler drew: stream 0 of each seed
                from pbe_amd.noise import STREAM_X_T
                start_code = ops.randn_seeded(list(opt.seeds), [nb] + shape, STREAM_X_T)
            np.savez(opt.dump_tensors, x_T=(start_code if start_code is not None else torch.zeros(0)).float().cpu().numpy(),
                     post_eps=post_eps.numpy(), c=c.float().cpu().numpy(), z_inpaint=z_inpaint.float().cpu().numpy(),
                     mask64=test_model_kwargs["inpaint_mask"].float().cpu().numpy(), latent=samples.float().cpu().numpy(), image=x.numpy(),
                     reference_weight=(cw if cw is not None else torch.ones(c.shape[:2])).double().numpy(),
                     **({} if win is None else {"window": np.array(win, dtype=np.int64)}),
                     **({} if cr is None else {"reference_region": cr.double().cpu().numpy()}),
                     **({} if ref_maps is None else {"ref_maps": ref_maps.float().cpu().numpy()}))
    print(f"Your samples are ready and waiting for you here: \n{opt.outdir} \n \nEnjoy.")
    return x


if __name__ == "__main__":
    main()
