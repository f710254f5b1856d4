"""Tensor-level wrappers over the C-ABI (include/pbe_hip.h) around uint8 pictures and masks: the conversions between bytes and fp32
planes, the window kernels, the tone of a pasted window, the holes of a mask and its shape, Pillow's resize and the box of a mask.

ops.py re-exports every public name of this module (``from .ops_picture import *``): callers write ``ops.window_image`` as they
always did.  Like ops.py, nothing here computes on the CPU: all wrappers raise if handed CPU tensors.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import lib as _l
from .opsbase import _f, _p, _req, _stream, floats3, out_tensor, workspace

__all__ = ["clip_patchify", "resize_bilinear", "u8_to_planes", "mul_planes", "planes_to_canvas",
           "window_image", "window_mask", "feather_alpha", "paste_window",
           "tone_stats", "TONE_CELLS", "tone_cells", "tone_field",
           "mask_components", "component_boxes", "select_components",
           "MASK_RMAX", "mask_dist2", "mask_grow", "mask_close", "mask_open", "fill_boxes",
           "MASK_BOX_BAND", "resample_u8", "mask_box"]


def clip_patchify(pixels: torch.Tensor, patch: int, kp: int) -> torch.Tensor:
    _f(pixels, "clip_patchify pixels")
    pixels = pixels.contiguous()
    B, _, S, _ = pixels.shape
    g = S // patch
    y = torch.empty((B * g * g, kp), dtype=torch.float16, device=pixels.device)
    _l.check(_l.load().pbe_clip_patchify_f16(_p(pixels), _p(y), B, S, patch, kp, _stream()), "pbe_clip_patchify_f16")
    return y


def resize_bilinear(x: torch.Tensor, size, antialias: bool = True) -> torch.Tensor:
    """fp32 [B, C, H, W] -> [B, C, h, w], bilinear, align_corners=False (the mask resize of scripts/inference.py:332)."""
    _f(x, "resize_bilinear x")
    x = x.contiguous()
    B, Cc, H, W = x.shape
    h, w = int(size[0]), int(size[1])
    y = torch.empty((B, Cc, h, w), dtype=torch.float32, device=x.device)
    _l.check(_l.load().pbe_resize_bilinear_f32(_p(x), _p(y), B * Cc, H, W, h, w, 1 if antialias else 0, _stream()), "pbe_resize_bilinear_f32")
    return y


def u8_to_planes(src: torch.Tensor, mean=None, std=None, mask_mode: int = 0) -> torch.Tensor:
    """uint8 [B, H, W, C] (C = 3) or [B, H, W] (mask) on the GPU -> fp32 [B, C, H, W]: (v/255 - mean) / std, or the mask forms
    mask_mode 1: (1 - v/255) thresholded at 0.5 (scripts/inference.py:311-315), 2: 1 - v/255 (test_bench_dataset.py)."""
    _req(src, torch.uint8, "u8_to_planes src")
    src = src.contiguous()
    if src.dim() == 3:
        src = src.unsqueeze(-1)
    B, H, W, Cc = src.shape
    y = torch.empty((B, Cc, H, W), dtype=torch.float32, device=src.device)
    m = floats3((list(mean) + [0.0] * 3)[:3]) if mean is not None else None
    sd = floats3((list(std) + [1.0] * 3)[:3]) if std is not None else None
    _l.check(_l.load().pbe_u8_to_planes_f32(_p(src), _p(y), B, Cc, H * W, m, sd, mask_mode, _stream()), "pbe_u8_to_planes_f32")
    return y


def mul_planes(x: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """x [B, C, H, W] * m [B, 1, H, W] (inpaint_image = image * mask)."""
    _f(x, "mul_planes x"); _f(m, "mul_planes m")
    x, m = x.contiguous(), m.contiguous()
    B, Cc, H, W = x.shape
    y = torch.empty_like(x)
    _l.check(_l.load().pbe_mul_planes_f32(_p(x), _p(m), _p(y), B, Cc, H * W, _stream()), "pbe_mul_planes_f32")
    return y


def planes_to_canvas(src: torch.Tensor, canvas: torch.Tensor, y0: int, x0: int, a=(1.0, 1.0, 1.0), b=(0.0, 0.0, 0.0)) -> None:
    """One fp32 [3, H, W] (or [1, H, W]: broadcast to 3 channels) image -> canvas[y0:y0+H, x0:x0+W, :] (uint8 [Hc, Wc, 3]) as
    trunc(255 * clamp(x * a[c] + b[c], 0, 1))."""
    _f(src, "planes_to_canvas src"); _req(canvas, torch.uint8, "planes_to_canvas canvas")
    src = src.contiguous()
    Cc, H, W = src.shape
    if not canvas.is_contiguous() or canvas.dim() != 3 or canvas.shape[2] != 3 or Cc not in (1, 3):
        raise _l.PbeError("planes_to_canvas: canvas must be a contiguous [Hc, Wc, 3] uint8 tensor, src [3 or 1, H, W]")
    _l.check(_l.load().pbe_planes_to_u8_canvas(_p(src), _p(canvas), H, W, canvas.shape[0], canvas.shape[1], int(y0), int(x0), floats3(a), floats3(b),
                                               1 if Cc == 1 else 0, _stream()), "pbe_planes_to_u8_canvas")


# ---- windowed pre/post-processing (csrc/window.hip): one picture per call ---------------------------------------------------------
def _picture_args(what: str, plane: torch.Tensor, channels: int) -> Tuple[int, int]:
    """(Hs, Ws) of a contiguous uint8 [Hs, Ws, 3] picture (channels = 3) or [Hs, Ws] mask (channels = 1) on the GPU.  No limit on the
    edges: the entry points have their own (_plane_args, for the wrappers that take a bare plane, checks 16384 here)."""
    _req(plane, torch.uint8, f"{what}")
    if plane.dim() != (3 if channels == 3 else 2) or (channels == 3 and plane.shape[2] != 3) or not plane.is_contiguous() or plane.numel() == 0:
        raise _l.PbeError(f"{what}: expected a contiguous uint8 {'[Hs, Ws, 3] picture' if channels == 3 else '[Hs, Ws] mask'}, got {tuple(plane.shape)} "
                          f"with strides {tuple(plane.stride())}")
    return int(plane.shape[0]), int(plane.shape[1])


def _window_in(what: str, window, Hs: int, Ws: int) -> Tuple[int, int, int, int]:
    """(y0, x0, wh, ww) of a window of four integers inside a Hs x Ws picture."""
    try:
        y0, x0, wh, ww = (int(v) for v in window)
        exact = all(int(v) == v for v in window)
    except (TypeError, ValueError) as e:
        raise _l.PbeError(f"{what}: the window must be four integers (y0, x0, wh, ww), got {window!r}") from e
    if not exact or y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > Hs or x0 + ww > Ws:
        raise _l.PbeError(f"{what}: window (y0, x0, wh, ww) = {tuple(window)} is not inside the {Hs} x {Ws} picture")
    return y0, x0, wh, ww


def _window_args(what: str, plane: torch.Tensor, channels: int, window) -> Tuple[int, int, int, int, int, int]:
    """(Hs, Ws, y0, x0, wh, ww): _picture_args of the plane, then _window_in of the window."""
    Hs, Ws = _picture_args(what, plane, channels)
    return (Hs, Ws, *_window_in(what, window, Hs, Ws))


def window_image(picture: torch.Tensor, window, size, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [Hs, Ws, 3] picture, window (y0, x0, wh, ww) -> fp32 [3, H, W] at the working size `size` = (H, W): the antialiased triangle
    filter (pbe_resize_bilinear_f32's, any scale) over bytes / 255 of the window alone, then (v - mean) / std.  A window of the working
    size gives u8_to_planes of the cropped bytes bit for bit."""
    Hs, Ws, y0, x0, wh, ww = _window_args("window_image picture", picture, 3, window)
    H, W = int(size[0]), int(size[1])
    y = out_tensor("window_image", out, (3, H, W), torch.float32, picture.device)
    _l.check(_l.load().pbe_window_image_u8_f32(_p(picture), _p(y), Hs, Ws, y0, x0, wh, ww, H, W, floats3(mean), floats3(std), _stream()),
             "pbe_window_image_u8_f32")
    return y


def window_mask(mask: torch.Tensor, window, size, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [Hs, Ws] mask (a byte >= 128 is the hole), window -> the keep plane fp32 [1, H, W] in {0, 1}: working pixel (Y, X) is 0 iff a
    hole byte lies in window rows (Y wh) // H .. ceil((Y + 1) wh / H) - 1 and the columns likewise.  No filter: exact, no hole pixel is
    lost at any scale; at the working size it is u8_to_planes(mask_mode=1)."""
    Hs, Ws, y0, x0, wh, ww = _window_args("window_mask mask", mask, 1, window)
    H, W = int(size[0]), int(size[1])
    y = out_tensor("window_mask", out, (1, H, W), torch.float32, mask.device)
    _l.check(_l.load().pbe_window_mask_u8_f32(_p(mask), _p(y), Hs, Ws, y0, x0, wh, ww, H, W, _stream()), "pbe_window_mask_u8_f32")
    return y


def feather_alpha(mask: torch.Tensor, window, feather: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [Hs, Ws] mask, window, r = feather >= 0 -> alpha fp32 [wh, ww] = box_r(dilate_r(hole)) / (2r + 1)^2 with replicate padding at
    the picture's border: 1 on the hole, > 0 exactly within Chebyshev distance 2r of it, 0 beyond; r = 0 is the hole itself."""
    Hs, Ws, y0, x0, wh, ww = _window_args("feather_alpha mask", mask, 1, window)
    r = int(feather)
    if r != feather or r < 0 or r > 2047:
        raise _l.PbeError(f"feather_alpha: feather must be an integer in 0 .. 2047, got {feather!r}")
    y = out_tensor("feather_alpha", out, (wh, ww), torch.float32, mask.device)
    lib = _l.load()
    ws = workspace(mask.device, "feather", lib.pbe_feather_alpha_workspace_bytes(wh, ww, r), 1 << 20)
    _l.check(lib.pbe_feather_alpha_f32(_p(mask), _p(y), Hs, Ws, y0, x0, wh, ww, r, _p(ws), ws.numel(), _stream()), "pbe_feather_alpha_f32")
    return y


def _tone_pair(tone):
    """tone = (gain, offset), two sequences of three finite floats -> two (c_float * 3) arrays, or PbeError."""
    try:
        gain, offset = tone
        g, b = [float(v) for v in gain], [float(v) for v in offset]
    except (TypeError, ValueError) as e:
        raise _l.PbeError(f"paste_window: tone must be (gain, offset), two sequences of three floats, got {tone!r}") from e
    if len(g) != 3 or len(b) != 3 or not all(math.isfinite(v) for v in g + b):
        raise _l.PbeError(f"paste_window: tone must be (gain, offset), two sequences of three finite floats, got {tone!r}")
    return floats3(g), floats3(b)


def paste_window(result: torch.Tensor, alpha: torch.Tensor, picture: torch.Tensor, window, tone=None, field: Optional[torch.Tensor] = None,
                 cell: int = 8) -> torch.Tensor:
    """result fp32 [3, H, W] in [0, 1] (one image of image_post), alpha fp32 [wh, ww], window -> `picture` (uint8 [Hs, Ws, 3]) changed IN
    PLACE and returned: where alpha > 0, byte = rint(255 clamp(fma(alpha, res, (1 - alpha) byte / 255), 0, 1)) with res the antialiased
    filter of result to (wh, ww).  Where alpha == 0 and outside the window no byte is written.
    tone = (gain, offset), three floats each (pbe_amd.window.fit_tone's): res = fma(gain[c], res, offset[c]) per channel before the blend
    (pbe_paste_window_tone_u8); ((1, 1, 1), (0, 0, 0)) gives the bytes of tone=None, which launches the plain kernel as it always did.
    field = fp32 [3, Hc, Wc] (one window of tone_field's, at `cell` working pixels per cell: Hc = ceil(H / cell), Wc = ceil(W / cell)):
    res += the field, sampled bilinearly at the window pixel's centre, before the blend (pbe_paste_window_field_u8).  A zero field gives
    the bytes of the plain paste, a constant field b those of tone=((1, 1, 1), (b, b, b)).  field and tone together are refused."""
    Hs, Ws, y0, x0, wh, ww = _window_args("paste_window picture", picture, 3, window)
    _f(result, "paste_window result"); _f(alpha, "paste_window alpha")
    if result.dim() != 3 or result.shape[0] != 3 or not result.is_contiguous() or result.device != picture.device:
        raise _l.PbeError(f"paste_window: result must be a contiguous fp32 [3, H, W] tensor on the picture's device, got {tuple(result.shape)}")
    H, W = int(result.shape[1]), int(result.shape[2])
    if tuple(alpha.shape) != (wh, ww) or not alpha.is_contiguous() or alpha.device != picture.device:
        raise _l.PbeError(f"paste_window: alpha must be a contiguous fp32 [{wh}, {ww}] tensor on the picture's device, got {tuple(alpha.shape)}")
    if field is not None:
        if tone is not None:
            raise _l.PbeError("paste_window: field and tone together: the field is additive with gain 1, take one of the two")
        _f(field, "paste_window field")
        _cell("paste_window", cell)
        want = (3, -(-H // cell), -(-W // cell))
        if tuple(field.shape) != want or not field.is_contiguous() or field.device != picture.device:
            raise _l.PbeError(f"paste_window: field must be a contiguous fp32 {list(want)} tensor on the picture's device (cell {cell}), got {tuple(field.shape)}")
        _l.check(_l.load().pbe_paste_window_field_u8(_p(result), _p(alpha), _p(picture), Hs, Ws, y0, x0, wh, ww, H, W, _p(field), want[1], want[2], int(cell),
                                                     _stream()), "pbe_paste_window_field_u8")
        return picture
    if tone is not None:
        g, b = _tone_pair(tone)
        _l.check(_l.load().pbe_paste_window_tone_u8(_p(result), _p(alpha), _p(picture), Hs, Ws, y0, x0, wh, ww, H, W, g, b, _stream()),
                 "pbe_paste_window_tone_u8")
        return picture
    _l.check(_l.load().pbe_paste_window_u8(_p(result), _p(alpha), _p(picture), Hs, Ws, y0, x0, wh, ww, H, W, _stream()), "pbe_paste_window_u8")
    return picture


# ---- the tone of a pasted window (csrc/tone.hip): the sums pbe_amd.window.fit_tone fits its affine map from ---------------------------
def _tone_operands(what: str, image: torch.Tensor, result: torch.Tensor, sel: torch.Tensor) -> Tuple[int, int, int]:
    """(B, H, W) of image fp32 [B, 3, H, W], result fp32 [B, 3, H, W] and sel fp32 [B, 1, H, W], contiguous on one GPU, B in 1 .. 65535 and
    edges in 1 .. 16384."""
    _f(image, f"{what} image"); _f(result, f"{what} result"); _f(sel, f"{what} sel")
    if image.dim() != 4 or image.shape[1] != 3 or image.numel() == 0 or max(image.shape[2:]) > 16384 or image.shape[0] > 65535:
        raise _l.PbeError(f"{what}: image must be fp32 [B, 3, H, W] with B in 1 .. 65535 and edges in 1 .. 16384, got {tuple(image.shape)}")
    B, _, H, W = (int(v) for v in image.shape)
    if tuple(result.shape) != (B, 3, H, W) or tuple(sel.shape) != (B, 1, H, W):
        raise _l.PbeError(f"{what}: result must be [{B}, 3, {H}, {W}] and sel [{B}, 1, {H}, {W}], got {tuple(result.shape)} and {tuple(sel.shape)}")
    if not (image.is_contiguous() and result.is_contiguous() and sel.is_contiguous()):
        raise _l.PbeError(f"{what}: image, result and sel must be contiguous")
    if result.device != image.device or sel.device != image.device:
        raise _l.PbeError(f"{what}: image, result and sel must be on one device, got {image.device}, {result.device}, {sel.device}")
    return B, H, W


def tone_stats(image: torch.Tensor, result: torch.Tensor, sel: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """image fp32 [B, 3, H, W] model-normalised in [-1, 1] (window_image), result fp32 [B, 3, H, W] in [0, 1] (image_post), sel fp32
    [B, 1, H, W] -> int64 [B, 3, 6] on the device: per sample and channel n, sum o, sum q, sum o^2, sum q^2, sum o q over the pixels with
    sel >= 0.5, o = rint(255 clamp(0.5 x + 0.5, 0, 1)) and q = rint(255 clamp(r, 0, 1)) the two pictures as bytes (a NaN value counts as
    0, a NaN in sel selects nothing).  Integer sums: the table is exact and the same from run to run.  Every element is written."""
    B, H, W = _tone_operands("tone_stats", image, result, sel)
    y = out_tensor("tone_stats", out, (B, 3, 6), torch.int64, image.device)
    lib = _l.load()
    ws = workspace(image.device, "tone", lib.pbe_tone_stats_workspace_bytes(B, H, W), 1 << 16)
    _l.check(lib.pbe_tone_stats_i64(_p(image), _p(result), _p(sel), _p(y), B, H, W, _p(ws), ws.numel(), _stream()), "pbe_tone_stats_i64")
    return y


# ---- a tone that varies across the window (csrc/tone_field.hip): cell sums of o - q, and the pull-push field made of them -------------
TONE_CELLS = (4, 8, 16, 32, 64)


def _cell(what: str, cell) -> None:
    if isinstance(cell, bool) or cell not in TONE_CELLS:
        raise _l.PbeError(f"{what}: cell must be one of {TONE_CELLS}, got {cell!r}")


def tone_cells(image: torch.Tensor, result: torch.Tensor, sel: torch.Tensor, cell: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """image, result, sel as for tone_stats; cell in (4, 8, 16, 32, 64) working pixels (8: one latent cell) -> int32 [B, 4, Hc, Wc] on the
    device, Hc = ceil(H / cell), Wc = ceil(W / cell): plane 0 the number of pixels of the cell with sel >= 0.5, planes 1 .. 3 the sum of
    o - q over them per channel (o, q: tone_stats' two bytes).  The last cell row and column may be ragged.  Integer sums: the table is
    exact and the same from run to run.  Every element is written exactly once."""
    B, H, W = _tone_operands("tone_cells", image, result, sel)
    _cell("tone_cells", cell)
    y = out_tensor("tone_cells", out, (B, 4, -(-H // cell), -(-W // cell)), torch.int32, image.device)
    _l.check(_l.load().pbe_tone_cells_i32(_p(image), _p(result), _p(sel), _p(y), B, H, W, int(cell), _stream()), "pbe_tone_cells_i32")
    return y


def tone_field(cells: torch.Tensor, cell: int = 8, limit: float = 0.125, min_pixels: int = 64, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cells int32 [B, 4, Hc, Wc] (tone_cells at the same `cell`) -> fp32 [B, 3, Hc, Wc] on the device: the pull-push fill of
    pbe_tone_field_f32 (include/pbe_hip.h), in [0, 1] units, every cell mean clamped to +-limit (a blended value may pass it by a rounding).  A sample with fewer than min_pixels selected
    pixels (and with none, always) gets zeros.  One launch; every element is written; the same bits from run to run."""
    _req(cells, torch.int32, "tone_field cells")
    if cells.dim() != 4 or cells.shape[1] != 4 or cells.numel() == 0 or cells.shape[0] > 65535 or not cells.is_contiguous():
        raise _l.PbeError(f"tone_field: cells must be a contiguous int32 [B, 4, Hc, Wc] tensor with B in 1 .. 65535, got {tuple(cells.shape)}")
    B, _, Hc, Wc = (int(v) for v in cells.shape)
    if max(Hc, Wc) > 4096 or Hc * Wc > 1 << 20:
        raise _l.PbeError(f"tone_field: a grid of {Hc} x {Wc} cells: edges up to 4096 and at most 2^20 cells (one workgroup walks a sample's pyramid); "
                          "take a larger cell")
    _cell("tone_field", cell)
    try:
        lim = float(limit)
    except (TypeError, ValueError) as e:
        raise _l.PbeError(f"tone_field: limit must be a finite number > 0, got {limit!r}") from e
    lim = C.c_float(lim).value if math.isfinite(lim) else lim                # the fp32 value the kernel receives
    if not (lim > 0.0) or not math.isfinite(lim):
        raise _l.PbeError(f"tone_field: limit must be a finite number > 0 (in fp32), got {limit!r}")
    if isinstance(min_pixels, bool) or int(min_pixels) != min_pixels or not (0 <= min_pixels < 1 << 31):
        raise _l.PbeError(f"tone_field: min_pixels must be an integer >= 0, got {min_pixels!r}")
    y = out_tensor("tone_field", out, (B, 3, Hc, Wc), torch.float32, cells.device)
    lib = _l.load()
    ws = workspace(cells.device, "tone_field", lib.pbe_tone_field_workspace_bytes(B, Hc, Wc), 1 << 16)
    _l.check(lib.pbe_tone_field_f32(_p(cells), _p(y), B, Hc, Wc, int(cell), lim, int(min_pixels), _p(ws), ws.numel(), _stream()), "pbe_tone_field_f32")
    return y


# ---- holes of a mask (csrc/holes.hip): connected components, their boxes, the mask of some of them -----------------------------------
def _plane_args(what: str, plane: torch.Tensor, dtype) -> Tuple[int, int]:
    """(Hs, Ws) of a contiguous [Hs, Ws] tensor of `dtype` on the GPU with edges up to 16384."""
    _req(plane, dtype, what)
    if plane.dim() != 2 or not plane.is_contiguous() or plane.numel() == 0 or max(plane.shape) > 16384:
        raise _l.PbeError(f"{what}: expected a contiguous {dtype} [Hs, Ws] tensor with edges in 1 .. 16384, got {tuple(plane.shape)} with strides "
                          f"{tuple(plane.stride())}")
    return int(plane.shape[0]), int(plane.shape[1])


def mask_components(mask: torch.Tensor, connectivity: int = 8, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [Hs, Ws] mask (a byte >= 128 is a hole pixel) -> labels int32 [Hs, Ws]: -1 off the hole, else the smallest linear index
    y * Ws + x of the pixel's connected component (connectivity 8: diagonal neighbours join; or 4).  Unique, whatever the order of the
    kernel's atomics."""
    Hs, Ws = _plane_args("mask_components mask", mask, torch.uint8)
    if connectivity not in (4, 8):
        raise _l.PbeError(f"mask_components: connectivity must be 8 or 4, got {connectivity!r}")
    y = out_tensor("mask_components", out, (Hs, Ws), torch.int32, mask.device)
    lib = _l.load()
    ws = workspace(mask.device, "holes", lib.pbe_mask_components_workspace_bytes(Hs, Ws), 1 << 16)
    _l.check(lib.pbe_mask_components_u8_i32(_p(mask), _p(y), Hs, Ws, int(connectivity), _p(ws), ws.numel(), _stream()), "pbe_mask_components_u8_i32")
    return y


def component_boxes(labels: torch.Tensor, capacity: int = 4096):
    """labels int32 [Hs, Ws] of mask_components -> (count, table): table an int64 numpy [count, 6] array of (label, ya, yb, xa, xb, area)
    per component, bounds inclusive, SORTED BY LABEL (the raster order of each component's first pixel).  The one read-back of the
    per-hole path: 4 + 24 capacity bytes, not the mask.  More than `capacity` components raise PbeError."""
    import numpy as np
    Hs, Ws = _plane_args("component_boxes labels", labels, torch.int32)
    cap = int(capacity)
    if cap != capacity or cap < 1 or cap > (1 << 20):
        raise _l.PbeError(f"component_boxes: capacity must be an integer in 1 .. {1 << 20}, got {capacity!r}")
    lib = _l.load()
    ws = workspace(labels.device, "holes", lib.pbe_component_boxes_workspace_bytes(Hs, Ws, cap), 1 << 16)
    buf = torch.empty(6 * cap + 1, dtype=torch.int32, device=labels.device)                 # the table, then the count
    _l.check(lib.pbe_component_boxes_i32(_p(labels), _p(buf), buf.data_ptr() + 24 * cap, Hs, Ws, cap, _p(ws), ws.numel(), _stream()),
             "pbe_component_boxes_i32")
    count = int(buf[6 * cap:].cpu()[0])
    if count > cap:
        raise _l.PbeError(f"component_boxes: the mask has {count} components, more than capacity = {cap}: raise the `capacity` argument")
    table = buf[:6 * count].cpu().numpy().astype(np.int64).reshape(count, 6)
    return count, table[np.argsort(table[:, 0], kind="stable")]


def select_components(labels: torch.Tensor, wanted, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels int32 [Hs, Ws], wanted: up to 4096 labels (any order, on the host or the device) -> uint8 [Hs, Ws]: 255 where the pixel's
    label is one of them, else 0 - the mask of those holes alone."""
    Hs, Ws = _plane_args("select_components labels", labels, torch.int32)
    w = torch.as_tensor(wanted).reshape(-1)
    if w.numel() and (w.is_floating_point() or w.dtype == torch.bool):
        raise _l.PbeError(f"select_components: wanted must hold integer labels, got {w.dtype}")
    if w.numel() > 4096:
        raise _l.PbeError(f"select_components: {w.numel()} labels wanted, at most 4096 allowed")
    w = torch.sort(w.to(torch.int32)).values.to(labels.device).contiguous()
    y = out_tensor("select_components", out, (Hs, Ws), torch.uint8, labels.device)
    _l.check(_l.load().pbe_select_components_u8(_p(labels), _p(w) if w.numel() else None, w.numel(), _p(y), Hs, Ws, _stream()), "pbe_select_components_u8")
    return y


# ---- the shape of a mask (csrc/maskshape.hip): the exact squared Euclidean distance map, grow / shrink / close / open by a disc, boxes ----
MASK_RMAX = 2047


def _radius(what: str, r, signed: bool):
    """r as an exact rational, or PbeError unless it is a finite real in -2047 .. 2047 (signed) or 0 .. 2047."""
    import numbers
    from fractions import Fraction
    lo = -MASK_RMAX if signed else 0
    try:
        if isinstance(r, bool) or not isinstance(r, numbers.Real):
            raise TypeError(type(r))
        # the exact value of a float (numpy's scalars go through Python's); nan and inf raise
        f = r if isinstance(r, Fraction) else Fraction(int(r) if isinstance(r, numbers.Integral) else float(r))
    except (TypeError, ValueError, OverflowError) as e:
        raise _l.PbeError(f"{what} must be a real number in {lo} .. {MASK_RMAX}, got {r!r}") from e
    if f < lo or f > MASK_RMAX:
        raise _l.PbeError(f"{what} must be a real number in {lo} .. {MASK_RMAX}, got {r!r}")
    return f


def mask_dist2(mask: torch.Tensor, to_hole: bool = True, rmax: int = MASK_RMAX, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [Hs, Ws] mask (a byte >= 128 is a hole pixel) -> int32 [Hs, Ws]: the squared Euclidean distance to the nearest hole pixel
    (to_hole) or the nearest non-hole pixel (not to_hole) of the picture, exact, saturated at rmax^2 + 1 (0 <= rmax <= 2047).  The
    outside of the picture belongs to neither set; an empty set gives rmax^2 + 1 everywhere.  A pixel farther than rmax from the set
    costs 2 rmax + 1 taps: give the rmax you need."""
    Hs, Ws = _plane_args("mask_dist2 mask", mask, torch.uint8)
    f = _radius("mask_dist2: rmax", rmax, False)
    if f.denominator != 1:
        raise _l.PbeError(f"mask_dist2: rmax must be an integer in 0 .. {MASK_RMAX}, got {rmax!r}")
    rm = int(f)
    y = out_tensor("mask_dist2", out, (Hs, Ws), torch.int32, mask.device)
    lib = _l.load()
    ws = workspace(mask.device, "maskshape", lib.pbe_mask_dist2_workspace_bytes(Hs, Ws), 1 << 16)
    _l.check(lib.pbe_mask_dist2_u8_i32(_p(mask), _p(y), Hs, Ws, 1 if to_hole else 0, rm, _p(ws), ws.numel(), _stream()), "pbe_mask_dist2_u8_i32")
    return y


def mask_grow(mask: torch.Tensor, r, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [Hs, Ws] mask, r a real in -2047 .. 2047 -> uint8 [Hs, Ws] in {0, 255}: the hole grown by the disc of radius r, i.e. every
    pixel whose squared distance to a hole pixel is <= floor(r^2) (r = 1: the 4-neighbour cross, 1.5: the 3 x 3 square, 2: the 13-pixel
    disc); r < 0 shrinks it: the pixels whose squared distance to a non-hole pixel of the picture is > floor(r^2) - the picture's border
    does not erode.  r = 0 is the mask binarised.  The distance map is taken with rmax = ceil(|r|)."""
    Hs, Ws = _plane_args("mask_grow mask", mask, torch.uint8)
    f = _radius("mask_grow: r", r, True)
    y = out_tensor("mask_grow", out, (Hs, Ws), torch.uint8, mask.device)
    t2, rm = int(f * f // 1), int(-((-abs(f)) // 1))                                 # floor(r^2), ceil(|r|): exact, r is a rational
    d2 = workspace(mask.device, "maskshape d2", 4 * Hs * Ws, 1 << 16)[:4 * Hs * Ws].view(torch.int32).view(Hs, Ws)      # kept per device, not allocated per call
    mask_dist2(mask, f >= 0, rm, out=d2)
    _l.check(_l.load().pbe_mask_from_dist2_u8(_p(d2), _p(y), Hs, Ws, t2, 0 if f >= 0 else 1, _stream()), "pbe_mask_from_dist2_u8")
    return y


def _grow_and_back(what: str, mask: torch.Tensor, r, first: int, out: Optional[torch.Tensor]) -> torch.Tensor:
    """mask_grow by first * r, then by -first * r (first = 1: close, -1: open), r in 0 .. 2047."""
    f = _radius(f"{what}: r", r, False)
    Hs, Ws = _plane_args(f"{what} mask", mask, torch.uint8)
    if out is not None:
        out_tensor(what, out, (Hs, Ws), torch.uint8, mask.device)          # refused before the first stage runs
    return mask_grow(mask_grow(mask, first * f), -first * f, out=out)


def mask_close(mask: torch.Tensor, r, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mask_grow(mask_grow(mask, r), -r), r in 0 .. 2047: gaps and pits narrower than the disc are filled, nothing is removed."""
    return _grow_and_back("mask_close", mask, r, 1, out)


def mask_open(mask: torch.Tensor, r, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mask_grow(mask_grow(mask, -r), r), r in 0 .. 2047: specks and spurs narrower than the disc are removed, nothing is added."""
    return _grow_and_back("mask_open", mask, r, -1, out)


def fill_boxes(boxes, shape, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """boxes: anything torch.as_tensor takes, integers [n, 4] with rows (ya, yb, xa, xb), bounds inclusive (component_boxes' columns
    1 .. 4), 0 <= n <= 4096, on the host or the device; shape = (Hs, Ws) -> uint8 [Hs, Ws]: 255 inside any box, else 0.  A row that is
    not a box inside the picture raises: rows on the host are checked here, rows on the device by the entry point alone.  BLOCKS: the
    entry point reads the rows back to refuse a bad one before it launches, so this call waits for the current stream (once).  The
    result lives on `out`'s device, else `device`, else the boxes' GPU, else the current one."""
    try:
        Hs, Ws = (int(v) for v in shape)
        exact = len(tuple(shape)) == 2 and all(int(v) == v for v in shape)
    except (TypeError, ValueError) as e:
        raise _l.PbeError(f"fill_boxes: shape must be two integers (Hs, Ws), got {shape!r}") from e
    if not exact or Hs < 1 or Ws < 1 or max(Hs, Ws) > 16384:
        raise _l.PbeError(f"fill_boxes: shape (Hs, Ws) = {tuple(shape)!r} must have edges in 1 .. 16384")
    b = torch.as_tensor(boxes)
    if b.numel() and (b.is_floating_point() or b.is_complex() or b.dtype == torch.bool):
        raise _l.PbeError(f"fill_boxes: boxes must hold integers, got {b.dtype}")
    if (b.dim() != 2 or b.shape[1] != 4) and b.numel():
        raise _l.PbeError(f"fill_boxes: boxes must be [n, 4] rows (ya, yb, xa, xb), got {tuple(b.shape)}")
    n = b.numel() // 4
    if n > 4096:
        raise _l.PbeError(f"fill_boxes: {n} boxes, at most 4096 allowed")
    if not b.is_cuda:                                                                # (rows on the device: the entry point's read-back is the one check)
        host = b.detach().to(torch.int64).reshape(n, 4)
        bad = (host[:, 0] < 0) | (host[:, 0] > host[:, 1]) | (host[:, 1] >= Hs) | (host[:, 2] < 0) | (host[:, 2] > host[:, 3]) | (host[:, 3] >= Ws)
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            raise _l.PbeError(f"fill_boxes: box {i} (ya, yb, xa, xb) = {tuple(host[i].tolist())} is not a box inside the {Hs} x {Ws} picture")
    if out is not None:
        dev = out.device
    elif device is not None:
        dev = torch.device(device)
    else:
        dev = b.device if b.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _l.PbeError(f"fill_boxes: the result must live on a GPU, got {dev}")
    y = out_tensor("fill_boxes", out, (Hs, Ws), torch.uint8, dev)
    d = b.detach().reshape(n, 4).to(device=dev, dtype=torch.int64).clamp(-1, 1 << 20).to(torch.int32).contiguous()        # (the clamp: no wrap into range; both ends are refused)
    _l.check(_l.load().pbe_fill_boxes_u8(_p(d) if n else None, n, _p(y), Hs, Ws, _stream()), "pbe_fill_boxes_u8")
    return y


# ---- the exemplar cut from a picture (csrc/exemplar.hip): Pillow's 8-bit resize on the device, the box of a mask ----------------------
MASK_BOX_BAND = 32            # rows of one band of pbe_mask_box_i32


def resample_u8(picture: torch.Tensor, out_hw, box=None, filter: str = "bicubic", mask: Optional[torch.Tensor] = None, fill=None, mean=None, std=None,
                out: Optional[torch.Tensor] = None, out_planes: Optional[torch.Tensor] = None):
    """uint8 [Hs, Ws, 3] picture on the GPU -> (uint8 [oh, ow, 3], planes): the bytes of Pillow's
    Image.resize((ow, oh), filter, box=box) - its fixed-point arithmetic restated (pbe_amd.exemplar.resample_tables on the host, the two
    integer passes on the device), filter "bicubic" (Image.resize's default), "bilinear" or "lanczos".  box: Pillow's (x0, y0, x1, y1),
    floats allowed, None = the whole picture.  mask uint8 [Hs, Ws] with fill (three bytes): a pixel whose mask byte is < 128 reads as
    `fill`.  mean / std (three floats each): planes = fp32 [3, oh, ow] = (byte / 255 - mean) / std with u8_to_planes' bits; else None.
    As Pillow does, a pass whose axis keeps its size under a box that spans it is skipped: zero, one or two resampling launches (with
    none, one copying launch), plus pbe_u8_to_planes_f32 where the last launch is the horizontal pass.  The horizontal pass runs first,
    except under Image.resize's rule for very tall pictures (pbe_amd.exemplar.vertical_first)."""
    from . import exemplar as _ex
    Hs, Ws = _picture_args("resample_u8 picture", picture, 3)
    try:
        oh, ow = (int(v) for v in out_hw)
        exact = len(tuple(out_hw)) == 2 and all(int(v) == v for v in out_hw)
    except (TypeError, ValueError) as e:
        raise _l.PbeError(f"resample_u8: out_hw must be two integers (oh, ow), got {out_hw!r}") from e
    if not exact or min(oh, ow) < 1 or max(oh, ow, Hs, Ws) > 16384:
        raise _l.PbeError(f"resample_u8: output {out_hw!r} and picture {Hs} x {Ws} must have edges in 1 .. 16384")
    x0, y0, x1, y1 = _ex.validate_box(box, (Hs, Ws))
    fill3 = None
    if (mask is None) != (fill is None):
        raise _l.PbeError("resample_u8: mask and fill go together (fill is the colour of the pixels whose mask byte is < 128)")
    if mask is not None:
        _picture_args("resample_u8 mask", mask, 1)
        if tuple(mask.shape) != (Hs, Ws) or mask.device != picture.device:
            raise _l.PbeError(f"resample_u8: the mask is {tuple(mask.shape)} on {mask.device}, the picture {Hs} x {Ws} on {picture.device}")
        fill3 = (C.c_uint8 * 3)(*_ex._fill3(fill))
    if (mean is None) != (std is None):
        raise _l.PbeError("resample_u8: mean and std go together")
    dev = picture.device
    y = out_tensor("resample_u8", out, (oh, ow, 3), torch.uint8, dev)
    planes, m, sd = None, None, None
    if mean is not None:
        planes = out_tensor("resample_u8 planes", out_planes, (3, oh, ow), torch.float32, dev)
        m, sd = floats3(mean), floats3(std)
    elif out_planes is not None:
        raise _l.PbeError("resample_u8: out_planes needs mean and std")
    need_h = ow != Ws or x0 != 0.0 or x1 != ow                   # Pillow's need_horizontal / need_vertical
    need_v = oh != Hs or y0 != 0.0 or y1 != oh
    lib = _l.load()

    def up(a):
        return torch.from_numpy(a).to(dev)
    def ws(rows, cols):
        need = lib.pbe_resample_workspace_bytes(rows, cols)
        if need < rows * cols * 3:
            raise _l.PbeError(f"resample_u8: no workspace for an intermediate of {rows} x {cols}")
        return torch.empty(need, dtype=torch.uint8, device=dev)
    def after_h():
        """What follows a horizontal pass that wrote y: the planes of y's bytes (the vertical pass writes them itself)."""
        if planes is not None:
            _l.check(lib.pbe_u8_to_planes_f32(_p(y), _p(planes), 1, 3, oh * ow, m, sd, 0, _stream()), "pbe_u8_to_planes_f32")
        return y, planes
    bv, kv = _ex.resample_tables(Hs, y0, y1, oh, filter) if need_v else _ex.identity_tables(oh)
    src, src_mask, rows = picture, mask, Hs
    if need_h and _ex.vertical_first(Hs, Ws, oh):                 # Image.resize's rule for very tall pictures: the height first, over the full width
        bh, kh = _ex.resample_tables(Ws, x0, x1, ow, filter)
        tmp, dbv, dkv, dbh, dkh = ws(oh, Ws), up(bv), up(kv), up(bh), up(kh)
        _l.check(lib.pbe_resample_v_u8(_p(picture), _p(mask), fill3, _p(tmp), None, Hs, Ws, oh, _p(dbv), _p(dkv), kv.shape[1], None, None, _stream()),
                 "pbe_resample_v_u8")
        _l.check(lib.pbe_resample_h_u8(_p(tmp), None, None, _p(y), oh, Ws, 0, oh, ow, _p(dbh), _p(dkh), kh.shape[1], _stream()), "pbe_resample_h_u8")
        return after_h()
    if need_h:
        bh, kh = _ex.resample_tables(Ws, x0, x1, ow, filter)
        first, last = (int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])) if need_v else (0, Hs)      # the rows the vertical pass reads
        bv = bv.copy()
        bv[:, 0] -= first
        rows = last - first
        tmp = ws(rows, ow) if need_v else y
        dbh, dkh = up(bh), up(kh)
        _l.check(lib.pbe_resample_h_u8(_p(picture), _p(mask), fill3, _p(tmp), Hs, Ws, first, last, ow, _p(dbh), _p(dkh), kh.shape[1], _stream()),
                 "pbe_resample_h_u8")
        src, src_mask = tmp, None
        if not need_v:
            return after_h()
    dbv, dkv = up(bv), up(kv)
    _l.check(lib.pbe_resample_v_u8(_p(src), _p(src_mask), fill3 if src_mask is not None else None, _p(y), _p(planes), rows, ow, oh, _p(dbv), _p(dkv),
                                   kv.shape[1], m, sd, _stream()), "pbe_resample_v_u8")
    return y, planes


def mask_box(mask: torch.Tensor):
    """uint8 [Hs, Ws] mask on the GPU -> (ya, yb, xa, xb), inclusive: the bounding box of the bytes >= 128 (window.hole_box's, without
    bringing the mask to the host), or None where there is none.  One workgroup per band of 32 rows writes its own box; the
    ceil(Hs / 32) x 4 integers are read back and reduced here.  BLOCKS on that read-back."""
    Hs, Ws = _plane_args("mask_box mask", mask, torch.uint8)
    lib = _l.load()
    bands = lib.pbe_mask_box_bands(Hs)
    table = torch.empty((bands, 4), dtype=torch.int32, device=mask.device)
    _l.check(lib.pbe_mask_box_i32(_p(mask), _p(table), Hs, Ws, bands, _stream()), "pbe_mask_box_i32")
    t = table.cpu().numpy()
    t = t[t[:, 1] >= 0]
    if t.shape[0] == 0:
        return None
    return int(t[:, 0].min()), int(t[:, 1].max()), int(t[:, 2].min()), int(t[:, 3].max())
