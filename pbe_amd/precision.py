"""Operand precision of the U-Net's LayerNorm-fed linear projections (BASELINE configs[4]: "fp8 MFMA attention/linear path").

"fp16" (default): the reference's autocast precision - fp16 operands, fp32 accumulate.
"fp8":  in every BasicTransformerBlock the two LayerNorms emit OCP e4m3 with one scale per token (pbe_layernorm_f8) and the
        projections that read them - q|k, V^T and the GEGLU projection, 42 % of the linear FLOPs of a U-Net forward - run
        v_mfma_f32_16x16x32_fp8_fp8 on e4m3 weights with one scale per output channel (fp32 accumulate, scales applied in the
        epilogue).  The output projections, the convolutions, the VAE and CLIP stay fp16.
        Not the reference's precision: its results are held to a separate, re-validated tolerance (tests/test_model_gpu.py).

set_attention_precision switches the self-attention CORE (softmax(q k^T) v of every BasicTransformerBlock's attn1), independently:
"fp16" (default): pbe_attention_f16, fp16 operands, fp32 scores and softmax, P rounded to fp16.
"fp8":  q, k and V^T are quantised to MX-fp8 (OCP e4m3 with one power-of-two scale per 32 contraction elements, pbe_quant_mx8_f16)
        and both products run v_mfma_scale_f32_32x32x64_f8f6f4 (pbe_attention_mx8); P = exp2(s - m) <= 2^8 is rounded to e4m3 at
        scale 1 and shared by the numerator and the denominator.  attn2 (one-token context, no attention kernel) is unchanged.
        Where the q|k|v^T projection is the LayerNorm-folded fp16 launch (linear fp16) or the two fp8-operand launches (linear fp8),
        the projection writes the MX-fp8 operands itself (pbe_gemm_mx8out_f16: its epilogue quantises the fp16 values it would have
        stored), so no fp16 q|k / V^T is written and no quantiser runs; the bytes are those of the quantiser path, which stays for
        other shapes (N % 64 != 0), the unfolded projection and CrossAttention.mx8_from_projection = False (A/B runs).
        Tolerances: tests/test_attention_mx8_gpu.py.  Timing: tools/attn_mx8_ab.py.

Both switches, alone and together, are also held to a quantisation-aware fp64 reference (tests/q8ref.py: the same chain in exact
arithmetic with only the operand quantisations) - per block through q8ref.verdict, one full-size forward against
tests/golden/full_q8.npz (Q8_FWD_MEASURED) and the 50-step trajectory (Q8_TRAJ_MEASURED): tests/test_q8gate_gpu.py, DESIGN.md section 4.5.
"""
from __future__ import annotations

import torch


def set_linear_precision(model: torch.nn.Module, precision: str = "fp16") -> int:
    """Switch every BasicTransformerBlock under `model`; returns how many were switched."""
    from ldm.modules.attention import BasicTransformerBlock
    if precision not in ("fp16", "fp8"):
        raise ValueError(f"precision must be 'fp16' or 'fp8', got {precision!r}")
    n = 0
    for m in model.modules():
        if isinstance(m, BasicTransformerBlock):
            m.linear_fp8 = precision == "fp8"
            n += 1
    return n


def set_attention_precision(model: torch.nn.Module, precision: str = "fp16") -> int:
    """Switch the attention core of every BasicTransformerBlock's attn1 under `model`; returns how many were switched."""
    from ldm.modules.attention import BasicTransformerBlock
    if precision not in ("fp16", "fp8"):
        raise ValueError(f"precision must be 'fp16' or 'fp8', got {precision!r}")
    n = 0
    for m in model.modules():
        if isinstance(m, BasicTransformerBlock):
            m.attn1.attn_fp8 = precision == "fp8"
            n += 1
    return n
