"""CPU side of the MX-fp8 attention core: the precision switch and the host reference quantiser (tests/mx8ref.py) that the GPU tests
hold pbe_quant_mx8_f16 to, checked against hand-computed OCP e4m3 / E8M0 values."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx8ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_attention_precision_on_meta_v1():
    from ldm.util import instantiate_from_config, load_yaml_config
    from pbe_amd.precision import set_attention_precision, set_linear_precision
    from ldm.modules.attention import BasicTransformerBlock
    cfg = load_yaml_config(os.path.join(ROOT, "configs", "v1.yaml"))
    with torch.device("meta"):
        model = instantiate_from_config(cfg["model"])
    for bad in ("fp32", "FP8", "e4m3", ""):
        with pytest.raises(ValueError):
            set_attention_precision(model, bad)
    blocks = [m for m in model.modules() if isinstance(m, BasicTransformerBlock)]
    assert set_attention_precision(model, "fp8") == 16 == len(blocks)
    assert all(b.attn1.attn_fp8 and not b.attn2.attn_fp8 and not b.linear_fp8 for b in blocks)
    assert set_linear_precision(model, "fp8") == 16
    assert set_attention_precision(model, "fp16") == 16
    assert all(not b.attn1.attn_fp8 and b.linear_fp8 for b in blocks)       # the two switches are independent


@pytest.mark.parametrize("y,code", [
    (1.0, 0x38), (0.5, 0x30), (-2.0, 0xC0), (448.0, 0x7E), (256.0, 0x78), (240.0, 0x77), (3.5, 0x46),
    (500.0, 0x7E), (-1e6, 0xFE), (464.0, 0x7E), (float("inf"), 0x7E),          # saturating, never NaN
    (1.0625, 0x38), (1.1875, 0x3A), (17.0, 0x58), (18.0, 0x59), (19.0, 0x5A),   # ties to even
    (2.0 ** -6, 0x08), (2.0 ** -9, 0x01), (7 * 2.0 ** -9, 0x07), (2.0 ** -10, 0x00), (3 * 2.0 ** -10, 0x02),   # subnormals
    (15 * 2.0 ** -10, 0x08), (0.013671875, 0x07), (1e-10, 0x00), (0.0, 0x00)])
def test_e4m3_encode_hand_values(y, code):
    assert int(R.e4m3_encode(np.float32(y))) == code
    if code & 0x7F != 0x7E or abs(y) == 448.0:
        assert R.e4m3_decode(code) == pytest.approx(np.float64(np.float32(y)), rel=2.0 ** -4, abs=2.0 ** -10)


def test_e4m3_round_trip_every_code():
    v = R.e4m3_values()
    codes = np.arange(256)
    ok = ~np.isnan(v) & (codes != 0x80)                    # -0 encodes as +0
    assert np.array_equal(R.e4m3_encode(v[ok].astype(np.float32)), codes[ok])
    assert v[0x7E] == 448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6


@pytest.mark.parametrize("amax,code", [(448.0, 127), (448.00003, 128), (449.0, 128), (0.0, 127), (1.0, 119), (1.75, 119),
                                       (1.7500001, 120), (2.0 ** -30, 89), (896.0, 128), (896.1, 129), (65504.0, 135)])
def test_e8m0_scale_hand_values(amax, code):
    assert int(R.scale_exp(np.float32(amax))) == code
    s = 2.0 ** (code - 127)
    if amax > 0:
        assert np.float32(amax) / s <= 448.0 < np.float32(amax) / (s / 2)    # the smallest such power of two


def test_reference_blocks_and_padding():
    """tokens layout at D = 40 (a second block of 8 + 24 zeros), an all-zero block, one outlier per block, head boundaries."""
    B, H, N, D = 1, 2, 3, 40
    x = np.zeros((B * N, H * D), dtype=np.float16)
    x[0, :D] = 1.0                                        # head 0: blocks amax 1 -> scale 2^-8 (code 119), bytes 256 -> 0x78
    x[0, 5] = 300.0                                       # outlier in block 0: scale 1 (code 127): 1 -> 0x38, 300 -> 288 (0x79)
    x[1, D + 33] = -3.0                                   # head 1, block 1, element 1
    codes, scales = R.quant_tokens(x, B, H, N, D)
    assert codes.shape == (3, 128) and scales.shape == (1, 2, 2, 64)
    assert list(scales[0, 0, :, 0]) == [127, 119] and codes[0, 5] == 0x79 and codes[0, 4] == 0x38 and codes[0, 32] == 0x78
    assert not codes[0, 40:64].any() and not codes[2].any() and (scales[0, :, :, 2] == 127).all() and (scales[0, :, :, 3:] == 127).all()
    assert scales[0, 1, 1, 1] == 120 and codes[1, 64 + 33] == 0xFC and not codes[1, :64].any()   # amax 3 = 1.5 * 2: scale 2^-7, -384 = -1.5 * 2^8
    dq = R.dequant_tokens(codes, scales, B, H, N, D)
    assert dq[0, 0, 0, 5] == 288.0 and dq[0, 1, 1, 33] == -3.0 and dq[0, 0, 0, 33] == 1.0


def test_reference_vt_layout():
    B, H, N, D = 1, 1, 70, 40
    x = np.zeros((D, 72), dtype=np.float16)
    x[3, 65] = 2.0 ** -12                                 # key block 2 (keys 64..95) of channel 3, fp16 normal, tiny
    x[39, :N] = np.arange(N, dtype=np.float16)
    codes, scales = R.quant_vt(x, B, H, N, D)
    assert codes.shape == (40, 128) and scales.shape == (1, 1, 4, 64)
    assert (scales[0, 0, :, 40:] == 127).all() and scales[0, 0, 3, 3] == 127 and not codes[:, N:].any()
    assert scales[0, 0, 2, 3] == 127 - 12 - 8 and codes[3, 65] == 0x78
    dv = R.dequant_vt(codes, scales, B, H, N, D)
    assert dv.shape == (1, 1, N, D) and dv[0, 0, 65, 3] == 2.0 ** -12
    # block amax 31: scale 2^-3 (31 * 8 = 248 <= 448 < 496); 4 significant bits: 17 -> 16, 19 -> 20, 21 -> 20 (ties to even), 31 -> 32
    want = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 18, 20, 20, 20, 22, 24, 24, 24, 26, 28, 28, 28, 30, 32]
    assert scales[0, 0, 0, 39] == 127 - 3 and np.array_equal(dv[0, 0, :32, 39], np.array(want, dtype=np.float64))
