"""The wrappers are three modules - pbe_amd.opsbase (shared helpers), pbe_amd.ops (model and sampler path), pbe_amd.ops_picture (uint8
pictures and masks) - but one namespace for their callers: every public name ops ever exported is still ops.X, the scratch dict is one
object, and opsbase.workspace is the one scratch cache."""
import types

import pytest
import torch

# sorted(n for n, v in vars(ops).items() if not n.startswith('_') and not a module), less Optional / Tuple / annotations, before the split
PUBLIC = [
    'ACT_GEGLU', 'ACT_GELU', 'ACT_NONE', 'ACT_QUICK_GELU', 'ACT_SILU', 'CTX_MAX_C', 'CTX_MAX_HJ', 'CTX_MAX_TOKENS', 'CtxOperands', 'GroupStats',
    'MASK_BOX_BAND', 'MASK_RMAX', 'MX8_TOKENS', 'MX8_VT', 'Mx8', 'RowStats', 'SPLITK_WS_BYTES', 'TONE_CELLS', 'USE_CONV_GROUP_STATS', 'attention',
    'attention_mx8', 'axpy_', 'bcast_row', 'clip_patchify', 'component_boxes', 'conv3x3', 'conv3x3_small', 'conv_kblock', 'conv_out_hw', 'ctx_attention',
    'ctx_attention_check', 'ctx_attention_map_check', 'ctx_map_gather', 'dpmpp_update', 'feather_alpha', 'fill_boxes', 'geglu', 'gemm', 'gemm_f8',
    'groupnorm', 'image_post', 'interleave_geglu', 'layernorm', 'layernorm_f8', 'mask_box', 'mask_close', 'mask_components', 'mask_dist2', 'mask_grow',
    'mask_open', 'mul_planes', 'nchw_to_nhwc', 'nhwc_to_nchw', 'pack_conv3x3', 'pack_conv3x3_up_phases', 'pack_geglu', 'pack_linear', 'pack_linear_f8',
    'pack_linear_ln', 'paste_window', 'philox_u32', 'pinned_batch_scale', 'planes_to_canvas', 'plms_pack_input', 'plms_update', 'posterior_sample',
    'prof_collect', 'prof_enable', 'prof_reset', 'qkv_fusable', 'qkv_mx8', 'qkv_mx8_f8', 'qsample_blend', 'quant_mx8', 'randn_seeded', 'resample_u8',
    'resize_bilinear', 'row_stats', 'scale_latent', 'seed_tensor', 'seed_words', 'select_components', 'softmax_rows', 'sub_tensor',
    'timestep_embedding', 'tone_cells', 'tone_field', 'tone_stats', 'tune', 'u8_to_planes', 'window_image', 'window_mask']


def test_ops_still_exports_every_public_name():
    from pbe_amd import ops, ops_picture
    assert len(PUBLIC) == 92 and len(set(PUBLIC)) == 92
    have = {n for n, v in vars(ops).items() if not n.startswith("_") and not isinstance(v, types.ModuleType)}
    assert not set(PUBLIC) - have, f"ops no longer exports {sorted(set(PUBLIC) - have)}"
    moved = [n for n in PUBLIC if n in vars(ops_picture)]
    assert sorted(moved) == sorted(ops_picture.__all__), "ops_picture.__all__ is not the public names it defines"
    assert {"TONE_CELLS", "MASK_RMAX", "MASK_BOX_BAND", "window_image", "tone_stats", "mask_grow", "resample_u8", "mask_box"} <= set(moved)
    for n in moved:
        assert getattr(ops, n) is getattr(ops_picture, n), f"ops.{n} is not ops_picture.{n}"
    for n in ("bcast_row", "randn_seeded", "philox_u32", "pack_conv3x3", "pack_linear", "gemm", "groupnorm", "plms_update"):
        assert n not in vars(ops_picture) and getattr(ops, n).__module__ == "pbe_amd.ops", n


def test_the_scratch_dict_and_the_hooks_live_where_tests_and_tools_set_them():
    from pbe_amd import ops, ops_picture, opsbase
    assert ops._ws is opsbase._ws
    assert isinstance(ops._splitk_ws, types.FunctionType) and ops._splitk_ws.__module__ == "pbe_amd.ops" and ops._splitk_ws.__globals__ is vars(ops)
    for n in ("_PLANS", "_TIMES", "_RECORD", "_FORCE_CFG", "_PIN_SCALE", "_PIN_CACHE", "_PIN_MISSES"):
        assert n in vars(ops), n
    for n in ("_launch", "_tile", "_plan", "_key", "_desc_key"):
        assert getattr(ops, n).__module__ == "pbe_amd.ops", n
    for mod in (ops, ops_picture):
        for n in ("_stream", "_p", "_req", "_f", "workspace"):
            assert getattr(mod, n) is getattr(opsbase, n), (mod.__name__, n)
    assert ops._h is opsbase._h


def test_workspace_is_one_buffer_per_device_and_name():
    from pbe_amd import opsbase
    cpu, a, b = torch.device("cpu"), "test_ops_modules a", "test_ops_modules b"
    try:
        first = opsbase.workspace(cpu, a, 100, 4096)
        assert first.dtype == torch.uint8 and tuple(first.shape) == (4096,) and first.device == cpu
        assert opsbase._ws[(cpu.index, a)] is first
        assert opsbase.workspace(cpu, a, 10, 4096) is first and opsbase.workspace(cpu, a, 4096, 4096) is first      # smaller or equal need: kept
        assert tuple(opsbase.workspace(cpu, b, 5000, 4096).shape) == (5000,)                                         # need above the floor
        assert tuple(opsbase.workspace(cpu, b, 7).shape) == (5000,)
        grown = opsbase.workspace(cpu, a, 4097, 4096)
        assert grown is not first and grown.numel() >= 4097 and opsbase._ws[(cpu.index, a)] is grown
        assert opsbase.workspace(cpu, a, 1) is grown
        other = opsbase._ws[(cpu.index, b)]
        assert other is not grown and other.data_ptr() != grown.data_ptr()
        assert tuple(opsbase.workspace(cpu, "test_ops_modules c", 33).shape) == (33,)                                # floor defaults to 0
    finally:
        for name in (a, b, "test_ops_modules c"):
            opsbase._ws.pop((cpu.index, name), None)
    assert not [k for k in opsbase._ws if str(k[1]).startswith("test_ops_modules")]


def test_out_tensor_and_floats3():
    from pbe_amd import opsbase
    from pbe_amd.lib import PbeError
    assert [round(v, 6) for v in opsbase.floats3((0.5, 1, 2.25))] == [0.5, 1.0, 2.25]
    with pytest.raises(PbeError, match="GPU"):                                   # a given `out` is checked like any operand: no CPU fallback
        opsbase.out_tensor("what", torch.zeros(2, 3), (2, 3), torch.float32, torch.device("cpu"))
