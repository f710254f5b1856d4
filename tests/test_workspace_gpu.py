"""The per-device scratch of pbe_amd.ops: every wrapper that needs scratch keeps ONE uint8 buffer per device in ops._ws under the key
(device index, name), at least the name's floor long, and reuses it from call to call.  tests/test_tone_gpu.py and
tests/test_tone_field_gpu.py poison their scratch by that key; this is the contract they rely on, for all eight names."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOORS = {"gn": 1 << 21, "feather": 1 << 20, "tone": 1 << 16, "tone_field": 1 << 16, "holes": 1 << 16, "maskshape": 1 << 16, "maskshape d2": 1 << 16}


def test_every_scratch_buffer_is_keyed_floored_and_kept(dev):
    from pbe_amd import ops
    m = np.zeros((40, 56), np.uint8)
    m[8:12, 10:15] = 255
    m[25:28, 40:44] = 200
    mask = torch.from_numpy(m).to(dev)
    g = torch.Generator().manual_seed(5)
    image = (torch.rand(1, 3, 16, 24, generator=g) * 2 - 1).to(dev)
    result = torch.rand(1, 3, 16, 24, generator=g).to(dev)
    sel = torch.ones(1, 1, 16, 24, device=dev)
    x = torch.randn(3, 64, 64, generator=g).half().to(dev)                            # test_groupnorm's (3, 64, 64)
    gamma, beta = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    a, w = torch.randn(64, 8, generator=g).half().to(dev), torch.randn(64, 8, generator=g).half().to(dev)      # test_gemm_shapes' (64, 64, 8)

    def every_wrapper():
        ops.feather_alpha(mask, (4, 4, 24, 32), 2)
        labels = ops.mask_components(mask)
        count, _ = ops.component_boxes(labels)
        assert count == 2
        ops.mask_dist2(mask)
        ops.mask_grow(mask, 1.5)
        ops.tone_stats(image, result, sel)
        cells = ops.tone_cells(image, result, sel, cell=4)
        ops.tone_field(cells, cell=4)
        ops.groupnorm(x, gamma, beta, 1e-6, False)
        ops.gemm(a, w)

    every_wrapper()
    assert dev.index == 0
    entries = {}
    for name in ("splitk", *FLOORS):
        assert (0, name) in ops._ws, f"no scratch under (0, {name!r}): {sorted(ops._ws)}"
        ws = entries[name] = ops._ws[(0, name)]
        assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.device == dev, (name, ws.dtype, tuple(ws.shape), ws.device)
        assert ws.numel() >= FLOORS.get(name, ops.SPLITK_WS_BYTES), (name, ws.numel())
    assert entries["splitk"].numel() == ops.SPLITK_WS_BYTES
    ptrs = {name: ws.data_ptr() for name, ws in entries.items()}
    every_wrapper()
    torch.cuda.synchronize()
    assert {name: ops._ws[(0, name)].data_ptr() for name in ptrs} == ptrs, "a scratch buffer was allocated again by the second call"
