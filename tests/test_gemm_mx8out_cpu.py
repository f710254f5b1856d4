"""CPU side of the MX-fp8 projection output (pbe_gemm_mx8out_f16): the descriptor layout and the host-only plan query.  No kernel is
launched; the plan query never dereferences an operand, so stand-in pointers describe the problems."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20                                          # 16-byte aligned stand-in address (never read)
TOKENS, VT = 0, 1


def _lib():
    from pbe_amd import lib
    return lib, lib.load()


def _qkv_problem(M, C_, B, N, D, tile_cfg=-1):
    """The LayerNorm-folded q | k | v^T projection: x [M, C], w [3 C, C], inner = C = H D."""
    lib, _ = _lib()
    d = lib.GemmDesc(P, None, P, None, None, None, None, M, 3 * C_, C_, C_, C_, 0, C_, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1.0, 0, 0, None, 0, tile_cfg)
    d.alpha_cols, d.ln_stats, d.ln_parts, d.ln_stats_ld, d.ln_colsum, d.ln_eps = C_, P, 1, M, P, 1e-5
    d.vt_col0, d.vt_tokens = 2 * C_, N
    mx = lib.Mx8OutDesc()
    mx.nranges, mx.channel_rows = 3, 0
    for i, (lay, c0) in enumerate(((TOKENS, 0), (TOKENS, C_), (VT, 2 * C_))):
        mx.r[i] = lib.Mx8OutRange(P, P, lay, c0, 1.0, B, C_ // D, N, D)
    return d, mx


def _f8_qk_problem(M, C_, B, N, D, tile_cfg=-1):
    lib, _ = _lib()
    d = lib.GemmDesc(P, None, P, None, None, None, None, M, 2 * C_, C_, C_, C_, 0, C_, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1.0, 0, 0, None, 0, tile_cfg,
                     P, P, 0, 0, 1)
    mx = lib.Mx8OutDesc()
    mx.nranges, mx.channel_rows = 2, 0
    mx.r[0] = lib.Mx8OutRange(P, P, TOKENS, 0, 0.1, B, C_ // D, N, D)
    mx.r[1] = lib.Mx8OutRange(P, P, TOKENS, C_, 1.0, B, C_ // D, N, D)
    return d, mx


def _f8_vt_problem(C_, B, N, D, tile_cfg=-1):
    lib, _ = _lib()
    d = lib.GemmDesc(P, None, P, None, None, None, None, C_, N, C_, C_, C_, 0, C_, 0, 0, 0, 0, 0, N * C_, 0, 0, B, 1.0, 0, 0, None, 0, tile_cfg,
                     P, P, 0, N, 1)
    mx = lib.Mx8OutDesc()
    mx.nranges, mx.channel_rows = 1, 1
    mx.r[0] = lib.Mx8OutRange(P, P, VT, 0, 1.0, B, C_ // D, N, D)
    return d, mx


def _plan(d, mx):
    lib, h = _lib()
    out = (C.c_int32 * 6)()
    rc = h.pbe_gemm_mx8out_plan(C.byref(d), C.byref(mx), out)
    return rc, list(out)


def _tokens_whole(bn, width, D, half):
    """Every column-tile boundary inside a TOKENS range of `width` columns is an MX block boundary (h D + 32 j)."""
    step = bn // 2 if half else bn
    return all((x % D) % 32 == 0 for x in range(step, width, step))


def test_sizeof_mx8_out_desc_matches_library():
    lib, h = _lib()
    assert C.sizeof(lib.Mx8OutDesc) == h.pbe_sizeof_mx8_out_desc()


def _tuned():
    with open(os.path.join(ROOT, "pbe_amd", "tuned_mi355x.json")) as f:
        return json.load(f)


# the q|k|v^T projection keys of the tuned table: gx:M:3C:C:1 with C = 320 / 640 / 1280 (d = 40 / 80 / 160, 8 heads)
QKV_KEYS = sorted(k for k in _tuned() if k.startswith("gx:") and k.split(":")[2] == str(3 * int(k.split(":")[3])) and k.split(":")[3] in ("320", "640", "1280"))


def test_tuned_tiles_that_split_a_block_are_replaced():
    """gx:4096:1920:640:1 / gx:2048:1920:640:1 name 128-column tiles at d = 80 (128 = 80 + 48): the MX form plans an aligned tile instead,
    and the tuned A-stationary tile stays where it runs (K = 320 at batch >= 8)."""
    from pbe_amd import ops
    assert len(QKV_KEYS) >= 10
    for key in ("gx:4096:1920:640:1", "gx:2048:1920:640:1"):
        M = int(key.split(":")[1])
        d, mx = _qkv_problem(M, 640, 1, M, 80)
        assert _plan(d, mx)[0] == 0
        d.tile_cfg = _tuned()[key]
        assert _plan(d, mx)[0] == -1                  # requested explicitly: refused
        d.tile_cfg = ops._mx8_tile_cfg(d, mx, key, 80)
        rc, out = _plan(d, mx)
        assert rc == 0 and out[0] != (_tuned()[key] & 255) and _tokens_whole(out[3], 640, 80, False), (key, out)
    for key in ("gx:32768:960:320:1", "gx:73728:960:320:1"):
        M = int(key.split(":")[1])
        d, mx = _qkv_problem(M, 320, 8, M // 8, 40)
        d.tile_cfg = ops._mx8_tile_cfg(d, mx, key, 40)
        assert _plan(d, mx)[1][0] == 20, key


@pytest.mark.parametrize("key", QKV_KEYS)
def test_plan_keeps_blocks_whole_on_tuned_qkv_shapes(key):
    from pbe_amd import ops
    _, M, Nc, C_, _ = key.split(":")
    M, C_ = int(M), int(C_)
    D = C_ // 8
    tuned = _tuned()[key]
    d, mx = _qkv_problem(M, C_, 1, M, D)
    d.tile_cfg = ops._mx8_tile_cfg(d, mx, key, D)
    rc, out = _plan(d, mx)
    assert rc == 0, key
    cfg, splits, bm, bn = out[:4]
    assert splits == 1
    assert _tokens_whole(bn, C_, D, cfg == 20) and (2 * C_) % bn == 0 and bm % 32 == 0, (key, out)
    if (tuned & 255) == 20:                          # the A-stationary tile stays the choice where it runs today (K = 320)
        assert cfg == 20, (key, out)
    # a requested tile that splits a block is refused, never replaced
    bad = 3 if D != 160 else None                    # 128 columns: 128 = 3 * 40 + 8, 128 = 80 + 48
    if bad is not None:
        d.tile_cfg = bad | (1 << 8)
        assert _plan(d, mx)[0] == -1


@pytest.mark.parametrize("C_,N,B", [(320, 4096, 1), (640, 1024, 2), (1280, 256, 4), (1280, 64, 2), (320, 9216, 1), (640, 2304, 3), (1280, 576, 1)])
def test_plan_fp8_forms(C_, N, B):
    D = C_ // 8
    d, mx = _f8_qk_problem(B * N, C_, B, N, D)
    rc, out = _plan(d, mx)
    assert rc == 0 and out[1] == 1 and _tokens_whole(out[3], C_, D, False) and C_ % out[3] == 0, out
    d, mx = _f8_vt_problem(C_, B, N, D)
    rc, out = _plan(d, mx)
    assert rc == 0 and out[1] == 1 and out[3] % 32 == 0 and out[4] == -(-C_ // out[2]) * -(-N // out[3]) * B, out


def _refused(d, mx, msg):
    _, h = _lib()
    rc = _plan(d, mx)[0]
    err = h.pbe_last_error().decode()
    assert rc == -1 and msg in err, (msg, rc, err)


def test_plan_refuses():
    # N % 64 != 0 (the 12x12 mid block at 768: N = 144)
    _refused(*_qkv_problem(144, 1280, 1, 144, 160), "multiple of 64")
    _refused(*_f8_vt_problem(1280, 2, 144, 160), "multiple of 64")
    # head dims pbe_attention_mx8 does not take
    for D in (64, 32, 120):
        _refused(*_qkv_problem(4096, 8 * D, 1, 4096, D), "head dim")
    # split-K, residual, GEGLU, row statistics, an explicitly requested tile that splits a block
    for field, value, msg in (("tile_cfg", 8 | (2 << 8), "split-K"), ("resid", P, "no residual"), ("act", 4, "no activation (GEGLU"),
                              ("row_stats_out", P, "no row statistics"), ("tile_cfg", 3, "splits an MX block")):
        d, mx = _qkv_problem(4096, 320, 1, 4096, 40)
        setattr(d, field, value)
        _refused(d, mx, msg)
    # an fp16 problem without the LayerNorm fold, and ranges that disagree
    d, mx = _qkv_problem(4096, 320, 1, 4096, 40)
    d.ln_stats = None
    _refused(d, mx, "LayerNorm-folded")
    d, mx = _qkv_problem(4096, 320, 1, 4096, 40)
    mx.r[1].D = 80
    _refused(d, mx, "differ from range 0")
    d, mx = _qkv_problem(4096, 320, 1, 4096, 40)
    assert _plan(d, mx)[0] == 0


@pytest.mark.parametrize("keep", [(0, 1), (1, 2), (0,), (2,), (0, 2)])
def test_fp16_form_needs_all_three_ranges(keep):
    """The fp16 form takes exactly q | k | V^T (the A-stationary tile's form 2 counts on every column tile storing), also where tile 20 is
    requested (M = 32 768, K = 320)."""
    lib, _ = _lib()
    d, mx = _qkv_problem(32768, 320, 8, 4096, 40, tile_cfg=20 | (1 << 8))
    rc, out = _plan(d, mx)
    assert rc == 0 and out[0] == 20, out
    rs = [lib.Mx8OutRange.from_buffer_copy(mx.r[i]) for i in keep]
    mx.nranges = len(rs)
    for i, r in enumerate(rs):
        mx.r[i] = r
    _refused(d, mx, "exactly the q")
