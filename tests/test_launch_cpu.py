"""CPU side of the shared tiled-launch path of pbe_amd.ops (_tile, _pinned, _desc_key): the tile a launch takes under pinned_batch_scale and
the cache of those decisions.  Only host-side plan queries run; stand-in pointers describe the problems (never dereferenced)."""
import ctypes as C

import pytest

P = 1 << 20                                          # 16-byte aligned stand-in address (never read)
TOKENS, VT = 0, 1


def _ops():
    from pbe_amd import lib, ops
    lib.load()
    return lib, ops


def _gemm(M, N, K, **kw):
    """2-D fp16 GEMM x [M, K] w [N, K] -> [M, N] with bias and split-K workspace, extra fields from kw."""
    lib, ops = _ops()
    d = lib.GemmDesc(P, None, P, P, P, None, None, M, N, K, K, K, 0, K, N, 0, 0, 0, 0, 0, 0, 0, 1, 1.0, 0, 0, P, ops.SPLITK_WS_BYTES, -1)
    for f, v in kw.items():
        setattr(d, f, v)
    return d


def _proj_in(B, N, C_):
    return _gemm(B * N, C_, C_), True                                      # + row statistics for the first block's LayerNorm


def _to_out(B, N, C_):
    return _gemm(B * N, C_, C_, rowvec=P, ldv=C_, group_rows=N, resid=P, ldr=C_), True


def _geglu(B, N, C_):
    return _gemm(B * N, 8 * C_, C_, ldc=4 * C_, act=4, ln_stats=P, ln_parts=5, ln_stats_ld=B * N, ln_colsum=P, ln_eps=1e-5), False


def _qkv(B, N, C_):
    return _gemm(B * N, 3 * C_, C_, ldc=2 * C_, bias=None, alpha_cols=C_, ln_stats=P, ln_parts=5, ln_stats_ld=B * N, ln_colsum=P, ln_eps=1e-5,
                 VT=P, vt_col0=2 * C_, vt_tokens=N, vt_bs=C_ * N, vt_rs=N), False


def _vt_batch(B, N, C_):
    """The unfolded V^T projection: per sample wv [C, C] x x[b] [N, C] -> vt[b] [C, N] (a strided batch of B)."""
    d = _gemm(C_, N, C_, bias=None, ldc=N, strideW=N * C_, strideC=C_ * N, batch=B)
    return d, False


def _conv(B, H, W, C1, C2, Cout):
    lib, ops = _ops()
    return lib.Conv3x3Desc(P, P, P, P, P, None, None, B, H, W, C1, C2, Cout, 1, 1, 0, 0, 0, P, ops.SPLITK_WS_BYTES, -1, 64)


def _mx8(B, N, C_, D):
    """The LayerNorm-folded q | k | V^T projection with the MX-fp8 copy-out (C and VT are not written: null)."""
    lib, _ = _ops()
    d = _gemm(B * N, 3 * C_, C_, C=None, bias=None, ldc=0, alpha_cols=C_, ln_stats=P, ln_parts=1, ln_stats_ld=B * N, ln_colsum=P, ln_eps=1e-5,
              vt_col0=2 * C_, vt_tokens=N, workspace=None, workspace_bytes=0)
    mx = lib.Mx8OutDesc()
    mx.nranges, mx.channel_rows = 3, 0
    for i, (lay, c0) in enumerate(((TOKENS, 0), (TOKENS, C_), (VT, 2 * C_))):
        mx.r[i] = lib.Mx8OutRange(P, P, lay, c0, 1.0, B, C_ // D, N, D)
    return d, mx


GEMMS = {"proj_in": _proj_in, "to_out": _to_out, "geglu": _geglu, "qkv": _qkv}


def _expect(kind, big, key, mx=None):
    """What the pinned launch must take: the plan of the scaled problem with the scaled shape key's tuned tile."""
    _, ops = _ops()
    big.tile_cfg = ops._TUNED.get(key, -1)
    if mx is not None:
        big.tile_cfg = ops._mx8_tile(big, mx, big.tile_cfg)
    pl = ops._plan(kind, big, mx)
    return pl[0] | (max(1, pl[1]) << 8)


def _pinned_tile(kind, d, stats=False, mx=None):
    _, ops = _ops()
    misses = len(ops._PIN_MISSES)
    with ops.pinned_batch_scale(2):
        got = ops._tile(kind, d, ops._key(kind, d, stats), mx, stats)
    assert len(ops._PIN_MISSES) == misses
    return got


@pytest.mark.parametrize("name", sorted(GEMMS))
@pytest.mark.parametrize("B,N,C_", [(4, 4096, 320), (4, 1024, 640), (2, 256, 1280), (1, 64, 1280)])
def test_pinned_gemm_is_the_plan_at_twice_the_batch(name, B, N, C_):
    _, ops = _ops()
    d, stats = GEMMS[name](B, N, C_)
    big, _ = GEMMS[name](2 * B, N, C_)
    assert _pinned_tile("gemm", d, stats) == _expect("gemm", big, ops._key("gemm", big, stats))


@pytest.mark.parametrize("B,N,C_", [(4, 4096, 320), (1, 1024, 640), (2, 256, 1280)])
def test_pinned_strided_batch_scales_the_batch(B, N, C_):
    _, ops = _ops()
    d, _ = _vt_batch(B, N, C_)
    big, _ = _vt_batch(2 * B, N, C_)
    key = ops._key("batch", big)
    assert key == f"g:{C_}:{N}:{C_}:{2 * B}"
    assert _pinned_tile("batch", d) == _expect("batch", big, key)


@pytest.mark.parametrize("B,H,C1,C2,Cout", [(4, 8, 1280, 1280, 1280), (4, 32, 640, 320, 320), (1, 64, 320, 320, 320), (2, 16, 1280, 640, 640)])
def test_pinned_concat_conv_scales_b(B, H, C1, C2, Cout):
    _, ops = _ops()
    d, big = _conv(B, H, H, C1, C2, Cout), _conv(2 * B, H, H, C1, C2, Cout)
    assert _pinned_tile("conv", d) == _expect("conv", big, ops._key("conv", big))


@pytest.mark.parametrize("B,N,C_,D", [(4, 4096, 320, 40), (4, 1024, 640, 80), (2, 256, 1280, 160), (4, 64, 1280, 160)])
def test_pinned_mx8_copy_out_scales_m_and_every_range(B, N, C_, D):
    _, ops = _ops()
    d, mx = _mx8(B, N, C_, D)
    big, bmx = _mx8(2 * B, N, C_, D)
    got = _pinned_tile("mx8", d, mx=mx)
    assert got == _expect("mx8", big, ops._key("mx8", big), bmx)
    d.tile_cfg = got
    plan = ops._plan("mx8", d, mx)
    d.tile_cfg = got & 255                           # the bare tile index (no split-K field) plans the same launch
    assert ops._plan("mx8", d, mx) == plan and plan[1] == 1


def test_fp8_operands_are_not_pinned():
    lib, ops = _ops()
    d = lib.GemmDesc(P, None, P, P, None, None, None, 4096, 640, 320, 320, 320, 0, 320, 640, 0, 0, 0, 0, 0, 0, 0, 1, 1.0, 0, 0, None, 0, -1,
                     P, P, 0, 0, 1)
    key = ops._key("gemm", d)
    assert key == "g8:4096:640:320:1"
    n = len(ops._PIN_CACHE)
    with ops.pinned_batch_scale(2):
        assert ops._tile("gemm", d, key) == ops._TUNED.get(key, -1)
    assert len(ops._PIN_CACHE) == n


@pytest.mark.parametrize("field,value", [("rowvec", P), ("act", 1), ("row_stats_out", P), ("C", P + 8), ("ldc", 648)])
def test_pin_cache_separates_planner_inputs(field, value):
    """Two launches with one shape key that differ in one input of the plan never share a cached decision."""
    _, ops = _ops()
    a = _gemm(4096, 640, 320, group_rows=4096)
    b = _gemm(4096, 640, 320, group_rows=4096, **{field: value})
    key = ops._key("gemm", a)
    assert ops._key("gemm", b) == key and ops._desc_key(a) != ops._desc_key(b)
    ops._PIN_CACHE.clear()
    with ops.pinned_batch_scale(2):
        ops._tile("gemm", a, key)
        ops._tile("gemm", b, key)
        ops._tile("gemm", _gemm(4096, 640, 320, group_rows=4096), key)            # the same inputs as `a`: its entry
    assert len(ops._PIN_CACHE) == 2


def test_desc_key_reduces_pointers():
    """Only null / non-null and the address mod 16 of a pointer reach the key."""
    _, ops = _ops()
    assert ops._desc_key(_gemm(4096, 640, 320)) == ops._desc_key(_gemm(4096, 640, 320, A=P + 4096, W=P + 32, C=P + 48))
    assert ops._desc_key(_gemm(4096, 640, 320)) != ops._desc_key(_gemm(4096, 640, 320, A=P + 4))
    assert ops._desc_key(_gemm(4096, 640, 320)) != ops._desc_key(_gemm(4096, 640, 320, resid=P))
    d, mx = _mx8(4, 1024, 640, 80)
    m2 = type(mx).from_buffer_copy(mx)
    m2.r[2].data = P + 64
    assert ops._desc_key(mx) == ops._desc_key(m2)
    m2.r[2].B = 8
    assert ops._desc_key(mx) != ops._desc_key(m2)


def test_plan_matches_the_entry_points():
    lib, ops = _ops()
    h = lib.load()
    d = _gemm(4096, 640, 320)
    out, need = (C.c_int32 * 6)(), C.c_size_t()
    assert h.pbe_gemm_plan(C.byref(d), out, C.byref(need)) == 0 and ops._plan("gemm", d) == list(out)
    cd = _conv(4, 32, 32, 640, 320, 320)
    assert h.pbe_conv3x3_plan(C.byref(cd), out, C.byref(need)) == 0 and ops._plan("conv", cd) == list(out)
    d, mx = _mx8(4, 1024, 640, 80)
    assert h.pbe_gemm_mx8out_plan(C.byref(d), C.byref(mx), out) == 0 and ops._plan("mx8", d, mx) == list(out)
    d.tile_cfg = 3 | (1 << 8)                                                           # 128 columns split a d = 80 block: refused
    with pytest.raises(lib.PbeError, match="splits an MX block"):
        ops._plan("mx8", d, mx)
    assert ops._mx8_tile(d, mx, 3) == -1
