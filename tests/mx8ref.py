"""Host reference of the MX-fp8 operands (include/pbe_hip.h, pbe_quant_mx8_f16): OCP e4m3 bytes with one E8M0 scale per 32 contraction
elements, in the layouts the attention kernel streams.  numpy only, so the CPU tests can check it against hand-computed values."""
import numpy as np

E4M3_MAX = 448.0


def e4m3_values() -> np.ndarray:
    """float64 value of every e4m3 code (0x7f / 0xff, the NaNs, as nan)."""
    v = np.empty(256)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        mag = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        v[c] = -mag if s else mag
    v[0x7F] = v[0xFF] = np.nan
    return v


_VALUES = e4m3_values()


def e4m3_encode(y) -> np.ndarray:
    """Codes of float32 y: round to nearest even, saturating at +-448, subnormals kept (quantum 2^-9), never NaN."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    a = np.minimum(np.abs(y), E4M3_MAX)
    e = np.where(a >= 2.0 ** -6, np.frexp(np.maximum(a, 2.0 ** -6))[1] - 1.0, -6.0)
    q = 2.0 ** (e - 3)
    r = np.minimum(np.rint(a / q) * q, E4M3_MAX)                     # np.rint: ties to even
    sub = r < 2.0 ** -6
    er = np.frexp(np.maximum(r, 2.0 ** -6))[1] - 1.0
    mant = np.rint((r / 2.0 ** er - 1) * 8)
    code = np.where(sub, np.rint(r * 512), (er + 7) * 8 + mant).astype(np.int64)
    return (code | np.where(y < 0, 0x80, 0)).astype(np.uint8)


def e4m3_decode(codes) -> np.ndarray:
    return _VALUES[np.asarray(codes, dtype=np.uint8)]


def scale_exp(amax) -> np.ndarray:
    """E8M0 code (biased exponent) of the smallest power of two s with amax / s <= 448; amax == 0 -> 127 (1.0)."""
    amax = np.asarray(amax, dtype=np.float32)
    m, E = np.frexp(amax.astype(np.float64))                         # amax = m 2^E, m in [0.5, 1)
    m, E = m * 2, E - 1                                               # m in [1, 2)
    e = np.where(m <= 1.75, E - 8, E - 7)
    return np.where(amax > 0, np.clip(e + 127, 1, 254), 127).astype(np.uint8)


def _blocks(v: np.ndarray):
    """v [..., 32] float32 -> (codes [..., 32] uint8, scale codes [...] uint8)"""
    se = scale_exp(np.abs(v).max(-1))
    inv = (2.0 ** (127.0 - se.astype(np.float64))).astype(np.float32)
    return e4m3_encode(v * inv[..., None]), se


def quant_tokens(x, B, H, N, D, alpha=1.0):
    """x: float16 [B*N, >= H*D] (row stride = its 2nd dim) -> (bytes [B*N, H*DP], scales [B, H, DP/32, NP])."""
    DP, NP = (D + 63) // 64 * 64, (N + 63) // 64 * 64
    v = np.zeros((B * N, H, DP), dtype=np.float32)
    v[:, :, :D] = np.asarray(x, dtype=np.float16)[:, :H * D].astype(np.float32).reshape(B * N, H, D) * np.float32(alpha)
    codes, se = _blocks(v.reshape(B * N, H, DP // 32, 32))
    scales = np.full((B, H, DP // 32, NP), 127, dtype=np.uint8)
    scales[:, :, :, :N] = se.reshape(B, N, H, DP // 32).transpose(0, 2, 3, 1)
    return codes.reshape(B * N, H * DP), scales


def quant_vt(x, B, H, N, D, alpha=1.0):
    """x: float16 [B*H*D, >= N] (V^T rows) -> (bytes [B*H*D, NP], scales [B, H, NP/32, DV])."""
    NP, DV = (N + 63) // 64 * 64, (D // 32 + 1) * 32
    v = np.zeros((B * H * D, NP), dtype=np.float32)
    v[:, :N] = np.asarray(x, dtype=np.float16)[:, :N].astype(np.float32) * np.float32(alpha)
    codes, se = _blocks(v.reshape(B * H * D, NP // 32, 32))
    scales = np.full((B, H, NP // 32, DV), 127, dtype=np.uint8)
    scales[:, :, :, :D] = se.reshape(B, H, D, NP // 32).transpose(0, 1, 3, 2)
    return codes.reshape(B * H * D, NP), scales


def dequant_tokens(codes, scales, B, H, N, D) -> np.ndarray:
    """-> float64 [B, H, N, D]"""
    DP = (D + 63) // 64 * 64
    v = e4m3_decode(codes).reshape(B, N, H, DP // 32, 32)
    s = 2.0 ** (scales[:, :, :, :N].astype(np.float64) - 127)       # [B, H, DP/32, N]
    v = v * s.transpose(0, 3, 1, 2)[..., None]
    return v.reshape(B, N, H, DP)[..., :D].transpose(0, 2, 1, 3)


def dequant_vt(codes, scales, B, H, N, D) -> np.ndarray:
    """-> float64 [B, H, N, D] (V, untransposed)"""
    NP = (N + 63) // 64 * 64
    v = e4m3_decode(codes).reshape(B, H, D, NP // 32, 32)
    s = 2.0 ** (scales[:, :, :, :D].astype(np.float64) - 127)       # [B, H, NP/32, D]
    v = v * s.transpose(0, 1, 3, 2)[..., None]
    return v.reshape(B, H, D, NP)[..., :N].transpose(0, 1, 3, 2)
