"""References for the two SpatialTransformer folds (ldm/modules/attention.py: the GroupNorm on proj_in's A operand, proj_out composed into
ff-out).  Helpers imported by test_stfold_cpu.py and test_stfold_gpu.py.  Not a conftest: plain functions only."""
import torch


def gn_table_ref(partials, gamma, beta, hw, eps):
    """pbe_groupnorm_table_f32 restated in fp64: partials [B, blocks, G, 2] (sum, sumsq) -> (sc, sh) [B, C] with sc = rstd gamma,
    sh = beta - mean sc; mean and var = E[x^2] - mean^2 (clamped at 0) over the hw * C / G elements of a group."""
    p = partials.double().sum(1)                                   # [B, G, 2]
    B, G = p.shape[:2]
    C = gamma.numel()
    n = float(hw * (C // G))
    mean = p[..., 0] / n
    var = (p[..., 1] / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    sc = rstd.repeat_interleave(C // G, 1) * gamma.double()[None, :]
    sh = beta.double()[None, :] - mean.repeat_interleave(C // G, 1) * sc
    return sc, sh


def table_layout(sc, sh):
    """(sc, sh) [B, C] -> the kernel's table [B, C / 8, 16]: sc | sh of 8 consecutive channels."""
    B, C = sc.shape
    return torch.cat([sc.view(B, C // 8, 8), sh.view(B, C // 8, 8)], 2)


def partials_of(x, groups, blocks):
    """Partial (sum, sumsq) [B, blocks, G, 2] fp32 of x [B, HW, C] over `blocks` equal row blocks, as a producing conv leaves them."""
    B, HW, C = x.shape
    v = x.float().view(B, blocks, HW // blocks, groups, C // groups)
    return torch.stack([v.sum((2, 4)), (v * v).sum((2, 4))], -1).contiguous()


def h16(t):
    """Round to fp16 (nearest even), carried in fp64."""
    return t.to(torch.float16).double()


def tail_problem(M, C, seed, device="cpu"):
    """Random operands of the transformer's tail at width C (ff inner 4 C): fp16 h [M, 4C], x2, x_in [M, C]; fp32 master weights."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    h = (r(M, 4 * C) * 0.5).half()
    x2, xin = r(M, C).half(), r(M, C).half()
    wff, bff = r(C, 4 * C) / (4 * C) ** 0.5, r(C) * 0.1
    wpo, bpo = r(C, C) / C ** 0.5, r(C) * 0.1
    return tuple(t.to(device) for t in (h, x2, xin, wff, bff, wpo, bpo))


def tail_fp64(h, x2, xin, wff, bff, wpo, bpo):
    """x_in + proj_out(x2 + ff_out(h)) in fp64 from the master weights."""
    x3 = x2.double() + h.double() @ wff.double().T + bff.double()
    return xin.double() + x3 @ wpo.double().T + bpo.double()


def tail_chain_emulated(h, x2, xin, wff, bff, wpo, bpo):
    """The two launches with every rounding of the GEMM epilogue (fp16 weights; fp16(acc + bias), then fp16(that + residual)); the
    accumulation itself in fp64 (its fp32 error is common to both forms)."""
    x3 = h16(h16(h.double() @ h16(wff).T + bff.float().double()) + x2.double())
    return h16(h16(x3 @ h16(wpo).T + bpo.float().double()) + xin.double())


def tail_composed_emulated(h, x2, xin, wt, bt):
    """The composed launch with its roundings: wt / bt from compose_tail (fp16 / fp32)."""
    a = torch.cat([h, x2], 1).double()
    return h16(h16(a @ wt.double().T + bt.double()) + xin.double())


def err(y, ref):
    d = (y.double() - ref).abs()
    return d.max().item(), (d * d).mean().sqrt().item()
