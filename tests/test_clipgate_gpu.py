"""The exemplar-conditioning chain on the device against tests/clipref.py: every case of clipref.CASES through the product entry, the output
through clipref.verdict (limits from the fp32 emulation in two summation orders, never from a kernel's output), and the launches the
stage must make asserted from recorders around ops.layernorm / gemm / attention / clip_patchify / bcast_row.

Product entries: _EncoderLayer.run(x, B, N, vt) with vt zeroed as pooled makes it; _VisionTransformer.pooled - and, for the residual
stream after each layer (every token, which the pooled output cannot see), the layers driven one at a time by the statements of pooled,
whose last step must reproduce pooled bit for bit; Transformer.run + ops.layernorm as FrozenCLIPImageEmbedder.forward runs them; the
embedder's forward followed by HipLinear.  Parameters come from load_state_dict of the case's dict.

The printed lines (pytest -s) are the GPU half of the DESIGN.md section; PBE_CLIPGATE_REPORT=<file> appends them there.
"""
import os

import pytest
import torch

import clipref as R

pytestmark = pytest.mark.gpu

IDS = [c["id"] for c in R.CASES]
CONTROL_CASE = "layer-256h4-N65-unit"


def report(line):
    print(line)
    path = os.environ.get("PBE_CLIPGATE_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


class _Recorded:
    """Recorders around the five ops the chain launches through; the originals are back on exit."""
    NAMES = ("layernorm", "gemm", "attention", "clip_patchify", "bcast_row")

    def __enter__(self):
        from pbe_amd import ops
        self.ops, self.saved, self.calls = ops, {n: getattr(ops, n) for n in self.NAMES}, []

        def wrap(name, fn):
            def rec(*a, **kw):
                call = dict(op=name)
                if name == "gemm":
                    out = kw.get("out")
                    call.update(batched=a[0].dim() == 3, a_stride0=a[0].dim() == 3 and a[0].stride(0) == 0, rows=a[0].shape[-2],
                                bias=len(a) > 2 and a[2] is not None, bias_per_row=bool(kw.get("bias_per_row")), resid=kw.get("resid") is not None,
                                resid_2d=kw.get("resid") is not None and kw["resid"].dim() == 2, act=kw.get("act", 0),
                                out_strided=out is not None and not out.is_contiguous())
                elif name == "attention":
                    call.update(B=a[3], H=a[4], Nq=a[5], Nk=a[6], D=a[7], scale=a[8], q_strides=kw["q_strides"], k_strides=kw["k_strides"],
                                vt_strides=kw["vt_strides"], shared=a[0].data_ptr() + 2 * a[4] * a[7] == a[1].data_ptr())
                elif name == "layernorm":
                    call.update(rows=a[0].reshape(-1, a[0].shape[-1]).shape[0], eps=a[3] if len(a) > 3 else kw.get("eps", 1e-5),
                                strided=not a[0].is_contiguous())
                self.calls.append(call)
                return fn(*a, **kw)
            return rec
        for n, fn in self.saved.items():
            setattr(ops, n, wrap(n, fn))
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(self.ops, n, fn)

    def of(self, name):
        return [c for c in self.calls if c["op"] == name]


def _clip_config(c):
    return dict(hidden_size=c["hidden"], intermediate_size=c["mlp"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                image_size=c["image"] or 14, patch_size=c["patch"], layer_norm_eps=R.EPS)


def _load(m, sd, prefix="", allow_missing=()):
    res = m.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=False)
    assert not res.unexpected_keys and sorted(res.missing_keys) == sorted(allow_missing), res
    return m


def _module(c, sd, dev):
    """The product module(s) of a case with the case's parameters, on the device."""
    from ldm.models.diffusion.ddpm import HipLinear
    from ldm.modules.encoders import modules as enc
    from ldm.modules.encoders.xf import LayerNorm, Transformer
    kind = c["kind"]
    if kind == "layer":
        return _load(enc._EncoderLayer(_clip_config(c)), sd).to(dev)
    if kind == "tower":
        return _load(enc._VisionTransformer(_clip_config(c)), sd, allow_missing=["embeddings.position_ids"]).to(dev)
    if kind == "mapper":
        return (_load(Transformer(1, c["hidden"], c["layers"], 1), sd, "mapper.").to(dev), _load(LayerNorm(c["hidden"]), sd, "final_ln.").to(dev))
    emb = enc.FrozenCLIPImageEmbedder(clip_config=_clip_config(c), mapper_layers=c["layers"])
    _load(emb, sd, "cond_stage_model.", allow_missing=["transformer.vision_model.embeddings.position_ids"])
    return emb.to(dev), _load(HipLinear(c["hidden"], R.PROJ), sd, "proj_out.").to(dev)


def _tower_by_layer(vm, pixels):
    """The statements of _VisionTransformer.pooled with the residual stream kept after each layer -> (streams, pooled)."""
    from pbe_amd import ops
    p, cfg = vm.pk(), vm.cfg
    Bn = pixels.shape[0]
    d, P, eps = cfg["hidden_size"], cfg["patch_size"], cfg["layer_norm_eps"]
    G = cfg["image_size"] // P
    N = G * G + 1
    patches = ops.clip_patchify(pixels, P, p.kp)
    tokens = torch.empty((Bn, N, d), dtype=torch.float16, device=pixels.device)
    ops.gemm(patches.view(Bn, G * G, p.kp), p.wpatch.unsqueeze(0), resid=p.pos[1:], out=tokens[:, 1:, :])
    ops.bcast_row(p.cls, p.pos[0], tokens, Bn, N * d)
    x = ops.layernorm(tokens.view(Bn * N, d), p.gpre, p.bpre, eps)
    vt = torch.zeros((Bn, d, (N + 7) // 8 * 8), dtype=torch.float16, device=pixels.device)
    streams = []
    for layer in vm.encoder.layers:
        x = layer.run(x, Bn, N, vt)
        streams.append(x.clone())
    return streams, ops.layernorm(x.view(Bn, N, d)[:, 0, :], p.gpost, p.bpost, eps)


def _run(c, m, inp, dev):
    """The stage on the device -> ({output name: tensor on the device}, the recorder of the product entry's own launches)."""
    from pbe_amd import ops
    kind, outs = c["kind"], {}
    if kind == "layer":
        vt = torch.zeros((c["B"], c["hidden"], (c["N"] + 7) // 8 * 8), dtype=torch.float16, device=dev)
        with _Recorded() as rec:
            outs["out"] = m.run(inp["x"].to(dev), c["B"], c["N"], vt)
    elif kind == "tower":
        px = inp["pixels"].to(dev)
        with _Recorded() as rec:
            outs["out"] = m.pooled(px)
        streams, pooled = _tower_by_layer(m, px)
        assert torch.equal(pooled, outs["out"]), "the layers driven one at a time do not reproduce pooled()"
        outs.update({f"stream{i}": s for i, s in enumerate(streams)})
    elif kind == "mapper":
        tr, ln = m
        with _Recorded() as rec:
            z = tr.run(inp["z"].to(dev))
            outs["out"] = ops.layernorm(z, ln.weight.float(), ln.bias.float(), ln.eps)
    else:
        emb, lin = m
        px = inp["pixels"].to(dev)
        with _Recorded() as rec:
            outs["out"] = lin(emb(px))
        outs["pooled"] = emb.transformer(pixel_values=px).pooler_output
    return outs, rec


def _check_layer_launches(c, ln, gemm, att, Bn):
    """2 layernorm, 5 gemm, 1 attention of one encoder layer."""
    from pbe_amd import ops
    d, N, H = c["hidden"], c["N"], c["heads"]
    assert len(ln) == 2 and len(gemm) == 5 and len(att) == 1, (ln, gemm, att)
    assert all(g["rows"] == Bn * N and not g["batched"] for i, g in enumerate(gemm) if i != 1)
    vt = gemm[1]                                                       # V^T: the expanded weight, bias per row, written into vt[:, :, :N]
    assert vt["a_stride0"] and vt["bias_per_row"] and vt["batched"] and vt["rows"] == d and vt["out_strided"] == (N % 8 != 0)
    assert [g["a_stride0"] or g["bias_per_row"] for g in gemm] == [False, True, False, False, False]
    assert [g["resid"] for g in gemm] == [False, False, True, False, True]
    assert [g["act"] for g in gemm] == [0, 0, 0, ops.ACT_QUICK_GELU, 0] and all(g["bias"] for g in gemm)
    a = att[0]
    assert (a["B"], a["H"], a["Nq"], a["Nk"], a["D"]) == (Bn, H, N, N, d // H) and a["scale"] == (d // H) ** -0.5
    assert a["shared"] and a["q_strides"] == a["k_strides"] == (N * 2 * d, 2 * d)                         # q and k out of one [B*N, 2d] tensor
    assert a["vt_strides"] == (d * ((N + 7) // 8 * 8), (N + 7) // 8 * 8)
    assert all(x["eps"] == R.EPS and x["rows"] == Bn * N for x in ln)


def _check_mapper_launches(c, ln, gemm, Bn):
    """2 layernorm and 4 gemm per block, then final_ln."""
    from pbe_amd import ops
    L = c["layers"]
    assert len(ln) == 2 * L + 1 and len(gemm) == 4 * L, (ln, gemm)
    assert all(g["rows"] == Bn and not g["batched"] and g["bias"] for g in gemm) and all(x["rows"] == Bn and x["eps"] == R.EPS for x in ln)
    assert [g["resid"] for g in gemm] == [False, True, False, True] * L and [g["act"] for g in gemm] == [0, 0, ops.ACT_GELU, 0] * L


def _check_launches(c, rec):
    kind, Bn, L = c["kind"], c["B"], c["layers"]
    ln, gemm, att, pat, bc = (rec.of(n) for n in _Recorded.NAMES)
    if kind == "layer":
        assert not pat and not bc
        return _check_layer_launches(c, ln, gemm, att, Bn)
    if kind == "mapper":
        assert not att and not pat and not bc
        return _check_mapper_launches(c, ln, gemm, Bn)
    nt_ln, nt_gemm = 2 + 2 * L, 1 + 5 * L                              # the tower's share
    assert len(pat) == 1 and len(bc) == 1 and len(att) == L
    pg = gemm[0]                                                       # the patch GEMM: batched, pos[1:] shared over the batch, out = tokens[:, 1:, :]
    assert pg["batched"] and pg["resid"] and pg["resid_2d"] and pg["out_strided"] and not pg["bias"] and pg["rows"] == c["N"] - 1 and not pg["a_stride0"]
    assert ln[0]["rows"] == Bn * c["N"] and ln[nt_ln - 1]["rows"] == Bn and ln[nt_ln - 1]["strided"]                   # pre_layrnorm; post_layernorm of the CLS rows
    for i in range(L):
        _check_layer_launches(c, ln[1 + 2 * i:3 + 2 * i], gemm[1 + 5 * i:6 + 5 * i], att[i:i + 1], Bn)
    if kind == "tower":
        assert len(ln) == nt_ln and len(gemm) == nt_gemm
        return
    _check_mapper_launches(c, ln[nt_ln:], gemm[nt_gemm:-1], Bn)
    proj = gemm[-1]
    assert len(gemm) == nt_gemm + 4 * L + 1 and proj["rows"] == Bn and proj["bias"] and not proj["resid"] and proj["act"] == 0


_RESULTS = {}


def _case_result(dev, cid):
    """{output name: tensor on the CPU} of a case, run once; the launches are checked on the way."""
    if cid not in _RESULTS:
        r = R.refs(cid)
        with torch.no_grad():
            outs, rec = _run(r.c, _module(r.c, r.sd, dev), r.inp, dev)
        torch.cuda.synchronize()
        _check_launches(r.c, rec)
        _RESULTS[cid] = {k: v.cpu() for k, v in outs.items()}
    return _RESULTS[cid]


def _judge(cid, outs, what=""):
    r = R.refs(cid)
    assert set(outs) == set(r.names()), (cid, sorted(outs))
    ok = True
    for n in r.names():
        assert tuple(outs[n].shape) == tuple(r.ref64()[n].shape) and outs[n].dtype == torch.float16, (cid, n, tuple(outs[n].shape))
        o, text = r.verdict_of(n, outs[n])
        report(f"clipgate gpu  {cid + what:36s} {n:8s}: {text}")
        ok = ok and o
    return ok


@pytest.mark.parametrize("cid", IDS)
def test_case_against_ref64(dev, cid):
    assert _judge(cid, _case_result(dev, cid)), cid


def test_forward_of_several_exemplars_is_the_flattened_batch_and_repeats(dev):
    """forward(image [B, K, 3, S, S]) equals forward of the flattened [B * K, 3, S, S] batch bit for bit, and a second call on the same
    module (cached pack, fresh scratch) equals the first."""
    r = R.refs("cond-256h4-img56x2to96-unit")
    emb, lin = _module(r.c, r.sd, dev)
    px = r.inp["pixels"].to(dev)
    with torch.no_grad():
        flat = emb(px)
        again = emb(px)
        five = emb(px.reshape(1, 3, *px.shape[1:]))
        col = emb(px.reshape(3, 1, *px.shape[1:]))
        c1, c2 = lin(flat), lin(again)
    assert tuple(flat.shape) == (3, 1, 256) and tuple(five.shape) == (1, 3, 256) and tuple(col.shape) == (3, 1, 256)
    assert torch.equal(flat, again) and torch.equal(c1, c2)
    assert torch.equal(five.reshape(3, 256), flat.reshape(3, 256)) and torch.equal(col, flat)
    assert torch.equal(c1.cpu(), _case_result(dev, r.c["id"])["out"])


def test_positive_control_wrong_head_count_on_the_product_layer(dev):
    """The product layer told to split 8 heads instead of 4: the verdict rejects the run, and accepts it again once the module is
    restored."""
    r = R.refs(CONTROL_CASE)
    m = _module(r.c, r.sd, dev)
    keep = m.heads
    try:
        m.heads = 2 * keep
        with torch.no_grad():
            bad = {k: v.cpu() for k, v in _run(r.c, m, r.inp, dev)[0].items()}
    finally:
        m.heads = keep
    assert not _judge(CONTROL_CASE, bad, " [8 heads]")
    with torch.no_grad():
        good = {k: v.cpu() for k, v in _run(r.c, m, r.inp, dev)[0].items()}
    assert _judge(CONTROL_CASE, good, " [restored]")
