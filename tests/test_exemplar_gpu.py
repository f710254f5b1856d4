"""The exemplar cut on the device: the kernels of pbe_amd/csrc/exemplar.hip through ops.resample_u8 / ops.mask_box against tests/pilref.py
and against Pillow, by equality (pictures and masks between poison bytes, outputs in sentinel arenas: tests/guard.py), the public
surface (pbe_amd.exemplar, preprocess.load_reference_device) against the host path it replaces, pipeline.inpaint on the narrow model, and
the --reference_* flags of scripts/inference.py.  No tolerance anywhere, and no test here judges picture quality."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import cases
import guard
import modelbuild as build
import pilref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
PIC_POISON, MASK_POISON, SECOND_FILL = 0xEE, 0xFF, 0x5A


def _where():
    import platform
    import PIL
    return f"Pillow {PIL.__version__} on {platform.machine()} / {platform.system()}"


def _embed_u8(a, dev, poison):
    view, arena = guard.embed(torch.from_numpy(np.array(a)).reshape(-1), device=dev, poison=poison)      # a copy: the sources are read-only
    return view.view(a.shape), arena


def _resample_guarded(ops, pv, out_hw, what, **kw):
    """ops.resample_u8 into sentinel arenas: (bytes, planes) on the host, nothing outside them touched, the planes fully written, and the
    bytes fully written too - an output byte may equal the sentinel 0xA5, so the call is made twice, over 0xA5 and over 0x5A, and the two
    results must agree."""
    oh, ow = out_hw
    flat, arena = guard.sentinel_out((oh * ow * 3,), dtype=torch.uint8, device=pv.device)
    pflat, parena = guard.sentinel_out((3 * oh * ow,), dtype=torch.float32, device=pv.device)
    y, planes = ops.resample_u8(pv, out_hw, mean=CLIP[0], std=CLIP[1], out=flat.view(oh, ow, 3), out_planes=pflat.view(3, oh, ow), **kw)
    assert y.data_ptr() == flat.data_ptr() and planes.data_ptr() == pflat.data_ptr()
    guard.assert_untouched(arena, flat, what)
    guard.assert_untouched(parena, pflat, what + " planes")
    guard.assert_fully_written(pflat, what + " planes")
    first = y.cpu().numpy()
    arena.fill_(SECOND_FILL)
    ops.resample_u8(pv, out_hw, out=flat.view(oh, ow, 3), **kw)
    guard.assert_untouched(arena, flat, what, pattern=SECOND_FILL)
    assert np.array_equal(first, y.cpu().numpy()), f"{what}: bytes of the output were not written"
    same = ops.u8_to_planes(torch.from_numpy(first).to(pv.device)[None], *CLIP)[0]
    assert torch.equal(planes, same), f"{what}: the planes are not u8_to_planes of the bytes"
    return first


def _check(got, a, out_hw, box, filt, what, mask=None, fill=None):
    ref = P.resize(a, out_hw, box, filt, mask=mask, fill=fill)
    assert got.shape == ref.shape and np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.size} bytes differ from the restatement"
    pil = P.pillow(P.compose(a, mask, fill), out_hw, box, filt)
    assert np.array_equal(got, pil), f"{what}: {int((got != pil).sum())} of {pil.size} bytes differ from {_where()}"


# ---- 1. ops.resample_u8 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.SOURCES)
def test_resample_equals_restatement_and_pillow(dev, name):
    from pbe_amd import ops
    a = P.source(name)
    pv, _ = _embed_u8(a, dev, PIC_POISON)
    for box, out_hw, filt in P.cases(name):
        what = f"resample_u8 {name} box {box} -> {out_hw} {filt}"
        _check(_resample_guarded(ops, pv, out_hw, what, box=box, filter=filt), a, out_hw, box, filt, what)


@pytest.mark.parametrize("hw", ((6, 16384), (16384, 3)), ids=("6x16384", "16384x3"))
def test_resample_longest_edges(dev, hw):
    """The largest edge the entry points take: 7283 bicubic taps through four staging rounds of the horizontal pass / 16384 rows, which
    Image.resize takes height first (pilref.tall_first)."""
    from pbe_amd import ops
    a = P.random_picture(hw, 77)
    pv, _ = _embed_u8(a, dev, PIC_POISON)
    H, W = hw
    for box, out_hw, filt in ((None, (17, 9), "bicubic"), (None, (17, 9), "lanczos"), ((0.5, 0.25, W - 0.5, H - 1), (224, 224), "bilinear"),
                              (None, (H, 9) if W > H else (9, W), "bicubic")):
        what = f"resample_u8 {hw} box {box} -> {out_hw} {filt}"
        _check(_resample_guarded(ops, pv, out_hw, what, box=box, filter=filt), a, out_hw, box, filt, what)
    if P.tall_first(H, W, 17):                                     # Image.resize's vertical-first rule, with the mask read by the vertical pass
        m = P.random_mask(hw, 3)
        mv, _ = _embed_u8(m, dev, MASK_POISON)
        what = f"resample_u8 {hw} masked -> (17, 9) bicubic"
        _check(_resample_guarded(ops, pv, (17, 9), what, mask=mv, fill=(9, 200, 77)), a, (17, 9), None, "bicubic", what, m, (9, 200, 77))


def test_resample_skip_paths_and_mask_fill(dev):
    """Pillow skips a pass whose axis keeps its size under a box that spans it: 224x224 whole (both: a copy), 300x224 whole (the vertical
    pass reads the picture), 225x1000 whole at its own height (the horizontal result is the output); each with and without mask + fill,
    which must equal Pillow on the composed picture; then mask + fill through both passes, boxes and every filter."""
    from pbe_amd import ops
    fill = (255, 0, 17)
    for name, out_hw in (("random_224x224", (224, 224)), ("random_300x224", (224, 224)), ("random_225x1000", (225, 224)), ("random_225x1000", (224, 224))):
        a = P.source(name)
        m = P.random_mask(a.shape[:2], 11)
        pv, _ = _embed_u8(a, dev, PIC_POISON)
        mv, _ = _embed_u8(m, dev, MASK_POISON)
        for filt in P.FILTERS:
            what = f"resample_u8 {name} whole -> {out_hw} {filt}"
            _check(_resample_guarded(ops, pv, out_hw, what, filter=filt), a, out_hw, None, filt, what)
            _check(_resample_guarded(ops, pv, out_hw, what + " masked", filter=filt, mask=mv, fill=fill), a, out_hw, None, filt, what + " masked", m, fill)
    got = ops.resample_u8(torch.from_numpy(np.array(P.source("random_224x224"))).to(dev), (224, 224))
    assert got[1] is None and np.array_equal(got[0].cpu().numpy(), P.source("random_224x224"))
    for name in ("random_37x53", "random_640x481", "random_8x1200"):
        a = P.source(name)
        m = P.random_mask(a.shape[:2], 13)
        pv, _ = _embed_u8(a, dev, PIC_POISON)
        mv, _ = _embed_u8(m, dev, MASK_POISON)
        for box, out_hw, filt in P.cases(name):
            what = f"resample_u8 {name} masked box {box} -> {out_hw} {filt}"
            _check(_resample_guarded(ops, pv, out_hw, what, box=box, filter=filt, mask=mv, fill=fill), a, out_hw, box, filt, what, m, fill)


def test_resample_refuses_bad_arguments(dev):
    from pbe_amd import lib, ops
    pic = torch.from_numpy(np.array(P.source("random_37x53"))).to(dev)
    mask = torch.zeros((37, 53), dtype=torch.uint8, device=dev)
    for kw in (dict(box=(-1, 0, 53, 37)), dict(box=(0, 0, 54, 37)), dict(box=(5, 0, 5, 37)), dict(filter="nearest"), dict(mask=mask), dict(fill=(1, 2, 3)),
               dict(mask=mask[:36], fill=(1, 2, 3)), dict(mask=mask, fill=(1, 2, 256)), dict(mean=CLIP[0])):
        with pytest.raises(lib.PbeError):
            ops.resample_u8(pic, (9, 9), **kw)
    for bad in ((0, 9), (9, 16385), (9.5, 9)):
        with pytest.raises(lib.PbeError):
            ops.resample_u8(pic, bad)
    with pytest.raises(lib.PbeError):
        ops.resample_u8(pic.cpu(), (9, 9))
    # the entry points themselves: null, misaligned and out-of-range arguments are error codes, and nothing is written
    from pbe_amd.exemplar import resample_tables
    h, s = lib.load(), torch.cuda.current_stream().cuda_stream
    b, k = (torch.from_numpy(t).to(dev) for t in resample_tables(53, 0, 53, 9, "bicubic"))
    bv, kv = (torch.from_numpy(t).to(dev) for t in resample_tables(37, 0, 37, 9, "bicubic"))
    ks, kvs = k.shape[1], kv.shape[1]
    out, arena = guard.sentinel_out((37 * 9 * 3,), dtype=torch.uint8, device=dev)
    fill = (lib.C.c_uint8 * 3)(1, 2, 3)
    p, o, m = pic.data_ptr(), out.data_ptr(), mask.data_ptr()
    def hargs(**kw):
        d = dict(pic=p, mask=None, fill=None, out=o, Hs=37, Ws=53, first=0, last=37, ow=9, b=b.data_ptr(), k=k.data_ptr(), ks=ks)
        assert set(kw) <= set(d)
        d.update(kw)
        return tuple(d.values())

    def vargs(**kw):
        d = dict(src=p, mask=None, fill=None, out=o, planes=None, rows=37, ow=9, oh=9, b=bv.data_ptr(), k=kv.data_ptr(), ks=kvs, mean=None, std=None)
        assert set(kw) <= set(d)
        d.update(kw)
        return tuple(d.values())
    for kw in (dict(pic=None), dict(out=None), dict(b=None), dict(k=None), dict(b=b.data_ptr() + 2), dict(k=k.data_ptr() + 1), dict(last=38), dict(first=5, last=5),
               dict(first=-1), dict(Hs=0), dict(Ws=16385), dict(ow=0), dict(ow=16385), dict(ks=0), dict(ks=98306), dict(mask=m)):
        assert h.pbe_resample_h_u8(*hargs(**kw), s) == -1, kw
    planes = torch.empty(3 * 9 * 9 + 1, dtype=torch.float32, device=dev)
    mean, std = (lib.C.c_float * 3)(*CLIP[0]), (lib.C.c_float * 3)(*CLIP[1])
    for kw in (dict(src=None), dict(out=None), dict(rows=0), dict(oh=16385), dict(ow=0), dict(b=None), dict(k=kv.data_ptr() + 2), dict(ks=0), dict(mask=m),
               dict(planes=planes.data_ptr(), std=std), dict(planes=planes.data_ptr(), mean=mean), dict(planes=planes.data_ptr() + 2, mean=mean, std=std)):
        assert h.pbe_resample_v_u8(*vargs(**kw), s) == -1, kw
    table = torch.empty((2, 4), dtype=torch.int32, device=dev)
    for args in ((None, table.data_ptr(), 37, 53, 2), (m, None, 37, 53, 2), (m, table.data_ptr() + 2, 37, 53, 2), (m, table.data_ptr(), 37, 53, 1),
                 (m, table.data_ptr(), 0, 53, 0), (m, table.data_ptr(), 37, 16385, 2)):
        assert h.pbe_mask_box_i32(*args, s) == -1, args
    assert h.pbe_mask_box_bands(0) == 0 and h.pbe_mask_box_bands(1) == 1 and h.pbe_mask_box_bands(33) == 2 and h.pbe_mask_box_bands(16384) == 512
    assert h.pbe_mask_box_bands(16385) == 0
    assert h.pbe_resample_workspace_bytes(0, 9) == 0 and h.pbe_resample_workspace_bytes(9, 16385) == 0
    assert h.pbe_resample_workspace_bytes(37, 9) >= 37 * 9 * 3 and h.pbe_resample_workspace_bytes(16384, 16384) >= 16384 * 16384 * 3
    assert b"pbe_mask_box_i32" in h.pbe_last_error()
    torch.cuda.synchronize()
    assert bool((guard.bits(arena) == guard.SENTINEL_BITS[torch.uint8]).all()), "a refused call wrote something"
    assert h.pbe_resample_h_u8(p, m, fill, o, 37, 53, 0, 37, 9, b.data_ptr(), k.data_ptr(), ks, s) == 0            # and the good call goes through
    torch.cuda.synchronize()
    guard.assert_untouched(arena, out, "pbe_resample_h_u8")
    assert bool((out.view(37, 9, 3) == torch.tensor([1, 2, 3], dtype=torch.uint8, device=dev)).all())         # an all-background mask: the fill everywhere


# ---- 2. ops.mask_box ---------------------------------------------------------------------------------------------------------------------
def test_mask_box(dev):
    from pbe_amd import ops
    from pbe_amd.window import hole_box
    band = ops.MASK_BOX_BAND
    shapes = ((1, 1), (17, 300), (band, 7), (band + 1, 257), (3 * band + 5, 600), (2 * band, 64))
    for Hs, Ws in shapes:
        masks = [("empty", np.full((Hs, Ws), 127, dtype=np.uint8))]
        for y, x in ((0, 0), (0, Ws - 1), (Hs - 1, 0), (Hs - 1, Ws - 1)):
            m = np.zeros((Hs, Ws), dtype=np.uint8)
            m[y, x] = 128
            m[Hs // 2, Ws // 2] = max(m[Hs // 2, Ws // 2], 127)                       # one below the threshold: not the object
            masks.append((f"corner ({y}, {x})", m))
        if Hs > band:                                                                  # a hole crossing the band borders, and two in different bands
            m = np.zeros((Hs, Ws), dtype=np.uint8)
            m[band - 3:min(2 * band + 2, Hs), 2:Ws - 1] = 200
            masks.append(("across bands", m))
            m = np.zeros((Hs, Ws), dtype=np.uint8)
            m[band - 1, Ws - 2], m[band, 1] = 255, 255
            masks.append(("either side of a border", m))
        full = np.full((Hs, Ws), 255, dtype=np.uint8)
        masks.append(("full", full))
        for tag, m in masks:
            mv, _ = _embed_u8(m, dev, MASK_POISON)
            got = ops.mask_box(mv)
            assert got == P.mask_box(m), f"mask_box {Hs} x {Ws} {tag}: {got} != {P.mask_box(m)}"
            if got is not None:
                assert got == hole_box(m)
    rng = np.random.default_rng(5)
    m = rng.integers(0, 129, size=(101, 333), dtype=np.uint8)
    m[:7], m[:, :5], m[90:], m[:, 300:] = 0, 0, 127, 1
    mv, _ = _embed_u8(m, dev, MASK_POISON)
    assert ops.mask_box(mv) == P.mask_box(m) == hole_box(m)


# ---- 3. the public surface -------------------------------------------------------------------------------------------------------------
def test_load_reference_device_equals_the_host_path(dev, golden_dir):
    from pbe_amd import preprocess
    d = os.path.join(golden_dir, "examples")
    for i in (1, 2, 3):
        paths = [os.path.join(d, n) for n in (f"image_example_{i}.png", f"mask_example_{i}.png", f"reference_example_{i}.jpg")]
        trip = preprocess.load_triple_device(*paths, dev)
        e = preprocess.load_reference_device(paths[2], dev)
        assert e["ref"].shape == (1, 3, 224, 224) and e["ref"].dtype == torch.float32 and torch.equal(e["ref"], trip["ref"]), f"example {i}"
        assert np.array_equal(e["u8"].cpu().numpy(), preprocess.load_triple_u8(*paths)["ref"]), f"example {i}"
        assert torch.equal(e["ref"].cpu(), preprocess.load_triple(*paths)["ref"]), f"example {i}: not the host path's exemplar"
        w, h = P.source(f"reference_example_{i}.jpg").shape[1::-1]
        assert e["box"] == (0, 0, w, h)


def test_exemplar_from_picture_boxes_masks_and_lists(dev, tmp_path):
    from PIL import Image
    from pbe_amd import exemplar, lib, ops, preprocess
    a = P.source("reference_example_3.jpg")
    H, W = a.shape[:2]
    pic = torch.from_numpy(np.array(a)).to(dev)
    m = np.zeros((H, W), dtype=np.uint8)
    m[400:901, 100:351] = 255
    m[10, 10] = 127
    mask = torch.from_numpy(m).to(dev)

    def pil(box, src=a):
        return np.array(Image.fromarray(src).resize((224, 224), box=box), dtype=np.uint8)
    e = exemplar.exemplar_from_picture(pic, box=(100.5, 400, 351, 901.25))
    assert e["box"] == (100.5, 400.0, 351.0, 901.25) and np.array_equal(e["u8"].cpu().numpy(), pil((100.5, 400, 351, 901.25)))
    assert torch.equal(e["ref"][0], ops.u8_to_planes(e["u8"][None], *CLIP)[0])
    e = exemplar.exemplar_from_picture(pic, mask=mask)
    assert e["box"] == (100, 400, 351, 901) and np.array_equal(e["u8"].cpu().numpy(), pil((100, 400, 351, 901)))
    e = exemplar.exemplar_from_picture(pic, mask=mask, pad=0.1, square=True, fill=(0, 128, 255))
    box = exemplar.plan_crop((400, 900, 100, 350), (H, W), 0.1, True)
    assert e["box"] == box and box[2] - box[0] == box[3] - box[1] == 603
    assert np.array_equal(e["u8"].cpu().numpy(), pil(box, P.compose(a, m, (0, 128, 255))))
    e = exemplar.exemplar_from_picture(pic, box=(100, 400, 351, 901), square=True)
    assert e["box"] == exemplar.plan_crop((400, 900, 100, 350), (H, W), 0.0, True)
    small = exemplar.exemplar_from_picture(pic, box=(0, 0, 100, 50), size=64, filter="lanczos")
    assert np.array_equal(small["u8"].cpu().numpy(), P.pillow(a, (64, 64), (0, 0, 100, 50), "lanczos")) and small["ref"].shape == (1, 3, 64, 64)
    for kw in (dict(mask=torch.zeros_like(mask)), dict(fill=(1, 2, 3)), dict(pad=0.5), dict(box=(0.5, 0, 10, 10), square=True), dict(mask=mask[:-1])):
        with pytest.raises(lib.PbeError):
            exemplar.exemplar_from_picture(pic, **kw)
    # lists: [B][K], sizes differ per picture
    b = torch.from_numpy(np.array(P.source("random_37x53"))).to(dev)
    out = exemplar.exemplars_from_pictures([[pic, b], [b, pic]], boxes=[[(100, 400, 351, 901), None], [(1, 2, 52, 36), None]])
    assert out["ref"].shape == (2, 2, 3, 224, 224) and out["u8"].shape == (2, 2, 224, 224, 3) and out["boxes"][0][1] == (0, 0, 53, 37)
    assert np.array_equal(out["u8"][0, 0].cpu().numpy(), pil((100, 400, 351, 901))) and np.array_equal(out["u8"][1, 0].cpu().numpy(), pil((1, 2, 52, 36), P.source("random_37x53")))
    assert torch.equal(out["ref"][0, 1], ops.u8_to_planes(out["u8"][0, 1][None], *CLIP)[0]) and torch.equal(out["ref"][0, 1], exemplar.exemplar_from_picture(b)["ref"][0])
    with pytest.raises(lib.PbeError):
        exemplar.exemplars_from_pictures([[pic, b], [b]])
    # from files, with a mask file
    Image.fromarray(m, mode="L").save(str(tmp_path / "object.png"))
    e = preprocess.load_reference_device(os.path.join(P.GOLDEN, "reference_example_3.jpg"), dev, mask_path=str(tmp_path / "object.png"), pad=0.1)
    box = exemplar.plan_crop((400, 900, 100, 350), (H, W), 0.1)
    assert e["box"] == box and np.array_equal(e["u8"].cpu().numpy(), pil(box))


@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


def test_inpaint_with_the_device_cut_exemplar_equals_the_pil_cut_one(dev, narrow):
    from PIL import Image
    from pbe_amd import exemplar, ops, pipeline
    inp = cases.narrow_inputs()
    a = P.source("reference_example_3.jpg")
    pic = torch.from_numpy(np.array(a)).to(dev)
    boxes = [(100, 400, 351, 901), (0.5, 0.25, 700, 1200.5)]
    host = np.stack([np.array(Image.fromarray(a).resize((224, 224), box=b), dtype=np.uint8) for b in boxes])
    ref_host = ops.u8_to_planes(torch.from_numpy(host).to(dev), *CLIP)
    ref_dev = torch.cat([exemplar.exemplar_from_picture(pic, box=b)["ref"] for b in boxes])
    assert torch.equal(ref_dev, ref_host)
    kw = dict(steps=4, scale=5.0, x_T=inp["x_T"].to(dev), post_eps=inp["post_eps"])
    with torch.no_grad():
        one = pipeline.inpaint(narrow, inp["image"], inp["mask"], ref_dev, **kw)
        two = pipeline.inpaint(narrow, inp["image"], inp["mask"], ref_host, **kw)
    assert torch.equal(one["latent"], two["latent"]) and torch.equal(one["image"], two["image"])


# ---- 4. the CLI --------------------------------------------------------------------------------------------------------------------------
class _Cli:
    """scripts/inference.py on the bundled triple with the narrow model: run(tag, flags, references) -> {relative path: file bytes} of the
    output tree, each tag run once per module."""

    def __init__(self, root, golden_dir):
        import yaml
        from PIL import Image
        spec = importlib.util.spec_from_file_location("pbe_inference_cli_exemplar", os.path.join(ROOT, "scripts", "inference.py"))
        self.cli = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(self.cli)
        self.root, self.d, self.done = root, os.path.join(golden_dir, "examples"), {}
        self.refs = [os.path.join(self.d, f"reference_example_{i}.jpg") for i in (3, 1)]
        self.cfg = str(root / "narrow.yaml")
        with open(self.cfg, "w") as f:
            yaml.safe_dump({"model": build.narrow_config()}, f)
        self.picture = P.source("reference_example_3.jpg")
        m = np.zeros(self.picture.shape[:2], dtype=np.uint8)
        m[400:901, 100:351] = 255                                      # the "object": rows 400 .. 900, columns 100 .. 350
        self.object_box, self.object_png = (400, 900, 100, 350), str(root / "object.png")
        Image.fromarray(m, mode="L").save(self.object_png)

    def run(self, tag, extra, paths=None):
        if tag not in self.done:
            out = str(self.root / tag)
            self.cli.main(extra + ["--outdir", out, "--config", self.cfg, "--ddim_steps", "4", "--image_path", os.path.join(self.d, "image_example_1.png"),
                                   "--mask_path", os.path.join(self.d, "mask_example_1.png"), "--reference_path", *(paths or self.refs[:1]), "--seed", "321",
                                   "--scale", "5", "--fixed_code", "--random_weights"])
            files = {}
            for sub in sorted(os.listdir(out)):
                for n in sorted(os.listdir(os.path.join(out, sub))):
                    with open(os.path.join(out, sub, n), "rb") as fh:
                        files[f"{sub}/{n}"] = fh.read()
            self.done[tag] = files
        return self.done[tag]

    def crop(self, tag, k=0):
        from PIL import Image
        return np.asarray(Image.open(str(self.root / tag / "reference_crops" / f"image_example_1_ref{k}.png")))


@pytest.fixture(scope="module")
def cli(dev, golden_dir, tmp_path_factory):
    return _Cli(tmp_path_factory.mktemp("exemplar_cli"), golden_dir)


def _but_crops(files):
    return {k: v for k, v in files.items() if not k.startswith("reference_crops/")}


def test_inference_cli_reference_on_device(cli):
    """--reference_on_device writes the default run's files byte for byte, and the exemplar it cut is PIL's."""
    from PIL import Image
    plain, on_dev = cli.run("plain", []), cli.run("on_device", ["--reference_on_device"])
    assert len(plain) == 6 and not any(k.startswith("reference_crops/") for k in plain)
    assert _but_crops(on_dev) == plain and set(on_dev) - set(plain) == {"reference_crops/image_example_1_ref0.png"}
    assert np.array_equal(cli.crop("on_device"), np.array(Image.open(cli.refs[0]).convert("RGB").resize((224, 224))))


def test_inference_cli_reference_box_and_mask(cli):
    """--reference_box (two references, one fractional box) and --reference_mask --reference_square --reference_pad write
    reference_crops/ equal to Pillow's crop + resize, and change the result; counts that do not match the references are argparse errors."""
    from PIL import Image
    from pbe_amd import exemplar
    plain = cli.run("plain", [])
    boxes = ((100.5, 400, 351, 901.25), (0, 0, 960, 1277))
    boxed = cli.run("boxed", ["--reference_box"] + [str(v) for b in boxes for v in b], cli.refs)
    for k, (path, box) in enumerate(zip(cli.refs, boxes)):
        assert np.array_equal(cli.crop("boxed", k), np.array(Image.open(path).convert("RGB").resize((224, 224), box=box))), k
    assert boxed["results/image_example_1_321.png"] != plain["results/image_example_1_321.png"]
    masked = cli.run("masked", ["--reference_mask", cli.object_png, "--reference_square", "--reference_pad", "0.1"])
    box = exemplar.plan_crop(cli.object_box, cli.picture.shape[:2], 0.1, True)
    assert np.array_equal(cli.crop("masked"), np.array(Image.fromarray(cli.picture).resize((224, 224), box=box)))
    assert masked["results/image_example_1_321.png"] != plain["results/image_example_1_321.png"]
    base = ["--image_path", "i.png", "--mask_path", "m.png", "--reference_path", "a.jpg", "b.jpg"]
    for bad in (["--reference_box", "0", "0", "10", "10"], ["--reference_mask", "m.png"], ["--reference_mask", "a.png", "b.png", "--reference_fill", "1", "2", "300"],
                ["--reference_fill", "1", "2", "3"], ["--reference_pad", "0.5"], ["--reference_square"],
                ["--reference_box", "0", "0", "1", "1", "0", "0", "1", "1", "--reference_pad", "-1"]):
        with pytest.raises(SystemExit):
            cli.cli.parse(base + bad)
    ok = cli.cli.parse(base + ["--reference_box", "0", "0", "10", "10", "1", "1", "9", "9.5", "--reference_square"])
    assert cli.cli.reference_on_device(ok) and not cli.cli.reference_on_device(cli.cli.parse(base))


def test_inference_cli_reference_flags_per_hole(cli):
    """With --paste_back --per_hole --reference_per_hole and another sampler: the device path changes nothing, a box does."""
    from PIL import Image
    from pbe_amd import exemplar
    hole = ["--paste_back", "--per_hole", "--reference_per_hole", "--dpm_solver"]
    per_hole, per_hole_dev = cli.run("per_hole", hole), cli.run("per_hole_dev", hole + ["--reference_on_device"])
    assert "pasted/image_example_1_321.png" in per_hole and _but_crops(per_hole_dev) == per_hole
    per_hole_box = cli.run("per_hole_box", hole + ["--reference_box", "100", "400", "351", "901", "--reference_pad", "0.1"])
    assert per_hole_box["pasted/image_example_1_321.png"] != per_hole["pasted/image_example_1_321.png"]
    box = exemplar.plan_crop(cli.object_box, cli.picture.shape[:2], 0.1)
    assert np.array_equal(cli.crop("per_hole_box"), np.array(Image.fromarray(cli.picture).resize((224, 224), box=box)))
