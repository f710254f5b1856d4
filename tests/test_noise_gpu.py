"""Noise from per-sample seeds on the GPU: pbe_philox_u32 against the numpy Philox of tests/noiseref.py by equality, pbe_randn_philox_f32
against the float64 value of its definition per element, placement invariance and the accumulate form by bits, the statistics of the
device output, and seeds= through the three samplers and the pipeline on the narrow model against the same tensors handed in.

No test here judges picture quality: the weights are name-seeded noise."""
import os

import numpy as np
import pytest
import torch

import cases
import guard
import modelbuild as build
import noiseref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [f"n{n}-B{len(s)}-{i}" for i, (n, s, _, _) in enumerate(nr.CASES)]


def _out(B, n, dtype, dev):
    flat, arena = guard.sentinel_out((B * n,), dtype=dtype, device=dev)
    return flat.view(B, n), arena, flat


def _written(arena, flat, what):
    guard.assert_untouched(arena, flat, what)
    guard.assert_fully_written(flat, what)


def _draw(dev, seeds, n, stream, sub=None):
    from pbe_amd import ops
    return ops.randn_seeded(list(seeds), (len(seeds), n), stream, sub=sub)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. raw words ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nr.CASES, ids=CASE_IDS)
def test_philox_words_equal_the_reference(dev, case):
    from pbe_amd import ops
    n, seeds, sub, stream = case
    out, arena, flat = _out(len(seeds), n, torch.int32, dev)
    got = ops.philox_u32(list(seeds), n, stream, sub=None if sub is None else list(sub), out=out)
    assert got is out
    _written(arena, flat, f"pbe_philox_u32 {case}")
    want = np.stack([nr.words(s, 0 if sub is None else sub[b], stream, n) for b, s in enumerate(seeds)])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)


def test_philox_known_answers_on_the_device(dev):
    """The three Random123 vectors: the key is the seed, the counter's words are q, sub and the stream - q = 0xffffffff and 0x243f6a88
    would need 2^34 words, so those two are reached through sub / stream with q = 0 checked against numpy, and the first directly."""
    from pbe_amd import ops
    w = ops.philox_u32([0], 4, 0).cpu().numpy().view(np.uint32)[0]
    assert [int(x) for x in w] == list(nr.KAT[0][2])
    for ctr, key, _ in nr.KAT[1:]:
        seed, sub, stream = key[0] | (key[1] << 32), ctr[1] & 0x7fffffff, ctr[2] | (ctr[3] << 32)
        w = ops.philox_u32([seed], 8, stream, sub=[sub]).cpu().numpy().view(np.uint32)[0]
        assert np.array_equal(w, nr.words(seed, sub, stream, 8))


# ---- 2. floats ---------------------------------------------------------------------------------------------------------------------------
_ERR = {}


@pytest.mark.parametrize("case", nr.CASES, ids=CASE_IDS)
def test_randn_against_float64(dev, case):
    from pbe_amd import ops
    n, seeds, sub, stream = case
    out, arena, flat = _out(len(seeds), n, torch.float32, dev)
    ops.randn_seeded(list(seeds), (len(seeds), n), stream, sub=None if sub is None else list(sub), out=out)
    _written(arena, flat, f"pbe_randn_philox_f32 {case}")
    got = out.cpu().numpy().astype(np.float64)
    want = np.stack([nr.randn64(s, 0 if sub is None else sub[b], stream, n) for b, s in enumerate(seeds)])
    assert np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    _ERR[case] = err
    print(f"randn_seeded {case}: max |device - float64| = {err:.3e} (largest so far {max(_ERR.values()):.3e}, gate {nr.RANDN_ABS_TOL})")
    assert nr.RANDN_ABS_TOL is not None and nr.RANDN_ABS_TOL == 4 * nr.RANDN_MEASURED_MAX_ABS_ERR
    assert err <= nr.RANDN_ABS_TOL, err


def test_unit_uniform_gives_zeros(dev):
    for seed, sub, stream, elems in nr.ZERO_RADIUS:
        z = _draw(dev, [seed], 4, stream, sub=[sub]).cpu().numpy()[0]
        assert np.isfinite(z).all() and all(z[e] == 0.0 for e in elems), (seed, sub, z)
        other = [e for e in range(4) if e not in elems]
        assert np.abs(z[other] - nr.randn64(seed, sub, stream, 4)[other]).max() <= nr.RANDN_ABS_TOL


# ---- 3. placement invariance, by bits ---------------------------------------------------------------------------------------------------------
def test_placement_invariance(dev):
    seeds, sub, stream = [nr.SEEDS[3], 1, nr.SEEDS[4]], [1, (1 << 31) - 1, 0], 16
    for n in (5, 1023, 1024, 4 * 33 * 47):
        three = _draw(dev, seeds, n, stream, sub=sub)
        for b in range(3):                                                      # the sample's place in the batch and B (an odd n also moves
            one = _draw(dev, seeds[b:b + 1], n, stream, sub=sub[b:b + 1])       # samples 1, 2 off 16 bytes: the scalar path wrote them)
            assert torch.equal(_bits(three[b]), _bits(one[0])), (n, b)
        assert torch.equal(_bits(three), _bits(_draw(dev, seeds, n, stream, sub=sub))), n       # two runs
    for n in (4, 1024, 4 * 33 * 47):                                            # n: a prefix of a longer draw
        longer, short = _draw(dev, seeds, n + 1028, stream, sub=sub), _draw(dev, seeds, n, stream, sub=sub)
        assert torch.equal(_bits(longer[:, :n]), _bits(short)), n
    from pbe_amd import ops
    for n in (5, 1024, 1025):                                                   # the output pointer one float off 16 bytes
        buf = torch.full((n + 8,), float("nan"), device=dev)
        assert buf.data_ptr() % 16 == 0
        off = ops.randn_seeded(seeds[:1], (1, n), stream, sub=sub[:1], out=buf[1:1 + n].view(1, n))
        assert off.data_ptr() % 16 == 4
        assert torch.equal(_bits(off), _bits(_draw(dev, seeds[:1], n, stream, sub=sub[:1]))), n
        assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + n:]).all())
    # words the same way
    w3 = ops.philox_u32(seeds, 1025, stream, sub=sub)
    for b in range(3):
        assert torch.equal(w3[b], ops.philox_u32(seeds[b:b + 1], 1025, stream, sub=sub[b:b + 1])[0])


# ---- 4. the accumulate form ---------------------------------------------------------------------------------------------------------------------
def test_accumulate_form(dev):
    from pbe_amd import ops
    seeds, stream, s = [7, nr.SEEDS[3], 1 << 32], 17, 0.372
    for n in (5, 1025, 4 * 33 * 47):
        plain = _draw(dev, seeds, n, stream)
        poisoned = torch.full((3, n), float("nan"), device=dev)
        assert torch.equal(_bits(ops.randn_seeded(seeds, (3, n), stream, out=poisoned)), _bits(plain))          # a = 0 never reads out
        base = torch.from_numpy(np.random.default_rng(n).standard_normal((3, n)).astype(np.float32)).to(dev)
        acc = ops.randn_seeded(seeds, (3, n), stream, out=base.clone(), a=1.0, b=s)
        exact = base.cpu().numpy().astype(np.float64) + float(np.float32(s)) * plain.cpu().numpy().astype(np.float64)
        want = exact.astype(np.float32)                                                                         # the fused rounding
        ulp = np.spacing(np.abs(want))
        got = acc.cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), float(np.abs(got - want).max())
        axpy = ops.axpy_(base.clone(), s, plain).cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - axpy) <= ulp)
        print(f"accumulate n={n}: bits equal ops.axpy_: {np.array_equal(got.view(np.uint32), axpy.view(np.uint32))}, equal the fused rounding: "
              f"{np.array_equal(got, want)}")
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError):
        ops.randn_seeded(seeds, (3, 8), stream, a=1.0)                                                          # nothing to accumulate into
    with pytest.raises(PbeError):
        ops.randn_seeded(seeds, (2, 8), stream)                                                                 # 3 seeds, 2 samples
    with pytest.raises(PbeError):
        ops.randn_seeded(seeds, (3, 8), stream, out=torch.zeros(3, 8))                                          # a CPU tensor


# ---- 5. statistics of the device output ---------------------------------------------------------------------------------------------------------
def test_device_statistics(dev):
    nr.check_stats(lambda seed, stream, n: _draw(dev, [seed], n, stream).cpu().numpy()[0])


# ---- 6. samplers ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(dev):
    with torch.no_grad():
        return build.narrow_model(dev)


@pytest.fixture(scope="module")
def opt(dev):
    return {k: v.to(dev) for k, v in cases.sampler_option_inputs().items() if k != "noises"}


@pytest.fixture
def launches(monkeypatch):
    """Counts the calls of the loaded pbe_randn_philox_f32 symbol."""
    from pbe_amd import lib
    L = lib.load()
    real, count = L.pbe_randn_philox_f32, []
    monkeypatch.setattr(L, "pbe_randn_philox_f32", lambda *a: (count.append(1), real(*a))[1])
    return count


def _make(kind, narrow):
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.plms import PLMSSampler
    return {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}[kind](narrow)


SEEDS2, SUB2, S = [5, 9], [0, 3], 4


def _skw(opt, kind):
    return dict(S=S, batch_size=2, shape=[4, 16, 16], conditioning=opt["c"], verbose=False, unconditional_guidance_scale=5.0,
                unconditional_conditioning=opt["uc"], eta=0.7 if kind == "ddim" else 0.0, mask=opt["blend_mask"], x0=opt["x0"],
                test_model_kwargs={"images_inpaint": opt["z_inpaint"], "images_mask": opt["mask_lat"]})


@pytest.mark.parametrize("kind", ["plms", "ddim", "dpm"])
def test_sampler_seeds_equal_the_streams_by_hand(dev, narrow, opt, kind, launches):
    """sample(seeds=[5, 9]) with the mask / x0 blend (and, for DDIM, eta = 0.7) against the same sampler given x_T = stream 0 and a
    noise_like that returns streams 16, 17, ... in the order it is asked: bit for bit."""
    from pbe_amd import ops
    from pbe_amd.lib import PbeError
    with torch.no_grad():
        z_seeded, _ = _make(kind, narrow).sample(seeds=SEEDS2, seed_sub=SUB2, **_skw(opt, kind))
        draws = len(launches)
        assert draws == 1 + S * (2 if kind == "ddim" else 1)                    # x_T, one blend per step, DDIM's sigma term per step
        hand = _make(kind, narrow)
        asked = []
        hand.noise_like = lambda shape, device: (asked.append(1), ops.randn_seeded(SEEDS2, shape, nr.STREAM_STEP0 + len(asked) - 1, sub=SUB2))[1]
        z_hand, _ = hand.sample(x_T=ops.randn_seeded(SEEDS2, (2, 4, 16, 16), nr.STREAM_X_T, sub=SUB2), **_skw(opt, kind))
        assert len(asked) == draws - 1
        assert torch.equal(_bits(z_seeded), _bits(z_hand))
        swapped, _ = _make(kind, narrow).sample(seeds=SEEDS2[::-1], seed_sub=SUB2[::-1], **_skw(opt, kind))
        assert not torch.equal(swapped, z_seeded) and bool(torch.isfinite(z_seeded).all())
        with pytest.raises(PbeError):
            _make(kind, narrow).sample(seeds=SEEDS2, x_T=z_hand, **_skw(opt, kind))
        with pytest.raises(PbeError):
            _make(kind, narrow).sample(seeds=[5], **_skw(opt, kind))
        # without seeds: not one launch of the new kernel, and the overridden attribute is what draws
        before = len(launches)
        s = _make(kind, narrow)
        assert s._seeded is None
        it = iter([torch.full((2, 4, 16, 16), 0.25, device=dev)] * (2 * S))
        s.noise_like = lambda shape, device: next(it)
        s.sample(x_T=opt["x_T"], **_skw(opt, kind))
        assert len(launches) == before and s._seeded is None


# ---- 7. pipeline ----------------------------------------------------------------------------------------------------------------------------------
def test_inpaint_seeds_equal_the_tensors_by_hand(dev, narrow, launches):
    from pbe_amd import ops, pipeline
    from pbe_amd.lib import PbeError
    inp = {k: v.to(dev) for k, v in cases.narrow_inputs().items() if k in ("image", "mask", "ref")}
    kw = dict(steps=4, scale=5.0)
    with torch.no_grad():
        seeded = pipeline.inpaint(narrow, inp["image"], inp["mask"], inp["ref"], seeds=[3, 4], **kw)
        assert len(launches) == 2 and seeded["seeds"].tolist() == [3, 4]
        x_T, eps = ops.randn_seeded([3, 4], (2, 4, 16, 16), nr.STREAM_X_T), ops.randn_seeded([3, 4], (2, 4, 16, 16), nr.STREAM_POST_EPS)
        hand = pipeline.inpaint(narrow, inp["image"], inp["mask"], inp["ref"], x_T=x_T, post_eps=eps, **kw)
        for k in ("image", "latent", "z_inpaint"):
            assert torch.equal(_bits(seeded[k].float()), _bits(hand[k].float())), k
        assert "seeds" not in hand
        # sample 1 alone, in a batch of one: the same picture's noise (the bits of the picture itself depend on the tile choice, not gated)
        for bad in (dict(x_T=x_T), dict(post_eps=eps)):
            with pytest.raises(PbeError):
                pipeline.inpaint(narrow, inp["image"], inp["mask"], inp["ref"], seeds=[3, 4], **bad, **kw)
        with pytest.raises(PbeError):
            pipeline.inpaint(narrow, inp["image"], inp["mask"], inp["ref"], seeds=[3], **kw)
        before = len(launches)
        pipeline.inpaint(narrow, inp["image"], inp["mask"], inp["ref"], **kw)
        assert len(launches) == before                                          # the default draws are torch's, as before


def _holes_picture(dev, fourth=False):
    import windowref as wr
    pic = wr.random_picture((300, 400), 61)
    mask = np.zeros((300, 400), dtype=np.uint8)
    mask[30:50, 40:70] = 255
    mask[150:170, 300:330] = 255
    mask[250:270, 60:90] = 255
    if fourth:
        mask[100:115, 180:200] = 255                                            # in raster order between the first and the second
    return torch.from_numpy(pic).to(dev), torch.from_numpy(mask).to(dev)


def test_inpaint_holes_noise_does_not_depend_on_the_company(dev, narrow, monkeypatch):
    """Three well-separated holes, one picture seed: the x_T and post_eps each window receives are the same bits at batch = None, 1, 2 and
    with a fourth hole in the mask.  They are captured where inpaint hands them on: the sampler's start latent and the posterior's noise."""
    from ldm.models.diffusion.plms import PLMSSampler
    from pbe_amd import ops, pipeline
    ref = cases.narrow_inputs()["ref"][:1].to(dev)
    got = {}

    real_sampling, real_encoding = PLMSSampler.plms_sampling, narrow.get_first_stage_encoding

    def sampling(self, cond, shape, x_T=None, **kw):
        got.setdefault("x_T", []).append(x_T.clone())
        return real_sampling(self, cond, shape, x_T=x_T, **kw)

    def encoding(post, noise=None):
        got.setdefault("post_eps", []).append(noise.clone())
        return real_encoding(post, noise=noise)
    monkeypatch.setattr(PLMSSampler, "plms_sampling", sampling)
    monkeypatch.setattr(narrow, "get_first_stage_encoding", encoding)

    def run(fourth=False, seeds=(11,), **kw):
        got.clear()
        dp, dm = _holes_picture(dev, fourth)
        with torch.no_grad():
            out = pipeline.inpaint_holes(narrow, [dp], [dm], ref, size=(128, 128), feather=8, steps=2, scale=5.0, seeds=list(seeds), **kw)
        return out, {h["sub"]: (x, e) for h, x, e in zip(out["holes"], torch.cat(got["x_T"]), torch.cat(got["post_eps"]))}

    out, base = run()
    firsts = [30 * 400 + 40, 150 * 400 + 300, 250 * 400 + 60]
    assert [(h["seed"], h["sub"]) for h in out["holes"]] == [(11, f + 1) for f in firsts] and out["seeds"].tolist() == [11, 11, 11]
    for sub, (x, e) in base.items():                                            # what the plan says they are
        assert torch.equal(x, ops.randn_seeded([11], (1, 4, 16, 16), nr.STREAM_X_T, sub=[sub])[0])
        assert torch.equal(e, ops.randn_seeded([11], (1, 4, 16, 16), nr.STREAM_POST_EPS, sub=[sub])[0])
    assert not torch.equal(base[firsts[0] + 1][0], base[firsts[1] + 1][0])
    lat = {None: out["latent"]}
    for batch in (1, 2):
        o, other = run(batch=batch)
        lat[batch] = o["latent"]
        assert set(other) == set(base)
        for sub in base:
            assert torch.equal(_bits(other[sub][0]), _bits(base[sub][0])) and torch.equal(_bits(other[sub][1]), _bits(base[sub][1])), (batch, sub)
    rel = float((lat[1].double() - lat[None].double()).norm() / lat[None].double().norm())
    print(f"inpaint_holes seeds=[11]: rel-L2 of the latents, batch=1 against batch=None: {rel:.3e} (not gated: the tile choice depends on M)")
    o4, four = run(fourth=True)
    assert len(o4["holes"]) == 4 and set(base) < set(four)
    for sub in base:
        assert torch.equal(_bits(four[sub][0]), _bits(base[sub][0])) and torch.equal(_bits(four[sub][1]), _bits(base[sub][1])), sub
    # one seed per window: sub = 0, and window 1 re-rolled alone leaves the others their noise
    oN, _ = run(seeds=(11, 12, 13))
    assert [(h["seed"], h["sub"]) for h in oN["holes"]] == [(11, 0), (12, 0), (13, 0)]
    a = torch.cat(got["x_T"]).clone()
    run(seeds=(11, 99, 13))
    b = torch.cat(got["x_T"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])
    from pbe_amd.lib import PbeError
    with pytest.raises(PbeError):
        run(seeds=(1, 2))


# ---- 8. the CLI: fresh child processes, each under its own time limit -----------------------------------------------------------------------------
CLI_TIMEOUT = 240            # seconds per child: a narrow model, 4 steps - the limit only ends a child that hangs


class _Cli:
    def __init__(self, root, golden_dir):
        import yaml
        from PIL import Image
        import windowref as wr
        self.root, d = root, os.path.join(golden_dir, "examples")
        self.cfg = str(root / "narrow.yaml")
        with open(self.cfg, "w") as f:
            yaml.safe_dump({"model": build.narrow_config()}, f)
        self.common = ["--config", self.cfg, "--ddim_steps", "4", "--scale", "5", "--random_weights", "--seed", "321", "--reference_path",
                       os.path.join(d, "reference_example_1.jpg")]
        self.triple = ["--image_path", os.path.join(d, "image_example_1.png"), "--mask_path", os.path.join(d, "mask_example_1.png")]
        mask = np.zeros((300, 400), dtype=np.uint8)
        mask[30:50, 40:70] = 255
        mask[150:170, 300:330] = 255
        Image.fromarray(wr.random_picture((300, 400), 61)).save(str(root / "picture.png"))
        Image.fromarray(mask, mode="L").save(str(root / "mask.png"))
        self.holes = ["--image_path", str(root / "picture.png"), "--mask_path", str(root / "mask.png"), "--paste_back", "--per_hole", "--H", "128", "--W", "128"]

    def run(self, tag, args, ok=True):
        import subprocess
        import sys
        out = str(self.root / tag)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "inference.py"), "--outdir", out, *self.common, *args], capture_output=True,
                           text=True, timeout=CLI_TIMEOUT)
        assert (r.returncode == 0) == ok, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        files = {}
        if ok:
            for sub in sorted(os.listdir(out)):
                for n in sorted(os.listdir(os.path.join(out, sub))):
                    with open(os.path.join(out, sub, n), "rb") as fh:
                        files[f"{sub}/{n}"] = fh.read()
        return files, r.stdout + r.stderr


@pytest.fixture(scope="module")
def cli(dev, golden_dir, tmp_path_factory):
    return _Cli(tmp_path_factory.mktemp("noise_cli"), golden_dir)


def _tree(stem, tag):
    return {f"results/{stem}_{tag}.png", f"grid/grid-{stem}_{tag}.png", f"source/{stem}_{tag}_mask.png", f"source/{stem}_{tag}_GT.png",
            f"source/{stem}_{tag}_inpaint.png", f"source/{stem}_{tag}_ref.png"}


def test_cli_seeds_write_one_tree_per_seed(cli):
    dump = str(cli.root / "seeds.npz")
    files, _ = cli.run("seeds", cli.triple + ["--seeds", "1", "2", "--dump_tensors", dump])
    assert set(files) == _tree("image_example_1", 1) | _tree("image_example_1", 2)
    d = np.load(dump)                                                           # the noise the run used is the plan's: streams 0 and 1 of each seed
    for key, stream in (("x_T", nr.STREAM_X_T), ("post_eps", nr.STREAM_POST_EPS)):
        assert d[key].shape == (2, 4, 64, 64)
        for i, seed in enumerate((1, 2)):
            assert np.abs(d[key][i].reshape(-1) - nr.randn64(seed, 0, stream, 4 * 64 * 64)).max() <= nr.RANDN_ABS_TOL, (key, seed)
    assert files["results/image_example_1_1.png"] != files["results/image_example_1_2.png"]
    for k in ("mask", "GT", "inpaint", "ref"):                                  # one triple
        assert files[f"source/image_example_1_1_{k}.png"] == files[f"source/image_example_1_2_{k}.png"]


def test_cli_without_seeds_is_the_run_it_was(cli):
    """No --seeds: the six files under their usual names, the same bytes from two child processes (the start code fixed: --seed seeds
    torch's generators as always) - and the flags that exclude --seeds say so before any work."""
    a, _ = cli.run("plain_a", cli.triple + ["--fixed_code"])
    b, _ = cli.run("plain_b", cli.triple + ["--fixed_code"])
    assert set(a) == _tree("image_example_1", 321) and a == b
    for bad in (["--seeds", "1", "--fixed_code"], ["--seeds", "1", "--n_samples", "2"], ["--hole_seed", "0", "5"], ["--seeds", "3", "3"]):
        import importlib.util
        spec = importlib.util.spec_from_file_location("pbe_inference_cli_noise", os.path.join(ROOT, "scripts", "inference.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        with pytest.raises(SystemExit):
            mod.parse(cli.triple + bad)


def test_cli_hole_seed_rerolls_one_hole(cli):
    base, out0 = cli.run("holes", cli.holes + ["--seeds", "1"])
    again, out1 = cli.run("holes_reroll", cli.holes + ["--seeds", "1", "--hole_seed", "1", "99"])
    subs = [30 * 400 + 40 + 1, 150 * 400 + 300 + 1]
    assert f"noise (seed, sub) = (1, {subs[0]})" in out0 and f"noise (seed, sub) = (1, {subs[1]})" in out0
    assert f"noise (seed, sub) = (1, {subs[0]})" in out1 and "noise (seed, sub) = (99, 0)" in out1
    assert set(base) == set(again) == _tree("picture_hole0", 1) | _tree("picture_hole1", 1) | {"pasted/picture_1.png"}
    assert base["results/picture_hole0_1.png"] == again["results/picture_hole0_1.png"]           # hole 0 kept its noise: the same bytes
    assert base["results/picture_hole1_1.png"] != again["results/picture_hole1_1.png"]           # hole 1 was drawn again
    assert base["pasted/picture_1.png"] != again["pasted/picture_1.png"]
