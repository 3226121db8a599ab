"""CPU tests of the injection check's host side: SDSampler.get_timesteps against its three-line restatement, the duplication rule and
the draw order of prepare_latents_img2img (the launcher replaced by its f32 torch emulation), every refusal of the two new config
blocks -- each before any step -- and the record format of injection_rank0.jsonl."""
import json
import os

import numpy as np
import pytest
import torch

import injection_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pipe(monkeypatch=None, **kw):
    from siss_amd import sd_sampler
    if monkeypatch is not None:
        monkeypatch.setattr(sd_sampler, "latent_inject", R.inject_emul)
    return sd_sampler.SDSampler(unet=None, **kw)


# ---------------------------------------------------------------- get_timesteps
@pytest.mark.parametrize("N,strength", [(50, 0.5), (50, 1.0), (50, 0.019), (7, 0.3), (10, 1.7)])
def test_get_timesteps_matches_the_restatement(N, strength):
    from siss_amd.scheduler import DDIMScheduler
    pipe = _pipe()
    want, count = R.timesteps_ref(DDIMScheduler.from_pretrained(None).set_timesteps(N), N, strength)
    if not want:                                         # (50, 0.019): int(0.95) = 0 steps
        assert (N, strength) == (50, 0.019)
        with pytest.raises(ValueError, match="no denoising step"):
            pipe.get_timesteps(N, strength)
        return
    ts, n = pipe.get_timesteps(N, strength, device="cpu")
    assert ts == want and n == count == len(ts)
    assert pipe.scheduler.num_inference_steps == N       # the step's coefficients are those of the FULL schedule
    if (N, strength) == (50, 0.5):
        assert ts[0] == 481 and n == 25 and ts[-1] == 1
    if (N, strength) == (7, 0.3):
        assert n == 2 and ts == [143, 1]
    if strength >= 1.0:                                  # 1.7 clamps: the whole schedule
        assert n == N and ts[0] == pipe.scheduler.timesteps[0]


# ---------------------------------------------------------------- prepare_latents_img2img on the emulated launcher
def test_duplication_rule_and_latents_branch(monkeypatch):
    pipe = _pipe(monkeypatch)
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(2, 4, 5, 5, generator=g)
    a, b = R.scalars(pipe.scheduler.alphas_cumprod, 481)

    def run(image, bs, k, seed=7):
        gen = torch.Generator().manual_seed(seed)
        x = pipe.prepare_latents_img2img(image, 481, bs, k, device="cpu", generator=gen)
        noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed))      # latents draw the noise ONLY
        return x, noise

    x, noise = run(lat[:1], 3, 1)                        # m = 1 -> n = 3
    assert x.shape == (3, 4, 5, 5) and x.dtype == torch.float32
    assert torch.equal(x, a * lat[:1].expand(3, -1, -1, -1) + b * noise)                  # zero variance: mean + std * 0 = mean
    x, noise = run(lat, 2, 2)                            # m = 2 -> n = 4, tiled [0, 1, 0, 1]
    assert x.shape == (4, 4, 5, 5)
    assert torch.equal(x, a * lat[[0, 1, 0, 1]] + b * noise)
    assert not torch.equal(x, a * lat[[0, 0, 1, 1]] + b * noise)
    x, noise = run(lat, 1, 1)                            # fewer prompts than images: the images as they are
    assert torch.equal(x, a * lat + b * noise)
    with pytest.raises(ValueError, match="Cannot duplicate `image` of batch size 2 to 3"):
        run(lat, 3, 1)                                   # m = 2 -> n = 3
    with pytest.raises(NotImplementedError, match="list of generators"):
        pipe.prepare_latents_img2img(lat, 481, 2, 1, device="cpu", generator=[torch.Generator(), torch.Generator()])
    with pytest.raises(ValueError, match="vae_encoder"):
        pipe.prepare_latents_img2img(torch.zeros(1, 3, 16, 16), 481, 1, 1, device="cpu")


def test_vae_branch_draws_the_posterior_normals_first(monkeypatch):
    class Enc:
        cfg = type("C", (), dict(scaling_factor=0.18215))()

        def raw_moments(self, image):
            self.seen = image
            return mom

    mom = torch.randn(2, 8, 3, 3, generator=torch.Generator().manual_seed(1))
    enc = Enc()
    pipe = _pipe(monkeypatch, vae_encoder=enc)
    img = torch.zeros(2, 3, 24, 24)
    x = pipe.prepare_latents_img2img(img, 301, 2, 2, device="cpu", generator=torch.Generator().manual_seed(5))
    g = torch.Generator().manual_seed(5)
    eps_z = torch.randn(2, 4, 3, 3, generator=g)
    eps_t = torch.randn(4, 4, 3, 3, generator=g)
    a, b = R.scalars(pipe.scheduler.alphas_cumprod, 301)
    assert enc.seen.shape == img.shape and x.shape == (4, 4, 3, 3)
    assert torch.equal(x, R.inject_emul(mom, eps_z, eps_t, 0.18215, a, b))
    g = torch.Generator().manual_seed(5)                 # the noise first: another result
    eps_t2 = torch.randn(4, 4, 3, 3, generator=g)
    eps_z2 = torch.randn(2, 4, 3, 3, generator=g)
    assert not torch.equal(x, R.inject_emul(mom, eps_z2, eps_t2, 0.18215, a, b))


def test_denoise_injection_refuses_what_call_refuses():
    pipe = _pipe()
    e = torch.zeros(1, 77, 8)
    with pytest.raises(NotImplementedError, match="eta"):
        pipe.denoise_injection(torch.zeros(1, 4, 8, 8), e, eta=0.5)
    with pytest.raises(ValueError, match="output_type"):
        pipe.denoise_injection(torch.zeros(1, 4, 8, 8), e, output_type="pt")
    with pytest.raises(ValueError, match="VAE decoder"):
        pipe.denoise_injection(torch.zeros(1, 4, 8, 8), e, output_type="np")


def test_entry_point_is_declared_and_bound():
    from siss_amd import lib
    from siss_amd.build import EXACT
    assert "injection.hip" in EXACT
    assert "siss_latent_inject" in lib.F32_SAME
    assert lib.PARAMS["siss_latent_inject"] == ("moments", "moments_bf16", "eps_z", "eps_t", "x", "m", "n", "chw", "scaling", "a",
                                                "b", "nblk", "stream")


# ---------------------------------------------------------------- the record
def test_injection_record_format(tmp_path):
    from siss_amd.sscd import InjectionScore

    class Emulated(InjectionScore):                      # the scorer without its network: fixed scores per call
        def score_u8(self, u8):
            return torch.tensor([0.25, -0.5, 1.0, 0.1][:u8.shape[0]], dtype=torch.float32)

    out = tmp_path / "injection_rank0.jsonl"
    tr = Emulated(None, "forget.png", str(out), [0.5], [0.5])
    u8 = torch.zeros(4, 8, 8, 3, dtype=torch.uint8)
    vals = tr.score_u8(u8)
    rec = tr.record(vals, 3, 250)
    want = {"global_step": 3, "timestep": 250, "sscd_mean": float(vals.double().mean()), "sscd_max": 1.0,
            "sscd": [float(v) for v in vals.double()]}
    assert rec == want and list(rec) == ["global_step", "timestep", "sscd_mean", "sscd_max", "sscd"]
    assert rec["sscd_mean"] != float(vals.mean())        # f64 on the host, not the f32 mean
    tr.record(tr.score_u8(u8[:2]), 4, 250)
    lines = [json.loads(l) for l in open(out)]
    assert len(lines) == 2 and lines[0] == want          # one line per evaluation
    assert lines[1] == {"global_step": 4, "timestep": 250, "sscd_mean": -0.125, "sscd_max": 0.25, "sscd": [0.25, -0.5]}


# ---------------------------------------------------------------- refusals, each before any step
NORMALIZE = ("{_target_: torchvision.transforms.Compose, transforms: [{_target_: torchvision.transforms.Normalize, "
             "mean: [0.485, 0.456, 0.406], std: [0.229, 0.224, 0.225]}]}")


def _compose(name, tmp_path, *overrides):
    from siss_amd import hydra_lite as H
    return H.compose(name, os.path.join(ROOT, "config"), [f"output_dir={tmp_path}/out", *overrides])


def _checked(cls, cfg):
    task = cls(cfg)                                      # what run() does before it loads anything onto the device
    task.fill_cfg()
    task.check_supported()
    task.check_metrics()
    return task


def test_blocks_absent_check_metrics_passes_as_before(tmp_path):
    from siss_amd.tasks import DeleteCeleb, DeleteSD, DeleteTShirt
    for cls, name in ((DeleteCeleb, "delete_celeb"), (DeleteTShirt, "delete_tshirt"), (DeleteSD, "delete_sd")):
        task = _checked(cls, _compose(name, tmp_path))
        assert task.injection is None
    # the timestep alone (what the pixel-space tasks already read) configures no score
    assert _checked(DeleteCeleb, _compose("delete_celeb", tmp_path, "metrics.denoising_injections.timestep=3")).injection is None
    assert not os.path.exists(tmp_path / "out")


def test_pixel_space_refusals(tmp_path, capsys):
    from PIL import Image
    from siss_amd.sscd import InjectionScore
    from siss_amd.tasks import DeleteCeleb, DeleteTShirt
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / "forget.png"))
    img = f"metrics.denoising_injections.img_path={tmp_path}/forget.png"
    model = f"metrics.denoising_injections.sscd.model_path={tmp_path}/missing.pt"
    rand = "metrics.denoising_injections.sscd.allow_random_init=true"

    def check(*ov, cls=DeleteCeleb, name="delete_celeb"):
        return _checked(cls, _compose(name, tmp_path, *ov)).injection

    with pytest.raises(ValueError, match="model_path"):
        check(img, "metrics.denoising_injections.sscd=true")
    with pytest.raises(FileNotFoundError, match="model_path.*not a file"):
        check(img, model)                                # missing, and allow_random_init not given
    with pytest.raises(ValueError, match="in_channels=1"):
        check(img, model, rand, "unet.in_channels=1")
    with pytest.raises(ValueError, match="in_channels=1"):
        check(img, model, rand, cls=DeleteTShirt, name="delete_tshirt")     # the MNIST architecture
    with pytest.raises(FileNotFoundError, match="img_path"):
        check(model, rand)
    with pytest.raises(FileNotFoundError, match="img_path"):
        check(f"metrics.denoising_injections.img_path={tmp_path}/gone.png", model, rand)
    tot = NORMALIZE.replace("transforms: [", "transforms: [{_target_: torchvision.transforms.ToTensor}, ")
    with pytest.raises(ValueError, match="exactly one Normalize"):
        check(img, model, rand, f"metrics.denoising_injections.sscd.data_transforms={tot}")
    capsys.readouterr()
    tr = check(img, model, rand, f"metrics.denoising_injections.sscd.data_transforms={NORMALIZE}")
    said = capsys.readouterr().out
    assert isinstance(tr, InjectionScore) and tr.mean == [0.485, 0.456, 0.406] and tr.mem_img_path == f"{tmp_path}/forget.png"
    assert tr.out_path == f"{tmp_path}/out/injection_rank0.jsonl"
    assert "RANDOM-INIT" in said and "eval_every is not" in said           # eval_every unset: a warning, as for the SD checks
    capsys.readouterr()
    assert check(img, model, "allow_random_init=true", "eval_every=1").mean == [0.0] * 3   # the top-level switch; no transform
    assert "eval_every is not" not in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "out")


def test_delete_sd_refusals(tmp_path, capsys):
    from PIL import Image
    from siss_amd.tasks import DeleteSD
    ckpt = tmp_path / "ckpt"
    (ckpt / "vae").mkdir(parents=True)
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / "mem.png"))
    base = [f"base_dir={tmp_path}", f"pretrained_model_name_or_path={ckpt}", f"data_files.mem_img_path={tmp_path}/mem.png"]
    inj = "metrics.denoising_injections.strength=0.5"

    def check(*ov):
        return _checked(DeleteSD, _compose("delete_sd", tmp_path, *ov)).injection

    assert _compose("delete_sd", tmp_path).metrics.denoising_injections is None            # the shipped default
    assert check(*base) is None
    capsys.readouterr()
    got = check(*base, inj, "metrics.denoising_injections.num_images=4")
    assert got == dict(strength=0.5, num_images=4, prompt=0, mem_img_path=f"{tmp_path}/mem.png")
    assert "eval_every is not" in capsys.readouterr().out
    with pytest.raises(FileNotFoundError, match="vae"):
        check(base[0], f"pretrained_model_name_or_path={tmp_path}/nowhere", base[2], inj)
    with pytest.raises(FileNotFoundError, match="mem_img_path"):
        check(*base[:2], inj)
    with pytest.raises(FileNotFoundError, match="mem_img_path"):
        check(*base[:2], f"data_files.mem_img_path={tmp_path}/gone.png", inj)
    with pytest.raises(ValueError, match="no denoising step"):
        check(*base, "metrics.denoising_injections.strength=0.019")                        # 0.019 * 50 < 1
    with pytest.raises(ValueError, match="no denoising step"):
        check(*base, inj, "+pipeline.num_inference_steps=1")                               # 0.5 * 1 < 1
    with pytest.raises(ValueError, match="strength"):
        check(*base, "metrics.denoising_injections.strength=-1")
    with pytest.raises(ValueError, match="num_images"):
        check(*base, inj, "metrics.denoising_injections.num_images=0")
    with pytest.raises(ValueError, match="prompt"):
        check(*base, inj, "metrics.denoising_injections.prompt=1")                         # validation_prompts has one entry
    assert not os.path.exists(tmp_path / "out")
