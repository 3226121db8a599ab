"""The quality metrics' host side (no GPU): the target remaps and refusals, the Inception Score against an f64 restatement, the
T-shirt matcher's strict threshold, the metric tracker (fraction -> deletion_steps -> score trigger) on injected images, and the
refusals of a metrics block that cannot run -- before any step."""
import json
import math
import os

import pytest
import torch

from classifier_ref import inception_score_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the config surface
def test_target_remaps_resolve_and_the_yaml_classifier_node_builds():
    from siss_amd import classifier as Cl
    from siss_amd import hydra_lite as H
    assert H.get_object("metrics.classifier.Classifier") is Cl.Classifier
    assert H.get_object("metrics.inception_score.InceptionScore") is Cl.InceptionScore
    assert H.get_object("metrics.mnist_resnet.resnet18") is Cl.resnet18
    assert H.get_object("metrics.tshirt.TShirtClassifier") is Cl.TShirtClassifier
    assert H.get_object("hydra.utils.get_object") is H.get_object
    # the reference's classifier_cfg.classifier node resolves to the function itself
    node = H.Cfg({"_target_": "hydra.utils.get_object", "path": "metrics.mnist_resnet.resnet18"})
    assert H.instantiate(node) is Cl.resnet18
    m = Cl.resnet18(num_classes=11, grayscale=False)
    sd = m.state_dict()
    assert sd["conv1.weight"].shape == (64, 3, 7, 7) and sd["fc.weight"].shape == (11, 512)
    assert "layer2.0.downsample.0.weight" in sd and "layer1.0.downsample.0.weight" not in sd


@pytest.mark.parametrize("path", ["metrics.cifar_resnet.resnet56", "torch.hub.load"])
def test_classifiers_that_are_not_built_are_refused(path):
    from siss_amd import hydra_lite as H
    with pytest.raises(NotImplementedError, match=path.split(".")[0] + r"\." + path.split(".")[1]):
        H.get_object(path)
    with pytest.raises(NotImplementedError):
        H.instantiate(H.Cfg({"_target_": "hydra.utils.get_object", "path": path}))


def test_reference_init_and_strict_state_dict():
    from classifier_ref import make
    from siss_amd.classifier import resnet18
    ref = make(10, True, seed=0, randomize_bn=False)
    m = resnet18(10, True)
    assert list(m.state_dict()) == list(ref.state_dict())
    for k, v in m.state_dict().items():
        assert v.shape == ref.state_dict()[k].shape, k
    # the reference's init: conv N(0, sqrt(2 / (k^2 Cout))), BN 1 / 0 with stats 0 / 1, fc U(-1/sqrt(512), 1/sqrt(512))
    sd = m.state_dict()
    w = sd["layer4.1.conv2.weight"]
    assert abs(float(w.std()) / math.sqrt(2 / (9 * 512)) - 1) < 0.02
    assert bool((sd["bn1.weight"] == 1).all() and (sd["bn1.bias"] == 0).all() and (sd["bn1.running_var"] == 1).all())
    assert float(sd["fc.weight"].abs().max()) <= 1 / math.sqrt(512)
    # strict: only num_batches_tracked may be missing
    full = ref.state_dict()
    m.load_state_dict({k: v for k, v in full.items() if not k.endswith("num_batches_tracked")})
    assert torch.equal(m.state_dict()["fc.weight"], full["fc.weight"])
    with pytest.raises(RuntimeError, match="missing"):
        m.load_state_dict({k: v for k, v in full.items() if k != "fc.bias"})
    with pytest.raises(RuntimeError, match="unexpected"):
        m.load_state_dict(dict(full, **{"avgpool.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="shape"):
        m.load_state_dict(dict(full, **{"fc.weight": torch.zeros(11, 512)}))
    # H or W > 32 is refused before anything runs
    with pytest.raises(ValueError, match="32"):
        m(torch.zeros(1, 1, 33, 28))


# ---------------------------------------------------------------- 2. the Inception Score
class _Logits:
    def __init__(self, logits):
        self.logits = logits

    def compute_logits(self, imgs):
        return self.logits[imgs]


@pytest.mark.parametrize("n, splits, remove_class", [(40, 10, None), (11, 10, None), (1, 10, None), (40, 10, 3), (23, 4, 0)])
def test_inception_score_against_f64(n, splits, remove_class):
    from siss_amd.classifier import InceptionScore
    g = torch.Generator().manual_seed(n)
    logits = torch.randn(n, 10, generator=g, dtype=torch.float64) * 3
    if remove_class is not None:
        logits[: n // 4, remove_class] += 20                        # a quarter of the rows are dropped
    ic = InceptionScore(_Logits(logits), splits=splits, remove_class=remove_class)
    ic.update(torch.arange(n // 2))
    ic.update(torch.arange(n // 2, n))                           # two updates, concatenated
    mean, std = ic.compute(generator=torch.Generator().manual_seed(7))
    kept = logits if remove_class is None else logits[logits.argmax(-1) != remove_class]
    perm = torch.randperm(kept.shape[0], generator=torch.Generator().manual_seed(7))
    rm, rs, k = inception_score_f64(logits, splits, perm, remove_class)
    if n == 11:
        assert k == 6                                            # torch.chunk semantics: 6 chunks of 2, 2, 2, 2, 2, 1
    assert math.isclose(float(mean), rm, rel_tol=1e-6)
    if n == 1:
        assert math.isnan(float(std)) and math.isnan(rs)
    else:
        assert math.isclose(float(std), rs, rel_tol=1e-6)


# ---------------------------------------------------------------- 3. the T-shirt matcher
def test_tshirt_frequency_is_strict_below_the_threshold():
    from siss_amd.classifier import TShirtClassifier
    tshirt = torch.rand(1, 28, 28, generator=torch.Generator().manual_seed(0))
    d = torch.randn(1, 28, 28, generator=torch.Generator().manual_seed(1))
    d = d / d.norm()
    imgs = torch.stack([tshirt + d * r for r in (9.999, 10.001, 0.0, 10.0 * (1 - 1e-5), 30.0)])
    frac, matches = TShirtClassifier.get_tshirt_frequency(imgs, tshirt)
    assert matches.tolist() == [True, False, True, True, False]
    assert frac == pytest.approx(3 / 5)
    # exactly at the threshold: not a match
    _, m = TShirtClassifier.get_tshirt_frequency(torch.full((1, 1, 1, 100), 1.0), torch.zeros(1, 1, 100))
    assert m.tolist() == [False]                                 # distance sqrt(100) = 10: not < 10


# ---------------------------------------------------------------- 4. the tracker
def test_tracker_sets_deletion_steps_once_and_fires_the_score_there(tmp_path):
    from siss_amd.classifier import InceptionScore, TShirtMetrics
    tshirt = torch.zeros(1, 4, 4)
    far = torch.ones(1, 4, 4) * 5                                # distance 20 from the T-shirt
    shares = {0: 0.5, 2: 0.25, 4: 0.0, 6: 0.0}                   # the T-shirt share of the fraction samples at each evaluation
    calls = []

    def sample(n, bs):
        step = current[0]
        calls.append((step, n, bs))
        k = int(round(shares.get(step, 0.0) * n))
        return torch.stack([tshirt] * k + [far + 0.01 * i for i in range(n - k)])

    class C:
        def compute_logits(self, imgs):
            return torch.randn(imgs.shape[0], 10, generator=torch.Generator().manual_seed(imgs.shape[0]))

    path = str(tmp_path / "metrics_rank0.jsonl")
    tr = TShirtMetrics(tshirt, path, sample, sampling_steps=2, eval_images=8, eval_batch_size=4,
                       inception=lambda: InceptionScore(C(), splits=2), is_every=5, is_images=8, is_batch_size=8,
                       generator=torch.Generator().manual_seed(0))
    current = [0]
    for step in range(8):
        current[0] = step
        tr(step)
    lines = [json.loads(l) for l in open(path)]
    assert [r["global_step"] for r in lines] == [0, 2, 4, 5, 6]
    by = {r["global_step"]: r for r in lines}
    assert [by[s].get("deletion_class_fraction") for s in (0, 2, 4, 6)] == [0.5, 0.25, 0.0, 0.0]
    assert [s for s in by if "deletion_steps" in by[s]] == [4] and by[4]["deletion_steps"] == 4 and tr.deletion_steps == 4
    # the score: step 0 and 5 (multiples of is_every) and at deletion_steps = 4; not at 2 or 6
    assert sorted(s for s in by if "is_mean" in by[s]) == [0, 4, 5]
    assert "deletion_class_fraction" not in by[5]
    assert by[0]["is_images"] == 4 and by[4]["is_images"] == 8         # the T-shirt matches are left out of the score
    assert all(math.isfinite(by[s]["is_mean"]) for s in (0, 4, 5)) and all(r["seconds"] >= 0 for r in lines)
    assert calls[:2] == [(0, 8, 4), (0, 8, 8)]


def test_tracker_writes_null_for_a_score_over_no_kept_images(tmp_path):
    from siss_amd.classifier import InceptionScore, TShirtMetrics
    tshirt = torch.zeros(1, 2, 2)
    path = str(tmp_path / "m.jsonl")
    tr = TShirtMetrics(tshirt, path, lambda n, bs: torch.zeros(n, 1, 2, 2), sampling_steps=None,
                       inception=lambda: InceptionScore(None), is_every=1, is_images=3)
    tr(0)
    (r,) = [json.loads(l) for l in open(path)]
    assert r["is_mean"] is None and r["is_std"] is None and r["is_images"] == 0 and "deletion_class_fraction" not in r


# ---------------------------------------------------------------- 5. refusals before any step
def _cfg(tmp_path, extra):
    from siss_amd import hydra_lite as H
    return H.compose("delete_tshirt", os.path.join(ROOT, "config"), [f"output_dir={tmp_path}", *extra])


_IS = ["+metrics.inception_score.step_frequency=4", "+metrics.inception_score.num_imgs_to_generate=8",
       "+metrics.inception_score.class_cfg._target_=metrics.inception_score.InceptionScore"]


def _clf(ckpt):
    return ["+metrics.classifier_cfg._target_=metrics.classifier.Classifier",
            "+metrics.classifier_cfg.classifier._target_=hydra.utils.get_object",
            "+metrics.classifier_cfg.classifier.path=metrics.mnist_resnet.resnet18",
            f"+metrics.classifier_cfg.classifier_ckpt={ckpt}", "+metrics.classifier_cfg.classifier_args.num_classes=10",
            "+metrics.classifier_cfg.classifier_args.grayscale=true", "+metrics.classifier_cfg.transform=null"]


def test_metrics_that_cannot_run_are_refused_before_any_step(tmp_path):
    from siss_amd.tasks import DeleteTShirt
    with pytest.raises(ValueError, match="sampling_steps"):
        DeleteTShirt(_cfg(tmp_path, ["+metrics.fraction_deletion=true"])).check_metrics()
    with pytest.raises(ValueError, match="sampling_steps"):
        DeleteTShirt(_cfg(tmp_path, ["+metrics.fraction_deletion=true", "+sampling_steps=0"])).check_metrics()
    with pytest.raises(ValueError, match="classifier_cfg"):
        DeleteTShirt(_cfg(tmp_path, _IS)).check_metrics()
    with pytest.raises(FileNotFoundError, match="nope.pt"):
        DeleteTShirt(_cfg(tmp_path, _IS + _clf(tmp_path / "nope.pt"))).check_metrics()
    # ... and run() raises them before it builds anything (the first thing after check_supported)
    task = DeleteTShirt(_cfg(tmp_path, _IS))
    with pytest.raises(ValueError, match="classifier_cfg"):
        task.check_supported()
        task.check_metrics()
    # what can run passes: the repo's config (no metrics block) and a complete one
    DeleteTShirt(_cfg(tmp_path, [])).check_metrics()
    ck = tmp_path / "c.pt"
    torch.save({}, ck)
    DeleteTShirt(_cfg(tmp_path, ["+metrics.fraction_deletion=true", "+sampling_steps=5"] + _IS + _clf(ck))).check_metrics()


def test_configs_without_the_metrics_build_nothing(tmp_path):
    from siss_amd.tasks import DeleteCeleb, DeleteTShirt
    for name, cls in (("delete_tshirt", DeleteTShirt), ("delete_celeb", DeleteCeleb)):
        from siss_amd import hydra_lite as H
        cfg = H.compose(name, os.path.join(ROOT, "config"), [f"output_dir={tmp_path}"])
        cls(cfg).check_metrics()
        assert cls(cfg).deletion_metrics(None, None, torch.zeros(1, 28, 28), "cpu") is None
    # DeleteCeleb ignores the block (the classifier-argmax fraction of delete_celeb.py is not built)
    cfg = _cfg(tmp_path, ["+metrics.fraction_deletion=true"])
    assert DeleteCeleb(cfg).deletion_metrics(None, None, torch.zeros(1, 28, 28), "cpu") is None
