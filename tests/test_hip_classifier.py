"""The MNIST ResNet-18 of the quality metrics on the GPU: logits against the f64 CPU restatement (folded BN with randomised
statistics, 28 x 28 / 32 x 32, one / three channels, 10 / 11 classes, batches that cross the 2048-image batch), determinism, the
class-frequency and Inception Score surfaces, and the T-shirt metrics in the task loop."""
import json
import math
import os

import pytest
import torch

import classifier_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-4            # max |d| <= BOUND * max |ref|


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from siss_amd import lib
    lib.load()
    return torch.device("cuda", 0)


def _classifier(tmp_path, net, num_classes, gray, sd=None, name="c.pt"):
    from siss_amd.classifier import Classifier, resnet18
    path = str(tmp_path / name)
    torch.save(net.state_dict() if sd is None else sd, path)
    return Classifier(resnet18, path, {"num_classes": num_classes, "grayscale": gray}, None, "cuda:0")


def _images(n, c, hw, seed=0):
    return torch.rand(n, c, hw, hw, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("n, hw, gray, classes", [(1, 28, True, 10), (7, 32, False, 11), (128, 28, True, 11), (128, 32, True, 10),
                                                   (7, 28, False, 10), (2500, 28, True, 10)])
def test_logits_against_the_f64_restatement(dev, tmp_path, n, hw, gray, classes):
    net = R.make(classes, gray, seed=n)
    clf = _classifier(tmp_path, net, classes, gray)
    x = _images(n, 1 if gray else 3, hw, seed=n)
    ref = R.logits_f64(net, x)
    got = clf.compute_logits(x.to(dev)).cpu().double()
    assert got.shape == (n, classes)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"\nN={n} {hw}x{hw} C={1 if gray else 3} classes={classes}: max|d| {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}")
    assert err <= BOUND * scale
    # argmax agrees wherever the reference's top-2 margin is clear of the error
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3 * scale
    assert torch.equal(got.argmax(1)[clear], ref.argmax(1)[clear])
    # negative control: the same weights with the BN statistics reset are far outside the bound
    ctl = _classifier(tmp_path, net, classes, gray, sd=R.reset_bn_stats(net.state_dict()), name="ctl.pt")
    assert float((ctl.compute_logits(x.to(dev)).cpu().double() - got).abs().max()) > 100 * BOUND * scale


def test_logits_are_bitwise_deterministic(dev, tmp_path):
    net = R.make(10, True, seed=5)
    clf = _classifier(tmp_path, net, 10, True)
    x = _images(300, 1, 28, seed=5).to(dev)
    a = clf.compute_logits(x)
    b = clf.compute_logits(x)
    assert torch.equal(a, b)
    # a batch of one takes other split-K counts: the same image, the same bits on every call
    assert torch.equal(clf.compute_logits(x[:1]), clf.compute_logits(x[:1]))


def test_class_frequency_matches_the_reference_argmax(dev, tmp_path):
    net = R.make(10, True, seed=11)
    clf = _classifier(tmp_path, net, 10, True)
    x = _images(400, 1, 28, seed=11)
    ref = R.logits_f64(net, x)
    scale = float(ref.abs().max())
    top2 = ref.topk(2, dim=1).values
    keep = (top2[:, 0] - top2[:, 1]) > BOUND * scale * 4        # every margin clear of the bound
    x, ref = x[keep], ref[keep]
    assert x.shape[0] >= 200
    cls = int(ref.argmax(1).mode().values)
    want = float((ref.argmax(1) == cls).double().mean())
    assert clf.compute_class_frequency(x.to(dev), cls) == want
    assert clf.compute_class_frequency(x.to(dev), (cls + 1) % 10) == float((ref.argmax(1) == (cls + 1) % 10).double().mean())


def test_inception_score_end_to_end_against_f64_logits(dev, tmp_path):
    from siss_amd.classifier import InceptionScore
    net = R.make(10, True, seed=3)
    clf = _classifier(tmp_path, net, 10, True)
    x = _images(1000, 1, 28, seed=3)
    ic = InceptionScore(clf, splits=10)
    ic.update(x.to(dev))
    mean, std = ic.compute(generator=torch.Generator().manual_seed(1))
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(1))
    rm, rs, k = R.inception_score_f64(R.logits_f64(net, x), 10, perm)
    print(f"\nIS {float(mean):.8f} +- {float(std):.8f}; f64 logits {rm:.8f} +- {rs:.8f}")
    assert k == 10 and abs(float(mean) - rm) <= 1e-4 and abs(float(std) - rs) <= 1e-4


# ---------------------------------------------------------------- the task loop
def _tshirt(tmp_path, name, extra):
    from siss_amd import hydra_lite as H
    cfg = H.compose("delete_tshirt", os.path.join(ROOT, "config"),
                    ["training_steps=4", "train_batch_size=2", "gradient_accumulation_steps=1", f"output_dir={tmp_path}/{name}",
                     "checkpoint_path=/nonexistent", "allow_random_init=true", "allow_synthetic=true", "save_final=false",
                     "mixed_precision=bf16", "+dataloader_num_workers=1", *extra])
    cfg.unet = dict(sample_size=28, in_channels=1, out_channels=1, block_out_channels=[64, 128],
                    down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"],
                    layers_per_block=1)
    task = H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    return task.run(), cfg


def test_delete_tshirt_logs_the_fraction_and_the_score_without_changing_the_training(dev, tmp_path):
    plain, cfg0 = _tshirt(tmp_path, "plain", [])
    want = plain.e.ps.flat.clone()
    assert not os.path.exists(os.path.join(cfg0.output_dir, "metrics_rank0.jsonl"))
    ckpt = tmp_path / "mnist.pt"
    torch.save(R.make(10, True, seed=0).state_dict(), ckpt)
    extra = ["+sampling_steps=2", "+eval_images=6", "+eval_batch_size=4", "+pipeline.num_inference_steps=3",
             "+metrics.fraction_deletion=true",
             "+metrics.classifier_cfg._target_=metrics.classifier.Classifier",
             "+metrics.classifier_cfg.classifier._target_=hydra.utils.get_object",
             "+metrics.classifier_cfg.classifier.path=metrics.mnist_resnet.resnet18",
             f"+metrics.classifier_cfg.classifier_ckpt={ckpt}", "+metrics.classifier_cfg.classifier_args.num_classes=10",
             "+metrics.classifier_cfg.classifier_args.grayscale=true", "+metrics.classifier_cfg.transform=null",
             "+metrics.inception_score.class_cfg._target_=metrics.inception_score.InceptionScore",
             "+metrics.inception_score.class_cfg.splits=2", "+metrics.inception_score.step_frequency=4",
             "+metrics.inception_score.num_imgs_to_generate=8", "+metrics.inception_score.batch_size=8"]
    st, cfg = _tshirt(tmp_path, "metrics", extra)
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "metrics_rank0.jsonl"))]
    by = {r["global_step"]: r for r in lines}
    assert sorted(by) == [0, 2, 4] and len(lines) == 3
    assert all(0 <= r["deletion_class_fraction"] <= 1 and r["seconds"] > 0 for r in lines)
    dsteps = [r["deletion_steps"] for r in lines if "deletion_steps" in r]
    first_zero = [s for s in (0, 2, 4) if by[s]["deletion_class_fraction"] == 0][:1]
    assert dsteps == first_zero
    assert sorted(s for s in by if "is_mean" in by[s]) == sorted({0, 4, *dsteps})
    for s in by:
        if "is_mean" in by[s]:
            r = by[s]
            assert 0 <= r["is_images"] <= 8
            assert r["is_mean"] is None or (1 - 1e-6 <= r["is_mean"] <= 10 + 1e-6)
            assert (r["is_images"] == 0) == (r["is_mean"] is None)
    # the metrics draw their own samples from their own generators: the trained weights are those of the plain run
    assert float((st.e.ps.flat - want).abs().max()) <= 1e-6
