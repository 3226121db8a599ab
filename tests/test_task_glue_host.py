"""Host-only tests of the glue between the task loops and what is measured around them: the scorer chain of the SD evaluation, the
metric hooks' schedule, the one-step-late log writer, the one resolver of the UNet's configuration and the JSON-lines helpers."""
import itertools
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the scorer chain
class _Scorer:
    def __init__(self, name, calls):
        self.name, self.calls = name, calls
        self.u8 = torch.tensor([ord(name[0])], dtype=torch.uint8)

    def score_decoded(self, img):
        self.calls.append((self.name, "decoded", img))
        return torch.tensor([float(len(self.name))]), self.u8

    def score_u8(self, u8):
        self.calls.append((self.name, "u8", u8))
        return torch.tensor([-float(len(self.name))])


ORDER = ("fraction", "sscd", "clip_iqa")
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(ORDER, n)]


@pytest.mark.parametrize("on", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_scorer_chain_one_fused_call_then_the_same_bytes(on):
    from siss_amd.metric_net import score_chain
    calls = []
    every = {name: _Scorer(name, calls) for name in ORDER}
    img = torch.zeros(1, 3, 2, 2)
    results, u8 = score_chain([every[name] for name in ORDER if name in on], img)
    first = every[on[0]]
    assert u8 is first.u8
    assert [(n, kind) for n, kind, _ in calls] == [(on[0], "decoded")] + [(n, "u8") for n in on[1:]]     # inactive ones: never touched
    assert calls[0][2] is img and all(arg is first.u8 for _, _, arg in calls[1:])                          # the very tensor object
    assert [float(r) for r in results] == [float(len(on[0]))] + [-float(len(n)) for n in on[1:]]           # results in the fixed order


def test_scorer_chain_looks_its_methods_up_at_the_call():
    from siss_amd.metric_net import score_chain
    calls = []
    a, b = _Scorer("fraction", calls), _Scorer("sscd", calls)
    chain = [a, b]                                       # built ...
    a.score_decoded = lambda img: (calls.append("replaced decoded"), (torch.ones(1), a.u8))[1]
    b.score_u8 = lambda u8: (calls.append("replaced u8"), torch.ones(1))[1]
    results, u8 = score_chain(chain, torch.zeros(1, 3, 2, 2))                 # ... and called after the replacement
    assert calls == ["replaced decoded", "replaced u8"] and u8 is a.u8 and len(results) == 2


def test_deletion_fraction_has_the_scorer_methods():
    from siss_amd.kmeans import DeletionFraction

    class Classifier:
        def from_decoded(self, img):
            return "u8", "labels", "dist"

        def predict(self, u8):
            return "rows", "labels of " + u8, "dist"

    f = DeletionFraction(Classifier(), "unused")
    assert f.score_decoded("img") == ("labels", "u8") and f.score_u8("u8") == "labels of u8"


# ---------------------------------------------------------------- the hook schedule
def test_hooks_run_at_step_0_and_at_their_multiples_in_list_order():
    from siss_amd.tasks import _run_hooks, _start_hooks
    calls = []
    hooks = _start_hooks(iter([(every, lambda step, every=every: calls.append((step, every))) for every in (1, 3, 5)] + [None]))
    assert [every for every, _ in hooks] == [1, 3, 5]
    assert calls == [(0, 1), (0, 3), (0, 5)]
    for step in range(1, 8):
        _run_hooks(hooks, step)
    assert calls[3:] == [(s, every) for s in range(1, 8) for every in (1, 3, 5) if s % every == 0]
    assert calls[3:] == [(1, 1), (2, 1), (3, 1), (3, 3), (4, 1), (5, 1), (5, 5), (6, 1), (6, 3), (7, 1)]


def test_a_stop_from_a_builder_ends_the_start_without_any_later_hook():
    from siss_amd.tasks import _start_hooks
    calls = []

    def built():                                         # as metric_hooks: a generator, the next hook is built when asked for
        yield 2, lambda step: calls.append(("first", step))
        calls.append("the curve")
        yield None, None                                 # membership_metric's plot_params return
        calls.append("built after the stop")
        yield 1, lambda step: calls.append(("later", step))

    assert _start_hooks(built()) is None
    assert calls == [("first", 0), "the curve"]


# ---------------------------------------------------------------- the lagged log
class _Handle:
    def __init__(self, name, fail=False):
        self.name, self.fail = name, fail

    def get(self):
        if self.fail:
            raise RuntimeError(f"no stats for {self.name}")
        return {"name": self.name}


def _lagged(path, said):
    from siss_amd.records import LaggedLog

    def record(handle, meta):
        return dict(handle.get(), step=meta)
    return LaggedLog(path, record, lambda rec, meta: said.append(meta))


def _lines(path):
    return [json.loads(l) for l in open(path)]


def test_lagged_log_writes_each_record_once_in_order(tmp_path):
    path, said = str(tmp_path / "log.jsonl"), []
    with _lagged(path, said) as log:
        log.push(_Handle("a"), 1)
        assert _lines(path) == []                        # one step late
        log.push(_Handle("b"), 2)
        assert _lines(path) == [{"name": "a", "step": 1}]
        log.push(_Handle("c"), 3)
        log.flush()
        log.flush()                                      # nothing is kept: nothing is written twice
    assert _lines(path) == [{"name": n, "step": k} for n, k in (("a", 1), ("b", 2), ("c", 3))] and said == [1, 2, 3]
    assert log.file.closed


def test_lagged_log_keeps_the_last_completed_step_when_the_loop_raises(tmp_path):
    path = str(tmp_path / "log.jsonl")
    with pytest.raises(KeyError, match="the loop's own"):
        with _lagged(path, []) as log:
            log.push(_Handle("a"), 1)
            log.push(_Handle("b"), 2)
            raise KeyError("the loop's own")
    assert _lines(path) == [{"name": "a", "step": 1}, {"name": "b", "step": 2}]


def test_a_failing_last_flush_does_not_mask_the_loops_exception(tmp_path):
    path = str(tmp_path / "log.jsonl")
    with pytest.raises(KeyError, match="the loop's own"):
        with _lagged(path, []) as log:
            log.push(_Handle("a"), 1)
            log.push(_Handle("b", fail=True), 2)
            raise KeyError("the loop's own")
    assert _lines(path) == [{"name": "a", "step": 1}] and log.file.closed


# ---------------------------------------------------------------- the UNet configuration
TINY = dict(sample_size=8, block_out_channels=[32, 64], layers_per_block=1, norm_num_groups=32)
PIXEL = dict(TINY, down_block_types=["DownBlock2D", "AttnDownBlock2D"], up_block_types=["AttnUpBlock2D", "UpBlock2D"])
COND = dict(TINY, down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"], up_block_types=["UpBlock2D", "CrossAttnUpBlock2D"],
            cross_attention_dim=32, attention_head_dim=4)
TASKS = {"DeleteCeleb": ("delete_celeb", PIXEL), "DeleteTShirt": ("delete_tshirt", PIXEL), "DeleteSD": ("delete_sd", COND),
         "TrainUnconditional": ("train_tshirt_mnist", PIXEL)}


def _task(cls, tmp_path, *overrides):
    from siss_amd import hydra_lite as H
    from siss_amd import tasks
    return getattr(tasks, cls)(H.compose(TASKS[cls][0], os.path.join(ROOT, "config"), [f"output_dir={tmp_path}/out", *overrides]))


def _agree(task, channels, sample_size):
    """unet_config(), the parameter specs and _image_channels() of one task say the same, and what they should."""
    import importlib
    cfg = task.unet_config()
    assert (cfg.in_channels, cfg.sample_size) == (channels, sample_size) and task._image_channels() == channels
    mod, name = task.unet_engine.rsplit(".", 1)
    specs = task.unet_param_specs()
    assert list(specs) == list(getattr(importlib.import_module(mod), name).param_specs(cfg)) == task.unet_param_names()
    assert tuple(specs["conv_in.weight"].ref_shape)[:2] == (cfg.block_out_channels[0], channels)


def _write(d, arch, channels):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(arch, in_channels=channels, out_channels=channels), f)


@pytest.mark.parametrize("cls", list(TASKS))
def test_unet_config_has_one_answer_per_source(cls, tmp_path):
    arch = TASKS[cls][1]
    in_cfg = [f"unet.{k}={json.dumps(v)}" for k, v in dict(arch, sample_size=16, in_channels=2, out_channels=2).items()]
    default = _task(cls, tmp_path).default_unet()
    # neither a checkpoint on disk nor cfg.unet: the task's default architecture
    _agree(_task(cls, tmp_path, f"checkpoint_path={tmp_path}/none", f"pretrained_model_name_or_path={tmp_path}/none"),
           default.in_channels, default.sample_size)
    # cfg.unet only (its _target_ and the like are not architecture)
    _agree(_task(cls, tmp_path, f"checkpoint_path={tmp_path}/none", f"pretrained_model_name_or_path={tmp_path}/none", *in_cfg,
                 "unet._target_=diffusers.UNet2DModel"), 2, 16)
    # a checkpoint on disk wins over cfg.unet: through subfolders.unet, and through the unet/ fall-back where that folder has no config
    _write(str(tmp_path / "a" / "unet_ema"), arch, 5)
    _write(str(tmp_path / "a" / "unet"), arch, 7)
    _write(str(tmp_path / "b" / "unet"), arch, 7)
    by_sub = _task(cls, tmp_path, f"checkpoint_path={tmp_path}/a", f"pretrained_model_name_or_path={tmp_path}/a",
                   "subfolders.unet=unet_ema", *in_cfg)
    fall_back = _task(cls, tmp_path, f"checkpoint_path={tmp_path}/b", f"pretrained_model_name_or_path={tmp_path}/b",
                      "subfolders.unet=unet_ema", *in_cfg)
    if cls == "TrainUnconditional":                      # its checkpoint_path is a training state to resume, never an architecture
        _agree(by_sub, 2, 16), _agree(fall_back, 2, 16)
        return
    if cls == "DeleteSD":                                # <pretrained_model_name_or_path>/unet, whatever subfolders says
        assert by_sub.unet_checkpoint() == f"{tmp_path}/a/unet"
        _agree(by_sub, 7, 8), _agree(fall_back, 7, 8)
        return
    assert by_sub.unet_checkpoint() == f"{tmp_path}/a/unet_ema" and fall_back.unet_checkpoint() == f"{tmp_path}/b/unet"
    _agree(by_sub, 5, 8), _agree(fall_back, 7, 8)


def test_fid_reads_the_channels_of_the_checkpoint_that_will_be_loaded(tmp_path):
    os.makedirs(tmp_path / "real")
    fid = ["+metrics.fid.class_cfg._target_=metrics.fid.FIDEvaluator", "+metrics.fid.class_cfg.allow_random_init=true",
           f"+metrics.fid.class_cfg.data_path={tmp_path}/real", "+metrics.fid.step_frequency=2", "+metrics.fid.num_imgs_to_generate=4",
           "+metrics.fid.batch_size=2"]
    _write(str(tmp_path / "one"), PIXEL, 1)
    _write(str(tmp_path / "three"), PIXEL, 3)
    with pytest.raises(ValueError, match="metrics.fid: the Inception-v3 takes 3-channel images, the UNet has in_channels=1"):
        _task("DeleteCeleb", tmp_path, f"checkpoint_path={tmp_path}/one", *fid).check_metrics()
    _task("DeleteCeleb", tmp_path, f"checkpoint_path={tmp_path}/three", *fid).check_metrics()
    assert not os.path.exists(tmp_path / "out")


# ---------------------------------------------------------------- the JSON-lines helpers
def test_finite_or_none_and_append_jsonl(tmp_path):
    from siss_amd.records import append_jsonl, finite_or_none
    assert finite_or_none(float("nan")) is None and finite_or_none(float("inf")) is None and finite_or_none(-float("inf")) is None
    assert finite_or_none(1.5) == 1.5 and finite_or_none(torch.tensor(2.0, dtype=torch.float64)) == 2.0
    path = str(tmp_path / "r.jsonl")
    recs = [{"global_step": 1, "b": None, "a": [1.5, None]}, {"global_step": 2, "text": "x"}]
    for rec in recs:
        assert append_jsonl(path, rec) is rec
    assert open(path).read().count("\n") == 2 and _lines(path) == recs
    assert [list(r) for r in _lines(path)] == [list(r) for r in recs]           # key order kept
