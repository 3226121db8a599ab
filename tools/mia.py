#!/usr/bin/env python
"""Membership inference attacks on a checkpoint, outside a run (siss_amd/mia.py: SecMI, PIA, loss threshold; csrc/mia.hip).  NOT the
reference's protocol.

    python tools/mia.py --config-name=delete_celeb|delete_tshirt --out FILE [key=value ...]

The evaluation `metrics.mia` runs inside the loop, once, at the weights the task's configuration loads (checkpoint_path=...): the
members drawn from the keep dataset, the forget images and the holdout images, every attack, one JSON record appended to FILE.
The overrides are the task's own; `+metrics.mia={...}` takes the fields of the key (step_frequency is not needed here).  Run it on
the pretrained and on the unlearned checkpoint with the same overrides to compare the two: the groups and the noises are seeded by
metrics.mia.seed alone.  Stable Diffusion has no latent-space form of the attacks and is refused.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TASKS = ("delete_celeb", "delete_tshirt")


def evaluate(config_name, config_path, overrides, out, device=None, global_step=0):
    """The record of one evaluation at the configured checkpoint, appended to `out`."""
    import torch
    from siss_amd import hydra_lite
    if config_name not in TASKS:
        raise ValueError(f"--config-name={config_name}: one of {TASKS} (no latent-space form of the attacks is built)")
    cfg = hydra_lite.compose(config_name, config_path, list(overrides))
    task = hydra_lite.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    task.fill_cfg()
    task.mia = task.check_mia(in_loop=False)                     # a bad key is refused before anything is loaded
    assert torch.cuda.is_available(), "mia.py needs a GPU: the attacks run on the HIP forward (there is no fall-back)"
    device = torch.device("cuda", 0) if device is None else device
    unet = task.load_unet(device)
    sched = task.load_scheduler()
    ds_all, ds_del = task.datasets((unet.config.in_channels, unet.config.sample_size, unet.config.sample_size))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    return task.mia_evaluation(unet, sched, ds_all, ds_del, device, out)(global_step)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config-name", required=True)
    ap.add_argument("--config-path", default=os.path.join(ROOT, "config"))
    ap.add_argument("--out", required=True, help="the JSON-lines file the record is appended to")
    ap.add_argument("--global-step", type=int, default=0, help="the global_step the record carries")
    a, overrides = ap.parse_known_args(argv)
    return evaluate(a.config_name, a.config_path, overrides, a.out, global_step=a.global_step)


if __name__ == "__main__":
    main()
