"""Worker for tests/test_hip_ssd.py, in the manner of tests/rccl_ewc_worker.py: ONE process, a world-size-1 `nccl` (= RCCL) group,
dp.FORCE_COLLECTIVES -- the importances of Selective Synaptic Dampening are this rank's own (no collective inside from_batches although
the data-parallel overlap hook is on for the steps), the dampening is local, and the step that follows exchanges its gradients as
always.  A sum over one rank is the identity: importances, dampened parameters, and parameters and moments after two steps must
equal, bit for bit, those of the same sequence without a group.

    python tests/rccl_ssd_worker.py <repo root>

Prints one line `RCCL_SSD {json}`.
"""
import json
import os
import socket
import sys

ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SISS_DP_FORCE_COLLECTIVES"] = "1"
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
if "MASTER_PORT" not in os.environ:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(s.getsockname()[1])
os.environ["RANK"], os.environ["WORLD_SIZE"], os.environ["LOCAL_RANK"] = "0", "1", "0"

import torch                                   # noqa: E402
import torch.distributed as dist               # noqa: E402

from siss_amd import dp, ssd                   # noqa: E402
from siss_amd.config import UNet2DConfig       # noqa: E402
from siss_amd.step import SISSStepper          # noqa: E402
from siss_amd.unet import UNetEngine           # noqa: E402

KW = dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
          down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
          layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6,
          downsample_padding=0, flip_sin_to_cos=False, freq_shift=1)
CALLS = {"all_reduce": 0}


def images(seed, repeat):
    g = torch.Generator().manual_seed(seed)
    one = torch.rand(1, 3, 16, 16, generator=g) * 2 - 1
    while True:
        yield one.clone() if repeat else torch.rand(1, 3, 16, 16, generator=g) * 2 - 1


def main():
    assert torch.cuda.is_available() and dp.FORCE_COLLECTIVES
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", device_id=dev)
    pg = dist.group.WORLD
    orig = dist.all_reduce

    def counted(*a, **k):
        CALLS["all_reduce"] += 1
        return orig(*a, **k)
    dist.all_reduce = counted
    kw = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2, scaling_norm=5.0, lambd=0.5, mixed_precision="bf16",
              train_batch_size=2)
    ac = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, 1000, dtype=torch.float32), 0)
    g = torch.Generator().manual_seed(5)
    x0 = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev)
    a0 = (torch.rand(1, 3, 16, 16, generator=g) * 2 - 1).repeat(2, 1, 1, 1).to(dev)
    noise = torch.randn(2, 3, 16, 16, generator=g).to(dev)
    t, u = torch.tensor([999, 300], device=dev), torch.tensor([0.9, 0.2], device=dev)
    sd = UNetEngine(UNet2DConfig(**KW), dev).init_random(seed=4)
    out, res = {}, []
    for group in (None, pg):
        eng = UNetEngine(UNet2DConfig(**KW), dev)
        eng.load_state_dict(sd)
        st = SISSStepper(eng, ac, process_group=group, **kw)
        before = CALLS["all_reduce"]
        imp = ssd.Importances.from_batches(st, images(9, False), images(21, True), 3, 2, generator=torch.Generator(device=dev).manual_seed(0),
                                           batch_size=1, seed=0)
        in_build = CALLS["all_reduce"] - before
        thr, strict, k, gt, ge = ssd.select(imp, fraction=0.05)
        stats = ssd.dampen(eng, imp, thr, strict, 1.0)
        dampened = eng.ps.flat.clone()
        for _ in range(2):
            st.step(x0, a0, noise, t, u)
        torch.cuda.synchronize()
        res.append((imp.keep.clone(), imp.forget.clone(), dampened, eng.ps.flat.clone(), st.opt.m.clone(), st.opt.v.clone()))
        if group is not None:
            out.update(dp_on=st.dp_on, overlap=st.overlap, exchange=st.exchange, all_reduces=CALLS["all_reduce"] - before,
                       all_reduces_in_from_batches=in_build, selected=stats["selected"], dampened=stats["dampened"])
        else:
            assert CALLS["all_reduce"] == 0
    a, b = res

    def eq(x, y):
        return bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
    out["equal_importances"] = eq(a[0], b[0]) and eq(a[1], b[1])
    out["equal_dampened"] = eq(a[2], b[2])
    out["equal_params"] = eq(a[3], b[3])
    out["equal_moments"] = eq(a[4], b[4]) and eq(a[5], b[5])
    print("RCCL_SSD " + json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
