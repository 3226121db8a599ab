"""Worker for tests/test_hip_surgery.py, in the manner of tests/rccl_ewc_worker.py: ONE process, a world-size-1 `nccl` (= RCCL) group,
dp.FORCE_COLLECTIVES -- a step with gradient surgery exchanges the whole gradient buffer like the full update (the overlapped tail
all-reduce stays on: the gram pass reads the summed buffer after it) although one rank has nothing to exchange; SISS_DP_EXCHANGE=sharded
is refused for it: the stepper falls back to the all-reduce and says so, once.  A sum over one rank is the identity: parameters,
moments, the scalar block and the per-tensor sums after two steps must equal, by value, those of the same two steps without a group.

    python tests/rccl_surgery_worker.py <repo root>

Prints one line `RCCL_SURGERY {json}`.
"""
import json
import os
import socket
import sys

ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SISS_DP_FORCE_COLLECTIVES"] = "1"
os.environ["SISS_DP_EXCHANGE"] = "sharded"             # (refused with surgery: the stepper must fall back to the all-reduce and say so)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
if "MASTER_PORT" not in os.environ:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(s.getsockname()[1])
os.environ["RANK"], os.environ["WORLD_SIZE"], os.environ["LOCAL_RANK"] = "0", "1", "0"

import torch                                   # noqa: E402
import torch.distributed as dist               # noqa: E402

from siss_amd import dp                        # noqa: E402
from siss_amd.config import UNet2DConfig       # noqa: E402
from siss_amd.step import SISSStepper          # noqa: E402
from siss_amd.surgery import Surgery           # noqa: E402
from siss_amd.unet import UNetEngine           # noqa: E402

KW = dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
          down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
          layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6,
          downsample_padding=0, flip_sin_to_cos=False, freq_shift=1)
CALLS = {"all_reduce": 0}


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
        before = CALLS["all_reduce"]
        st = SISSStepper(eng, ac, process_group=group, surgery=Surgery(eng, "mutual", "tensor"), **kw)
        for _ in range(2):
            st.step(x0, a0, noise, t, u)
        torch.cuda.synchronize()
        res.append((eng.ps.flat.clone(), st.opt.m.clone(), st.opt.v.clone(), st.opt.scalars.clone(), st.surgery.group_sums.clone()))
        if group is not None:
            out.update(dp_on=st.dp_on, overlap=st.overlap, exchange=st.exchange, all_reduces=CALLS["all_reduce"] - before,
                       conflicts=int(st.stats()["surgery_conflicts"]))
        else:
            assert CALLS["all_reduce"] == 0
    (p0, m0, v0, s0, g0), (p1, m1, v1, s1, g1) = res
    out["equal_params"] = bool(torch.equal(p0, p1))
    out["equal_moments"] = bool(torch.equal(m0, m1) and torch.equal(v0, v1))
    out["equal_block"] = bool(torch.equal(s0, s1))
    out["equal_sums"] = bool(torch.equal(g0, g1))
    print("RCCL_SURGERY " + json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
