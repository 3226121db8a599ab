"""Worker for tests/test_hip_lora_dp.py, in the manner of tests/rccl_trainable_worker.py: ONE process, a world-size-1 `nccl` (= RCCL)
group, dp.FORCE_COLLECTIVES -- a LoRA step issues its exchange (ONE all-reduce of the adapters' [2, L] gradient pair, after the
projection) although one rank has nothing to exchange.  A sum over one rank is the identity: the adapters, the merged parameters and
the adapter gradients after two steps must be bitwise those of the same two steps without a group.

    python tests/rccl_lora_worker.py <repo root>

Prints one line `RCCL_LORA {json}`.
"""
import json
import os
import re
import socket
import sys

ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SISS_DP_FORCE_COLLECTIVES"] = "1"
os.environ["SISS_DP_EXCHANGE"] = "sharded"             # (refused for LoRA: the stepper must fall back to the all-reduce and say so)
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
from siss_amd.lora import LoRAState            # noqa: E402
from siss_amd.step import SISSStepper          # noqa: E402
from siss_amd.unet import UNetEngine           # noqa: E402

KW = dict(sample_size=16, in_channels=3, out_channels=3, block_out_channels=(64, 128),
          down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"),
          layers_per_block=1, attention_head_dim=None, norm_num_groups=32, norm_eps=1e-6,
          downsample_padding=0, flip_sin_to_cos=False, freq_shift=1)
CALLS = {"all_reduce": 0, "floats": 0}


def main():
    assert torch.cuda.is_available() and dp.FORCE_COLLECTIVES
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", device_id=dev)
    pg = dist.group.WORLD
    orig = dist.all_reduce

    def counted(*a, **k):
        CALLS["all_reduce"] += 1
        CALLS["floats"] += a[0].numel()
        return orig(*a, **k)
    dist.all_reduce = counted
    kw = dict(lr=1e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-2, scaling_norm=5.0, lambd=0.5, mixed_precision="bf16",
              train_batch_size=2)
    ac = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, 1000, dtype=torch.float32), 0)
    g = torch.Generator().manual_seed(5)
    batches = []
    for _ in range(2):
        x0 = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev)
        a0 = (torch.rand(1, 3, 16, 16, generator=g) * 2 - 1).repeat(2, 1, 1, 1).to(dev)
        noise = torch.randn(2, 3, 16, 16, generator=g).to(dev)
        batches.append((x0, a0, noise, torch.tensor([999, 300], device=dev), torch.tensor([0.9, 0.2], device=dev)))
    eng = UNetEngine(UNet2DConfig(**KW), dev)
    sd = eng.init_random(seed=4)
    names = [n for n in sd if re.search(r"attentions\.\d+\.to_(q|k|v|out\.0)\.weight", n)]
    out = {}
    res = []
    for group in (None, pg):
        eng = UNetEngine(UNet2DConfig(**KW), dev)
        eng.load_state_dict(sd)
        state = LoRAState(eng, names, 4, 8.0, seed=3)
        st = SISSStepper(eng, ac, process_group=group, lora=state, **kw)
        before, before_floats = CALLS["all_reduce"], CALLS["floats"]
        for b in batches:
            st.step(*b)
        torch.cuda.synchronize()
        res.append((state.p.clone(), eng.ps.flat.clone(), state.g.clone(), eng.ps.shadow.clone()))
        if group is not None:
            out.update(dp_on=st.dp_on, overlap=st.overlap, exchange=st.exchange, step_all_reduces=CALLS["all_reduce"] - before,
                       hook=eng.on_early_grads_final is not None, exchanged_floats=CALLS["floats"] - before_floats,
                       adapter_floats=state.L)
        else:
            assert CALLS["all_reduce"] == 0
    bw = lambda a, b: bool(torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int16),
                                       b.view(torch.int32 if b.element_size() == 4 else torch.int16)))
    (p0, f0, g0, s0), (p1, f1, g1, s1) = res
    out["bitwise_adapters"], out["bitwise_params"], out["bitwise_adapter_grads"], out["bitwise_shadow"] = bw(p0, p1), bw(f0, f1), bw(g0, g1), bw(s0, s1)
    eng0 = UNetEngine(UNet2DConfig(**KW), dev)
    eng0.load_state_dict(sd)
    out["moved"] = bool(not torch.equal(eng0.ps.flat, f1))
    out["collective_calls"] = dict(CALLS)
    out["ok"] = bool(out["dp_on"] and not out["hook"])
    print("RCCL_LORA " + json.dumps(out), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
