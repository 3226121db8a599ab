"""The data-parallel exchange of a LoRA step on ONE rank with forced collectives (tests/rccl_lora_worker.py, a fresh child process):
two steps with the all-reduce of the adapter gradients on are bit-identical to the same two steps without a process group, the
exchange is one all-reduce of the [2, L] adapter gradient pair per step, and the overlapped / sharded exchanges are off."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_gradient_exchange_on_one_rank_equals_the_steps_without_a_group():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_lora_worker.py"), ROOT], capture_output=True, text=True,
                       timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("RCCL_LORA ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(line[-1][len("RCCL_LORA "):])
    assert out["ok"] and out["moved"], out
    assert out["bitwise_adapters"] and out["bitwise_params"] and out["bitwise_adapter_grads"] and out["bitwise_shadow"], out
    assert not out["overlap"] and out["exchange"] == "allreduce", out
    assert "lora: the sharded exchange" in r.stdout, r.stdout[-2000:]
    # ONE all-reduce of the adapters' gradient pair per step -- not of the weight gradients
    assert out["step_all_reduces"] == 2 and out["exchanged_floats"] == 2 * 2 * out["adapter_floats"], out
