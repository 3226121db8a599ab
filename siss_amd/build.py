"""Build libsiss_hip.so (all HIP kernels + the C-ABI) for gfx950 with hipcc, in-tree.

    python -m siss_amd.build          # incremental
    python -m siss_amd.build --force

hipcc cross-compiles without a GPU; the .so is git-ignored but travels with gpurun snapshots.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libsiss_hip.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# bit-exact-vs-torch kernels (q_sample, AdamW, the probability-flow drift, the membership metric's pair noising, the k-means
# classifier's uint8 image, the SSCD preprocessing, the prompt embedding's AdamW, the img2img starting latents, the
# latent cache's sampling launch, the image store's table gather, the single-set update with its EMA, the DPM-Solver++ step and its
# noise norms, the masked AdamW pair, the SSCD search's similarities, the Fisher accumulation and the anchor fold, the
# SSD ratio and dampening, the UCE increments and their add, the gradient surgery's sums, coefficients and update, the feature sets' distances and kernel sums, the teacher target's
# cotangent and the weighted pass 1, the DDIM transfers of the membership attacks) must not
# contract a*b+c into fma
EXACT = {"siss_loss.hip", "optimizer.hip", "train_state.hip", "likelihood.hip", "membership.hip", "kmeans.hip", "sscd.hip", "prompt_grad.hip",
         "injection.hip", "latent_cache.hip", "image_store.hip", "dpm_solver.hip", "saliency.hip", "sscd_search.hip", "ewc.hip", "ssd.hip",
         "surgery.hip", "feature_sets.hip", "teacher.hip", "mia.hip", "uce.hip"}
# per-file extras.  flash_attn.hip: MFMA results straight into VGPRs -- the softmax arithmetic consumes every accumulator of every
# tile, and with the default (AGPR destinations) each one cost a v_accvgpr_read in loops that are VALU-bound (832 -> 10 in the file);
# no SLP vectoriser: it pairs the softmax arithmetic into v_pk_*_f32 (526 in the file), which cost more issue slots beside MFMAs than
# the scalar forms (MI355X_MICROARCH issue-cost table) -- same IEEE results, 1.0-1.5 % faster on both kernels (same-box A/B x2)
_FA = ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize"]
EXTRA = {"flash_attn.hip": _FA, "flash_attn32.hip": _FA}


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _stale(dst, srcs):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    return any(os.path.getmtime(s) > t for s in srcs)


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.abspath(__file__)]   # (flags live here)
    jobs = []
    objs = []
    for f in sources():
        src = os.path.join(CSRC, f)
        obj = os.path.join(OBJ, f[:-4] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append(["hipcc", *FLAGS, *(["-ffp-contract=off"] if f in EXACT else []), *EXTRA.get(f, []), "-c", src, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))
        return cmd[-1]

    for f in os.listdir(OBJ):                                  # objects of sources that no longer exist (moved to tools/probes/)
        if f.endswith(".o") and os.path.join(OBJ, f) not in objs:
            os.remove(os.path.join(OBJ, f))
    if jobs:
        with ThreadPoolExecutor(max_workers=4) as ex:
            for done in ex.map(run, jobs):
                if verbose:
                    print("compiled", os.path.basename(done))
    if force or jobs or _stale(LIB, objs):
        run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB])
        if verbose:
            print("linked", LIB)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
