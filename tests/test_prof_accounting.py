"""siss_amd/prof.py against recorded launches: tests/golden/prof_accounting.json holds every distinct (launcher, arguments) of the
benchmark's CelebA-HQ 256 B = 16 bf16 step, its `sd15` step (both eager, side streams on, as bench.py --full records them) and an
f32-mode step at the `small` configuration (plain and fused schedule), with the fields lib.call() appended to lib.PROF for it
BEFORE the accounting read its arguments by name -- plus, for the launchers those steps do not reach, the launches of their kernel
tests and of the `small` engine with phase_launch / subpixel_queue off.  Arguments are data only: numbers as they were, "T" for
a tensor, {"ints": [...]} for an int array, {"job" | "byref" | "jobs": ...} for siss_tn_job's scalar fields."""
import ctypes
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prof_accounting.json")

# every launcher with a rule of its own in the accounting: the fixture must hold at least one launch of each
ACCOUNTED = """siss_gemm_nt siss_gemm_nt_qstats siss_gemm_nt_alpha_cols siss_gemm_nt_geglu_fwd siss_gemm_nt_geglu_bwd siss_gemm_nt_d2s
    siss_gemm_nt_d2s_bias siss_gemm_nt_d2s_phases siss_gemm_nt_mulsub siss_conv3x3_sc siss_conv3x3_dgrad_sc siss_gemm_tn siss_gemm_tn_bs
    siss_gemm_tn_grouped siss_gemm_tn_grouped_capped siss_gemm_tn_pair siss_attn1h_fwd siss_attn1h_bwd siss_flash_attn_fwd
    siss_flash_attn_bwd siss_flash_attn_fwd_merged siss_flash_attn_bwd_merged siss_groupnorm_fwd siss_groupnorm_fwd_ld
    siss_groupnorm_fwd_qs siss_groupnorm_bwd siss_groupnorm_bwd_ld siss_groupnorm_bwd_ld_s2d siss_recombine_clip_adamw
    siss_mixture_fwd siss_loss_bwd_seed""".split()


def _rebuild(arg, lib):
    if arg == "T":
        return object()                     # a tensor: the accounting may only ask whether it is None
    if isinstance(arg, dict):
        (kind, v), = arg.items()
        job = lambda f: lib.TNJob(**{k: (ctypes.c_int * 9)(*x) if isinstance(x, list) else x for k, x in f.items()})
        if kind == "ints":
            return lib.int_array(v)
        if kind == "jobs":
            return (lib.TNJob * len(v))(*map(job, v))
        return job(v) if kind == "job" else ctypes.byref(job(v))
    return arg


def test_accounting_returns_the_recorded_fields_exactly():
    from siss_amd import lib, prof
    records = json.load(open(GOLDEN))["records"]
    seen = {r[0] for r in records}
    assert len(ACCOUNTED) == 31 and set(ACCOUNTED) == set(prof._RULES)
    assert not set(ACCOUNTED) - seen, sorted(set(ACCOUNTED) - seen)
    assert any(n.endswith("_f32") for n in seen)            # the f32 forms stay unaccounted, as recorded
    for name, args, base, work, shape, symbol, nbytes in records:
        assert len(args) == len(lib.PARAMS[name]) - 1, name                           # everything but the stream
        got = prof.account(name, dict(zip(lib.PARAMS[name], [_rebuild(a, lib) for a in args])))
        assert got == (base, work, tuple(shape), symbol, nbytes), (name, args, got)   # == on the floats: products of integers in double
        assert type(got[1]) is float and (nbytes is None or type(got[4]) is float), (name, got)
