"""ctypes binding of libsiss_hip.so -- the C-ABI declared in include/siss_hip.h: binding, f32-mode routing and launch.

The argument types, parameter names and return types are READ from the header (which tools/gen_header.py generates from the
extern "C" blocks of csrc/*.hip), so adding an entry point is: write the launcher, run tools/gen_header.py.  What a launch is
booked as when PROF is on lives in siss_amd/prof.py.

The product path has NO CPU fallback: if the library is missing or a launcher returns a
non-zero status, a RuntimeError is raised.
"""
import ctypes as C
import os
import re
import threading

import torch

from . import prof

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SISS_LIB_PATH") or os.path.join(_HERE, "libsiss_hip.so")   # override: A/B two builds

P, I, L, D = C.c_void_p, C.c_int, C.c_long, C.c_double      # (the fields of the two structs below)
HEADER = os.path.join(os.path.dirname(_HERE), "include", "siss_hip.h")
_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double}


def parse_prototypes(text):
    """{entry point: (restype, [(ctype, parameter name), ...])} of every `int|long siss_*(...);` in a header's text.  Scalars map
    to their ctypes, `[const] int*` to POINTER(c_int) (host arrays handed over as int_array), every other pointer to c_void_p;
    a declaration that is none of these raises with the prototype's name -- there is no default type."""
    text = " ".join(re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split())
    out = {}
    for ret, name, params in re.findall(r"\b(int|long) (siss_\w+) ?\(([^()]*)\) ?;", text):
        out[name] = (_SCALARS[ret], [])
        for decl in ([] if params.strip() in ("", "void") else params.split(",")):
            m = re.fullmatch(r"(?:const )?(\w+)( ?\* ?| )(\w+)", decl.strip())
            if m and "*" in m.group(2):
                ctype = C.POINTER(C.c_int) if m.group(1) == "int" else C.c_void_p
            elif m and m.group(1) in _SCALARS:
                ctype = _SCALARS[m.group(1)]
            else:
                raise TypeError(f"{name}: no ctypes mapping for the parameter `{decl.strip()}`")
            out[name][1].append((ctype, m.group(3)))
    return out


_PROTOTYPES = parse_prototypes(open(HEADER).read())
SIGNATURES = {n: [t for t, _ in ps] for n, (_, ps) in _PROTOTYPES.items()}        # name -> argtypes (the stream included)
PARAMS = {n: tuple(p for _, p in ps) for n, (_, ps) in _PROTOTYPES.items()}       # name -> the header's parameter names
RESTYPE = {n: r for n, (r, _) in _PROTOTYPES.items()}                             # int status, or long for the *_words / count queries

# ---- the f32 parity mode (csrc/f32_path.hip): same argument lists as the bf16 entry points, f32 tensors.  F32_ENTRY maps a bf16
# entry point to its f32 form; F32_SAME lists the ones that never see an activation (f32 / index tensors only) and serve both
# modes.  In f32 mode (f32_mode(True): set by an f32 engine around its launches) call() takes the f32 form and REFUSES an entry
# point that has none -- a bf16 kernel handed f32 bytes would produce numbers, not an error.
F32_ENTRY = {n: n + "_f32" for n in (
    "siss_gemm_nt", "siss_gemm_tn", "siss_groupnorm_fwd_ld", "siss_groupnorm_bwd_ld", "siss_upsample2x", "siss_upsample2x_bwd",
    "siss_concat", "siss_concat_tail", "siss_concat_bwd", "siss_add_inplace", "siss_space_to_depth_ld", "siss_depth_to_space",
    "siss_pad_to_compact", "siss_compact_add_to_pad", "siss_im2col3x3", "siss_conv_out_fprop", "siss_mha_small_fwd",
    "siss_mha_small_bwd", "siss_softmax_fwd", "siss_softmax_bwd", "siss_softmax_rows_fwd", "siss_softmax_rows_bwd",
    "siss_layernorm_fwd", "siss_layernorm_bwd", "siss_geglu_fwd", "siss_geglu_bwd", "siss_head_split", "siss_head_merge",
    "siss_rowdot", "siss_gemm_nt_mulsub", "siss_conv_in_dgrad")}
F32_ENTRY.update({"siss_transpose_bf16": "siss_transpose_f32", "siss_cast_f32_bf16": "siss_copy_f32",
                  "siss_conv_weight_dgrad_multi_bf16": "siss_conv_weight_dgrad_multi_f32"})
# round 5: f32 forms of the engine's SCHEDULE SWITCHES (folded shortcut, depth-to-space epilogue, sub-pixel upsample, grouped wgrads),
# so that UNetEngine(dtype=float32, f32_fused=True) runs the fused schedule against the fp32 oracle
F32_ENTRY.update({n: n + "_f32" for n in ("siss_gemm_nt_d2s", "siss_gemm_nt_d2s_bias", "siss_gemm_nt_d2s_phases", "siss_conv3x3_sc", "siss_conv3x3_dgrad_sc",
                                          "siss_gemm_tn_bs", "siss_gemm_tn_grouped", "siss_groupnorm_bwd_ld_s2d",
                                          "siss_upsample_phase_weights")})
# (siss_quick_gelu_f32 is named by its caller, the f32 text tower of siss_amd/text_encoder.py: an f32-only kernel, listed with the rest)
F32_SAME = {"siss_zero_ranges", "siss_upsample_phase_wgrad_fold", "siss_timestep_sincos", "siss_linear_small_fwd", "siss_linear_small_bwd", "siss_linear_multi_fwd", "siss_linear_multi_bwd",
            "siss_nchw_channel_sums", "siss_mixture_fwd", "siss_mixture_select", "siss_loss_bwd_seed", "siss_mse_bwd_seed",
            "siss_ddpm_step", "siss_cfg_ddim_step", "siss_cfg_dpmpp_step", "siss_pflow_drift_div", "siss_slab_rowsum_f64", "siss_rk_combine", "siss_rk_norm", "siss_pair_noise", "siss_pair_sqerr", "siss_metric_conv", "siss_metric_maxpool3", "siss_inc_avgpool", "siss_inc_global_avg", "siss_inc_preprocess", "siss_fid_stats_update", "siss_kmeans_decoded", "siss_kmeans_finalize", "siss_kmeans_assign", "siss_kmeans_update", "siss_sscd_preprocess", "siss_sscd_gem", "siss_sscd_normalize_score", "siss_clipiqa_avgpool", "siss_clipiqa_token_mean", "siss_clipiqa_fold_query", "siss_clipiqa_scores", "siss_clipiqa_pool", "siss_clipiqa_head_value", "siss_clipiqa_score", "siss_quick_gelu_f32", "siss_grad_norms_scale", "siss_grad_norm_partials", "siss_grad_scalars", "siss_recombine_clip_adamw",
            "siss_grad_norms_scale_ranges", "siss_recombine_clip_adamw_ranges",
            "siss_grad_norm_single", "siss_clip_adamw_ema", "siss_ema_advance", "siss_ema_step", "siss_swap_f32",
            "siss_ctx_dgrad", "siss_ctx_reduce", "siss_noise_norm_cot", "siss_prompt_embed_update", "siss_latent_inject", "siss_latent_sample", "siss_image_gather",
            "siss_lora_project", "siss_lora_merge", "siss_lora_project_conv", "siss_lora_merge_conv",
            "siss_absf_select", "siss_saliency_mask", "siss_grad_norms_scale_masked", "siss_recombine_clip_adamw_masked",
            "siss_fisher_accumulate", "siss_grad_norms_scale_ewc",
            "siss_grad_norms_scale_surgery", "siss_recombine_clip_adamw_surgery",
            "siss_teacher_seed", "siss_grad_norms_weighted",
            "siss_ssd_ratio", "siss_ssd_dampen",
            "siss_uce_delta", "siss_uce_apply",
            "siss_sscd_topk", "siss_sscd_count_above", "siss_sscd_fill_above",
            "siss_feat_sqnorm", "siss_feat_knn_radius", "siss_feat_ball_stats", "siss_kid_sums",
            "siss_jl_project",
            "siss_mia_gather", "siss_mia_transfer", "siss_mia_transfer_sqerr", "siss_mia_powdiff"}
for _b, _f in F32_ENTRY.items():          # the header's promise "same argument lists", checked once instead of assumed
    if SIGNATURES[_b] != SIGNATURES[_f]:
        raise TypeError(f"{_f} does not have the argument types of {_b} in {HEADER}")
_MODE = threading.local()        # per thread: autograd runs an engine's backward on its own device thread (siss_amd/model.py)


def in_f32_mode():
    return bool(getattr(_MODE, "f32", False))


class f32_mode:
    """`with lib.f32_mode(engine.f32):` -- the launches of THIS thread inside the block go to the f32 entry points when the flag is set."""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        self.prev, _MODE.f32 = getattr(_MODE, "f32", False), self.on
        return self

    def __exit__(self, *exc):
        _MODE.f32 = self.prev
        return False


# siss_dispatch_count() ids (common.h SissKernelId): which device kernel a launcher call landed on
KERNEL_IDS = {"gemm_nt_kernel": 0, "gemm_nt_c3p_kernel": 1, "flash_attn_fwd": 2, "flash_attn_bwd": 3,
              "gemm_nt_kernel/splitk": 4, "gemm_tn_kernel<1>": 5, "gemm_tn_kernel<3>": 6, "gn_slab": 7, "gn_qstats": 8, "flash_dkdv_qsplit": 9,
              "attn1h_fwd": 10, "attn1h_bwd": 11, "gemm_tn_pair": 12, "flash32_bwd": 13, "flash32_fwd": 14, "gemm_nt_kernel/wide": 15,
              "gn_bwd_sc_kernel": 16}


def dispatch_counts(reset=False):
    """{kernel symbol: launches since the last reset} from the library's own dispatch counters."""
    lib = load()
    out = {k: int(lib.siss_dispatch_count(i)) for k, i in KERNEL_IDS.items()}
    if reset:
        lib.siss_dispatch_reset()
    return out



class TNJob(C.Structure):
    """siss_tn_job of include/siss_hip.h: one problem of siss_gemm_tn_grouped."""
    _fields_ = [("Y", P), ("ldy", L), ("X", P), ("ldx", L), ("dW", P), ("set_stride", L),
                ("N", I), ("C", I), ("npanels", I), ("nsets", I), ("rows_per_set", I), ("row_begin", I), ("row_end", I),
                ("nsplits", I), ("x_set_rows", L), ("zero_page", P), ("dbias", P), ("dbias2", P),
                ("shifts", I * 9), ("coffs", I * 9), ("bias_set_stride", L)]


class RkTerms(C.Structure):
    """siss_rk_terms of include/siss_hip.h: sum_j c[j] * row[j] over up to 8 f64 device rows (csrc/likelihood.hip)."""
    _fields_ = [("row", P * 8), ("c", D * 8), ("n", I)]

    @classmethod
    def of(cls, pairs):
        pairs = list(pairs)
        assert len(pairs) <= 8
        t = cls()
        for j, (c, r) in enumerate(pairs):
            assert r.dtype == torch.float64 and r.is_cuda and r.is_contiguous()
            t.row[j], t.c[j] = r.data_ptr(), float(c)
        t.n = len(pairs)
        return t


_lib = None
MIN_ABI = 5          # oldest build an A/B may load: round 5's final (siss_tn_job with bias_set_stride, attn1h / quad_stats / grouped_capped)


def load():
    """Load the HIP library; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -m siss_amd.build` "
            "(there is no CPU fallback for the SISS hot path)")
    lib = C.CDLL(LIB_PATH)
    override = os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libsiss_hip.so")
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)       # AttributeError if the symbol is missing
        except AttributeError:
            if override:                  # an OLDER build loaded for an A/B (bench.py --lib, tools/ab_bench.sh): newer entry points absent
                continue
            raise
        fn.argtypes = argtypes
        fn.restype = RESTYPE[name]
    _lib = lib
    if override and abi_version() < MIN_ABI:
        _lib = None
        raise RuntimeError(f"{LIB_PATH}: ABI version {abi_version()} < {MIN_ABI} (siss_tn_job layout / entry points the engines call "
                           "unconditionally): rebuild that tree, or A/B against a newer build")
    return lib


def has(name):
    """Whether the loaded library exports `name` (an older build loaded through SISS_LIB_PATH / bench.py --lib may lack newer entry
    points: callers switch the feature off instead of failing in the middle of a step)."""
    return hasattr(load(), name)


def abi_version():
    """siss_abi_version() of the loaded library (struct layouts + the entry points the engines call unconditionally); builds
    before round 6 have no such export and count as 5."""
    lib = load()
    return int(lib.siss_abi_version()) if hasattr(lib, "siss_abi_version") else 5


_WORKSPACE = {}
WORKSPACE_BYTES = 64 << 20      # split-K partial tiles of siss_gemm_nt (at most 32 MiB) / query-chunk partials of the attention dK, dV kernel


def ensure_workspace(device):
    """Hand the library its split-K scratch for `device` (one buffer per device, kept alive here; the C side never
    allocates and keeps one pointer PER DEVICE).  Launches on one stream at a time use it -- the one-compute-stream
    schedule of this package."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (device.type, index)
    if key not in _WORKSPACE:
        with torch.cuda.device(index):           # the library files the pointer under hipGetDevice()
            buf = torch.zeros(WORKSPACE_BYTES, dtype=torch.uint8, device=torch.device("cuda", index))    # zero-filled once: arrival counters
            rc = load().siss_gemm_nt_set_workspace(C.c_void_p(buf.data_ptr()), WORKSPACE_BYTES)
        if rc != 0:
            raise RuntimeError(f"siss_gemm_nt_set_workspace failed with status {rc}")
        _WORKSPACE[key] = buf
    return _WORKSPACE[key]


def ptr(t):
    """Device (or host) pointer of a tensor; None -> NULL."""
    if t is None:
        return None
    if torch.is_tensor(t):
        return C.c_void_p(t.data_ptr())
    return t


def int_array(xs):
    return (C.c_int * len(xs))(*xs)



def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-launch timing (bench.py, tools/step_breakdown.py): when PROF is a list, every call is bracketed by events on the
# launch stream and (base name, start, end, work, shape key, kernel symbol, hbm bytes) is appended -- the last four and the name
# folding from siss_amd/prof.py, which reads the arguments by the header's parameter names.
PROF = None


def call(name, *args, refusable=False):
    """Call a launcher on torch's current stream; tensors are passed as raw pointers.  refusable: status 1 (a shape the launcher
    does not take) is RETURNED instead of raised -- for entry points documented to refuse shapes the caller then runs another way."""
    lib = load()
    if getattr(_MODE, "f32", False):
        if name in F32_ENTRY:
            name = F32_ENTRY[name]
        elif name not in F32_SAME:
            raise RuntimeError(f"{name} has no f32 form: the f32 parity mode runs the engines with the fused bf16 kernels "
                               "switched off (csrc/f32_path.hip)")
    fn = getattr(lib, name)
    conv = [ptr(a) if (torch.is_tensor(a) or a is None) else
            (C.cast(a, C.c_void_p) if isinstance(a, C.Array) and a._type_ is not C.c_int else a) for a in args]   # job tables
    if PROF is None:
        rc = fn(*conv, stream_ptr())
    else:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = fn(*conv, stream_ptr())
        e.record()
        base, *fields = prof.account(name, dict(zip(PARAMS[name], args)))
        PROF.append((base, s, e, *fields))
    if rc == 1 and refusable:
        if PROF is not None:
            PROF.pop()                      # nothing ran
        return 1
    if rc != 0:
        raise RuntimeError(f"{name} failed with status {rc} "
                           f"({'bad argument' if rc == 1 else 'launch error'})")
    return 0


def query(name, *args):
    return getattr(load(), name)(*args)


def overwrite_log(max_records=8192):
    """Drain siss_gemm_tn_overwrite_log: [(address, floats), ...] of the weight-gradient products that overwrote their output since
    the last drain (host-side bookkeeping, no device work), or None when the log is unusable (it had filled up, or held more)."""
    buf = (C.c_long * (2 * max_records))()
    n = load().siss_gemm_tn_overwrite_log(C.cast(buf, C.c_void_p), max_records)
    if n < 0 or n > max_records:
        return None
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]
