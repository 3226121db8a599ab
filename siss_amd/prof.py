"""What lib.call() books for a launch when lib.PROF is a list: the name a launcher is counted under, its ALGORITHMIC flops, its
problem shape, the device kernel it lands on and its ALGORITHMIC HBM bytes -- the figures behind bench.py --full's `roofline`,
`all_mfma_kernels`, `hbm_kernels` and `by_grid`, and tools/step_breakdown.py.

account(name, a) takes the launcher's name and its arguments keyed by the parameter names of include/siss_hip.h (lib.PARAMS); a
tensor argument is only ever asked whether it is None.  A launcher without a rule books no work, no shape and itself as the kernel.
"""


def _true_rows(M, rows_per_image, Hp, Wp):
    """The rows that count are the images' TRUE pixels (B * H * W), not the rows of the padded-NHWC layout the kernel walks
    (halo pixels are layout overhead, 3.3 % at 256 x 256, 13 % at 32 x 32)."""
    if Hp > 2 and Wp > 2 and M % rows_per_image == 0:
        return (M // rows_per_image) * (Hp - 2) * (Wp - 2)
    return M


def _triples(shifts, coffs, n):
    """Whether n filter taps come as row triples (shift, shift + 1, shift + 2) on one channel offset: the 3-tap kernels' condition."""
    return n % 3 == 0 and all(shifts[3 * g + 1] == shifts[3 * g] + 1 and shifts[3 * g + 2] == shifts[3 * g] + 2
                              and coffs[3 * g] == coffs[3 * g + 1] == coffs[3 * g + 2] for g in range(n // 3))


def _nt(a, N=None, npanels=1, batch=1, conv=False, planes=False):
    """One panelled NT product, 2 * M * N * Kp * npanels * batch, booked as siss_gemm_nt whichever epilogue the variant adds.
    conv: the launcher takes the image geometry and the tap table (the others are plain matrices); planes: the four phases of
    siss_gemm_nt_d2s_phases in one launch, which never takes the c3p kernel (mirrors the dispatch in gemm_nt.hip)."""
    M, N, Kp = a["M"], a["N"] if N is None else N, a["Kp"]
    rpi, Hp, Wp = (a["rows_per_image"], a["Hp"], a["Wp"]) if conv else (1, 0, 0)
    c3p = (conv and not planes and npanels == 9 and batch == 1 and Kp % 64 == 0 and N % 128 == 0 and rpi >= 256
           and -(-M // 128) * -(-N // 128) >= 256 and _triples(a["shifts"], a["coffs"], 9))
    key = ("M", M, "N", N, "K", Kp, "panels", npanels, "batch", batch) + (("4 planes",) if planes else ())
    return ("siss_gemm_nt", 2.0 * _true_rows(M, rpi, Hp, Wp) * N * Kp * npanels * batch, key,
            "gemm_nt_c3p_kernel" if c3p else "gemm_nt_kernel", None)


def _nt_shortcut(a, outer, inner, folded, tag):
    """A 3x3 product with a resnet's 1x1 shortcut folded in, 2 * M * outer * (9 inner + folded): always the c3p kernel."""
    rows = _true_rows(a["M"], a["rows_per_image"], a["Hp"], a["Wp"])
    key = ("M", a["M"], "N", a["N"], "K", a["Kp"], "panels", 9, tag, a[folded])
    return "siss_gemm_nt", 2.0 * rows * a[outer] * (9 * a[inner] + a[folded]), key, "gemm_nt_c3p_kernel", None


def _tn_flops(j):
    """2 * N * C * npanels * nsets * rows of one TN product (j: a siss_tn_job, or siss_gemm_tn's arguments under the same names)."""
    rows, rps, rb = j["row_end"] - j["row_begin"], j["rows_per_set"], j["row_begin"]
    wp = rb - 1                 # padded layouts reduce over rows [wp + 1, rows_per_set - (wp + 1)); images are square
    if wp > 2 and rps % (wp * wp) == 0 and rows == rps - 2 * rb:
        rows = (rps // (wp * wp)) * (wp - 2) * (wp - 2)
    return 2.0 * j["N"] * j["C"] * j["npanels"] * j["nsets"] * rows


def _job(j):
    return {f: getattr(j, f) for f in ("N", "C", "npanels", "nsets", "rows_per_set", "row_begin", "row_end")}


def _tn(a):
    rows = a["row_end"] - a["row_begin"]
    three = _triples(a["shifts"], a["coffs"], a["npanels"]) and (a["nsplits"] > 0 or rows >= 8192)
    key = ("N", a["N"], "C", a["C"], "panels", a["npanels"], "sets", a["nsets"], "rows", rows, "splits", a["nsplits"])
    return "siss_gemm_tn", _tn_flops(a), key, "gemm_tn_kernel<3>" if three else "gemm_tn_kernel<1>", None


def _tn_table(a, symbol):
    return None, sum(_tn_flops(_job(j)) for j in a["jobs"]), (), symbol, None


def _tn_pair(a):                # (byref(job3), byref(job1)): both products
    j3, j1 = _job(a["job3"]._obj), _job(a["job1"]._obj)
    key = ("N", j3["N"], "C", j3["C"], "panels", j3["npanels"], "+ N", j1["N"], "C", j1["C"], "panels", j1["npanels"],
           "rows", j3["row_end"] - j3["row_begin"])
    return None, _tn_flops(j3) + _tn_flops(j1), key, "gemm_tn_mixed_kernel", None


def _attn(products, heads, Sq, Sk, D, one_head=False):
    """Fused attention: forward QK^T and PV (2 products); backward S, dP, dQ, dK, dV (5: algorithmic -- the kernels recompute S
    and dP, 7 products run).  Padded queries / head dim count as laid out, keys as valid."""
    key = ("B", heads, "S", Sq, "D", D) if one_head else ("BH", heads, "Sq", Sq, "Sk", Sk, "D", D)
    return None, 2.0 * products * heads * Sq * Sk * D, key, None, None


def _gn_fwd(a, name="siss_groupnorm_fwd_ld"):          # read x + write y (bf16); the _qs form is booked as the _ld one
    return name, 0.0, ("n", a["N"], "H", a["H"], "C", a["C"]), name, 2.0 * 2 * a["N"] * a["H"] * a["W"] * a["C"]


def _gn_bwd(a, name="siss_groupnorm_bwd_ld"):          # read x (nx samples), read dy + write dx (n2 samples) (+ accum reads)
    passes = 2 + (a["accum"] is not None) + (a["accum2"] is not None)
    return (name, 0.0, ("n2", a["n2"], "H", a["H"], "C", a["C"]), name,
            2.0 * (a["H"] * a["W"] * a["C"]) * (a["nx"] + passes * a["n2"]))


def _gn_bwd_sc(a):
    """siss_groupnorm_bwd_sc: a GroupNorm backward whose apply pass is the epilogue of the shortcut's dgrad, 2 * M * C * K over the
    true pixels; bytes as _gn_bwd books them (every operand once): x (nx samples), dy, dx (+ the running cotangents) and dout."""
    px = a["H"] * a["W"]
    passes = 2 + (a["accum2"] is not None) + bool(a["accumulate2"] and a["dx2"] is not None)
    key = ("n2", a["n2"], "H", a["H"], "C", a["C"], "K", a["K"])
    return (None, 2.0 * a["n2"] * px * a["C"] * a["K"], key, "gn_bwd_sc_kernel",
            2.0 * px * (a["C"] * (a["nx"] + passes * a["n2"]) + a["K"] * a["n2"]))


def _hbm(nbytes):
    """An HBM-bound element-wise launcher (every operand read once, every result written once)."""
    return None, 0.0, (), None, nbytes


def _conv_nt(a):
    return _nt(a, npanels=a["npanels"], conv=True)


_RULES = {
    "siss_gemm_nt": lambda a: _nt(a, npanels=a["npanels"], batch=a["batch"], conv=True),
    "siss_gemm_nt_qstats": _conv_nt,
    "siss_gemm_nt_d2s": _conv_nt,
    "siss_gemm_nt_d2s_bias": _conv_nt,
    "siss_gemm_nt_d2s_phases": lambda a: _nt(a, npanels=a["phase_p0"][4], conv=True, planes=True),
    "siss_gemm_nt_alpha_cols": _nt,
    "siss_gemm_nt_geglu_bwd": _nt,
    "siss_gemm_nt_geglu_fwd": lambda a: _nt(a, N=2 * a["F"]),          # value and gate halves
    "siss_conv3x3_sc": lambda a: _nt_shortcut(a, "N", "Kp", "K2", "+1x1 K"),
    "siss_conv3x3_dgrad_sc": lambda a: _nt_shortcut(a, "Kp", "N", "Nx", "+1x1 N"),
    "siss_gemm_nt_mulsub": lambda a: (None, 2.0 * a["M"] * a["N"] * a["Kp"] * a["batch"], (), "gemm_nt_kernel", None),
    "siss_gemm_tn": _tn,
    "siss_gemm_tn_bs": _tn,
    "siss_gemm_tn_grouped": lambda a: _tn_table(a, "gemm_tn_grouped_kernel"),
    "siss_gemm_tn_grouped_capped": lambda a: _tn_table(a, "gemm_tn_grouped_capped_kernel"),
    "siss_gemm_tn_pair": _tn_pair,
    "siss_attn1h_fwd": lambda a: _attn(2, a["B"], a["S"], a["S"], a["D"], one_head=True),
    "siss_attn1h_bwd": lambda a: _attn(5, a["nb"], a["S"], a["S"], a["D"], one_head=True),
    "siss_flash_attn_fwd": lambda a: _attn(2, a["BH"], a["Sq_pad"], a["valid_k"], a["D_pad"]),
    "siss_flash_attn_bwd": lambda a: _attn(5, a["nBH"], a["Sq_pad"], a["valid_k"], a["D_pad"]),
    "siss_flash_attn_fwd_merged": lambda a: _attn(2, a["B"] * a["H"], a["Sq"], a["Sk"], a["D"]),
    "siss_flash_attn_bwd_merged": lambda a: _attn(5, a["nB"] * a["H"], a["Sq"], a["Sk"], a["D"]),
    "siss_groupnorm_fwd": lambda a: _gn_fwd(a, None),
    "siss_groupnorm_fwd_ld": _gn_fwd,
    "siss_groupnorm_fwd_qs": _gn_fwd,
    "siss_groupnorm_bwd": lambda a: _gn_bwd(a, None),
    "siss_groupnorm_bwd_ld": _gn_bwd,
    "siss_groupnorm_bwd_ld_s2d": _gn_bwd,
    "siss_recombine_clip_adamw": lambda a: _hbm(32.0 * a["n"]),     # read g_x, g_a, theta, m, v; write theta, m, v (f32)
    "siss_mixture_fwd": lambda a: _hbm(4.0 * (2 if a["in_bf16"] else 4) * a["B"] * a["chw"]),    # read x0, a0, noise; write x_mix
    "siss_loss_bwd_seed": lambda a: _hbm((4 + 3 * (2 if a["in_bf16"] else 4) + 8.0) * a["B"] * a["chw"]),   # read pred (f32), x_mix, x0, a0; write c_x, c_a (f32)
}


# Launchers that came after the recorded launches of tests/golden/prof_accounting.json (which holds one launch per rule of _RULES):
# their rules are held against hand-worked figures by the tests of the launcher itself.
_LATER_RULES = {
    "siss_groupnorm_bwd_sc": _gn_bwd_sc,
}


def account(name, a):
    """-> (base name, work, shape key, kernel symbol, hbm bytes) of one launch.  The base name folds the row-stride (`_ld`) and
    merged-layout (`_merged`) variants into their plain form, so that one launcher's launches add up under one name."""
    rule = _RULES.get(name) or _LATER_RULES.get(name)
    booked, work, key, symbol, nbytes = rule(a) if rule else (None, 0.0, (), None, None)
    base = booked or name               # (a rule names what it is booked as / lands on only where that is not the launcher itself)
    base = base[:-3] if base.endswith("_ld") else base
    return base[:-7] if base.endswith("_merged") else base, work, key, symbol or booked or name, nbytes
