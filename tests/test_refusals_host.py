"""What the launchers REFUSE (status 1, SISS_ERR_ARG), entry point by entry point, without a GPU.

Each entry point below has a `base` argument set that passes every argument check and a list of rows, each changing the base so that
exactly one SISS_CHECK_ARG of that entry point (or of the internal function it goes through: gemm_nt_dispatch, tn_setup, the GroupNorm
backward checks, the f32 instrument's validators) fails.  Every row must return 1; every base must NOT (it gets as far as the launch,
which fails with status 2 on a host without a device) -- which is what shows that a row's change is the only thing wrong with it.

The pointers are made-up 16-byte-aligned integers: nothing here may ever reach a launch on a real device, so the module skips where a
GPU is visible.  The table runs against any build (SISS_LIB_PATH): the refusals are part of the C ABI and do not move when the host
code behind it is reorganised.
"""
import ctypes as C

import pytest
import torch

from siss_amd import lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: host-only test")


def P(k):
    """Fake device pointer number k (16-byte aligned, 1 MiB apart)."""
    return 0x1000000 + (k << 20)


OFF8 = 8                    # + 8: breaks 16-byte alignment, keeps 8- and 4-byte alignment
Z1 = [0]
TAPS18 = [(ky - 1) * 18 + (kx - 1) for ky in range(3) for kx in range(3)]      # a 3x3 filter's panels on 18-pixel padded rows
INT_ARRAYS = ("shifts", "coffs", "phase_p0", "written")


def invoke(name, kw):
    args = []
    for ctype, pname in zip(lib.SIGNATURES[name], lib.PARAMS[name]):
        v = kw.get(pname)
        if pname in INT_ARRAYS and v is not None:
            v = lib.int_array(v)
        args.append(v)
    assert set(kw) <= set(lib.PARAMS[name]), (name, set(kw) - set(lib.PARAMS[name]))
    return getattr(lib.load(), name)(*args)


# ---------------------------------------------------------------------------------------------------------------- NT products
NT = dict(A=P(1), lda=64, W=P(2), C=P(3), ldc=128, bias=None, rowbias=None, ldrb=0, R=None, ldr=0, M=256, N=128, Kp=64, npanels=1,
          shifts=Z1, coffs=Z1, rows_per_image=256, Hp=0, Wp=0, alpha=1.0, batch=1, strideA=0, strideW=0, strideC=0)
NT_ROWS = [
    ("A null", dict(A=None)), ("W null", dict(W=None)), ("C null", dict(C=None)), ("shifts null", dict(shifts=None)),
    ("coffs null", dict(coffs=None)),
    ("M 0", dict(M=0)), ("N 0", dict(N=0)), ("Kp 0", dict(Kp=0)), ("Kp % 64", dict(Kp=96)), ("npanels 0", dict(npanels=0)),
    ("npanels 17", dict(npanels=17, shifts=[0] * 17, coffs=[0] * 17)),
    ("lda % 8", dict(lda=68)), ("ldc % 8", dict(ldc=132)), ("ldr % 8", dict(R=P(4), ldr=132)), ("batch 0", dict(batch=0)),
    ("A align", dict(A=P(1) + OFF8)), ("W align", dict(W=P(2) + OFF8)), ("C align", dict(C=P(3) + OFF8)),
    ("R align", dict(R=P(4) + OFF8, ldr=128)),
    ("strideA % 8", dict(strideA=4)), ("strideW % 8", dict(strideW=4)), ("strideC % 8", dict(strideC=4)),
    ("rows_per_image 0", dict(rows_per_image=0)), ("Hp Wp != rows_per_image", dict(Hp=4, Wp=4)),
    ("rowbias, image < 64 rows", dict(rowbias=P(5), ldrb=128, rows_per_image=32)),
    ("halo, image < 64 rows", dict(M=144, rows_per_image=36, Hp=6, Wp=6)),
    ("N % 8", dict(N=132, ldc=136)), ("ldrb % 4", dict(rowbias=P(5), ldrb=130)), ("bias align", dict(bias=P(6) + OFF8)),
    ("coff % 8", dict(coffs=[4])),
]
NT_KEYS = lambda *keys: {k: NT[k] for k in keys}
CORE = ("A", "lda", "W", "C", "ldc", "M", "N", "Kp")
PIX = dict(M=200, rows_per_image=100, Hp=10, Wp=10)                          # two 10 x 10 padded images

# persistent-3x3-kernel shapes: 102 images of 18 x 18 padded pixels = 259 row tiles of 128
C3 = dict(A=P(1), lda=64, W=P(2), C=P(3), ldc=128, M=102 * 324, N=128, Kp=64, shifts=TAPS18, coffs=[0] * 9, rows_per_image=324,
          Hp=18, Wp=18)
SC = dict(C3, bias=None, rowbias=None, ldrb=0, A2=P(7), lda2=64, W2=P(8), K2=64, bias2=None, qstats=None, written=None)
DSC = dict(C3, lda=128, Kp=128, R=None, ldr=0, Wx=P(7), Cx=P(8), ldcx=128, Nx=128)        # (the second product needs two K-groups)
BROKEN_TAPS = TAPS18[:1] + [TAPS18[1] + 1] + TAPS18[2:]

D2S = dict(NT_KEYS(*CORE, "R", "ldr", "npanels", "shifts", "coffs"), **PIX, plane=0)
D2SB = dict(NT_KEYS(*CORE, "bias", "npanels", "shifts", "coffs"), **PIX, plane=0)
PH = dict(NT_KEYS(*CORE, "bias", "R", "ldr"), **PIX, phase_p0=[0, 1, 2, 3, 4], shifts=[0] * 4, coffs=[0] * 4)
GEGLU_F = dict(A=P(1), lda=64, W=P(2), bias=None, h=P(3), y=P(4), M=256, F=64, Kp=64)
GEGLU_B = dict(A=P(1), lda=64, W=P(2), dh=P(3), h=P(4), rows_x=256, M=256, N=128, Kp=64)
MULSUB = dict(NT_KEYS(*CORE, "batch", "strideA", "strideW", "strideC"), R=P(4), ldr=128, rowsub=P(5), alpha=0.5)
ACOLS = dict(NT_KEYS(*CORE, "bias", "R", "ldr"), alpha=0.5, alpha_cols=64)
QS = dict({k: v for k, v in NT.items() if k not in ("batch", "strideA", "strideW", "strideC")}, qstats=P(9), written=[0])
D2S_ROWS = [("plane -1", dict(plane=-1)), ("plane 4", dict(plane=4)), ("Hp 2", dict(M=160, rows_per_image=80, Hp=2, Wp=40)),
            ("Wp 2", dict(M=160, rows_per_image=80, Hp=40, Wp=2)), ("Kp % 64", dict(Kp=96))]

# ---------------------------------------------------------------------------------------------------------------- f32 instrument
# (an entry point that is several launches -- the d2s phases, the folded shortcuts, the grouped walk -- stops at its first launch's
# error on a host without a device: only what is checked before that launch can be shown here)
NTF = dict(NT, lda=64)
NTF_ROWS = [
    ("A null", dict(A=None)), ("W null", dict(W=None)), ("C null", dict(C=None)), ("shifts null", dict(shifts=None)),
    ("coffs null", dict(coffs=None)), ("M 0", dict(M=0)), ("N 0", dict(N=0)), ("Kp 0", dict(Kp=0)), ("Kp % 16", dict(Kp=72)),
    ("npanels 0", dict(npanels=0)), ("npanels 17", dict(npanels=17, shifts=[0] * 17, coffs=[0] * 17)),
    ("batch 0", dict(batch=0)), ("batch 65536", dict(batch=65536)), ("rows_per_image 0", dict(rows_per_image=0)),
    ("lda % 4", dict(lda=66)), ("A align", dict(A=P(1) + OFF8)), ("W align", dict(W=P(2) + OFF8)),
    ("Hp Wp != rows_per_image", dict(Hp=4, Wp=4)), ("coff % 4", dict(coffs=[2])), ("N tiles > 65535", dict(N=64 * 65535 + 1)),
]
MULSUB_F_ROWS = [("R null", dict(R=None)), ("rowsub null", dict(rowsub=None)), ("A null", dict(A=None)), ("Kp % 16", dict(Kp=72)),
                 ("batch 0", dict(batch=0)), ("batch 65536", dict(batch=65536)), ("lda % 4", dict(lda=66)),
                 ("W align", dict(W=P(2) + OFF8)), ("N tiles > 65535", dict(N=64 * 65535 + 1))]
D2S_F_ROWS = D2S_ROWS[:4] + [("Kp % 16", dict(Kp=72)), ("npanels 17", dict(npanels=17, shifts=[0] * 17, coffs=[0] * 17)),
                             ("coff % 4", dict(coffs=[2]))]

# ---------------------------------------------------------------------------------------------------------------- weight gradients
TN = dict(Y=P(1), ldy=128, X=P(2), ldx=64, dW=P(3), set_stride=128 * 64, N=128, C=64, npanels=1, shifts=Z1, coffs=Z1, nsets=1,
          rows_per_set=256, x_set_rows=256, row_begin=0, row_end=256, nsplits=1, zero_page=P(4), dbias=None, dbias2=None)
TN_COMMON = [
    ("Y null", dict(Y=None)), ("X null", dict(X=None)), ("dW null", dict(dW=None)), ("shifts null", dict(shifts=None)),
    ("coffs null", dict(coffs=None)), ("N 0", dict(N=0)), ("C 0", dict(C=0)), ("npanels 0", dict(npanels=0)), ("nsets 0", dict(nsets=0)),
    ("row_begin < 0", dict(row_begin=-1)), ("row_end <= row_begin", dict(row_end=0)), ("row_end > rows_per_set", dict(row_end=257)),
]
TN_ROWS = TN_COMMON + [
    ("zero_page null", dict(zero_page=None)), ("npanels 10", dict(npanels=10, shifts=[0] * 10, coffs=[0] * 10)),
    ("ldy % 8", dict(ldy=132)), ("ldx % 8", dict(ldx=68)), ("C % 8", dict(C=60)),
    ("Y align", dict(Y=P(1) + OFF8)), ("X align", dict(X=P(2) + OFF8)), ("zero_page align", dict(zero_page=P(4) + OFF8)),
    ("dW align", dict(dW=P(3) + 2)), ("coff % 8", dict(coffs=[4])),
]
TNF_ROWS = TN_COMMON + [("npanels 17", dict(npanels=17, shifts=[0] * 17, coffs=[0] * 17)), ("panels x sets > 65535", dict(nsets=65536))]


def tn_job(**over):
    kw = dict(TN, **over)
    j = lib.TNJob()
    for k in ("ldy", "ldx", "set_stride", "N", "C", "npanels", "nsets", "rows_per_set", "row_begin", "row_end", "nsplits", "x_set_rows"):
        setattr(j, k, kw[k])
    for k in ("Y", "X", "dW", "zero_page", "dbias", "dbias2"):
        setattr(j, k, kw[k])
    for i in range(min(kw["npanels"], 9)):
        j.shifts[i], j.coffs[i] = (kw["shifts"] + [0] * 9)[i], (kw["coffs"] + [0] * 9)[i]
    j.bias_set_stride = kw.get("bias_set_stride", 0)
    return j


def job_table(*jobs):
    t = (lib.TNJob * len(jobs))(*jobs)
    return C.cast(t, C.c_void_p)


JOB3 = dict(npanels=3, shifts=[0, 1, 2], coffs=[0, 0, 0], dW=P(5))
JOB_ROWS = [("Y null", dict(Y=None)), ("zero_page null", dict(zero_page=None)), ("N 0", dict(N=0)), ("npanels 10", dict(npanels=10)),
            ("ldy % 8", dict(ldy=132)), ("C % 8", dict(C=60)), ("dW align", dict(dW=P(3) + 2)), ("row_end > rows_per_set", dict(row_end=257)),
            ("coff % 8", dict(coffs=[4]))]

# ---------------------------------------------------------------------------------------------------------------- GroupNorm backward
GN = dict(dy=P(1), x=P(2), gamma=P(3), beta=P(4), mean=P(5), rstd=P(6), dx=P(7), accum=None, accum2=None, dx2=None, split_c=0,
          accumulate2=0, dgamma=P(8), dbeta=P(9), colsum=None, colsum_ld=0, partial=P(10), n2=2, nx=1, set_images=1, set_stride=64,
          H=8, W=8, C=64, G=32, silu=1, dy_compact=0, ldx=0)
GN_SPLIT = dict(dx2=P(11), split_c=32)
GN_SHARED = [                                                       # the checks every backward entry point makes
    *[(f"{k} null", {k: None}) for k in ("dy", "x", "gamma", "beta", "mean", "rstd", "dx", "dgamma", "dbeta", "partial")],
    ("n2, nx 0", dict(n2=0, nx=0)), ("set_images 0", dict(set_images=0)), ("n2 % set_images", dict(set_images=3)),
    ("n2 = 3 nx", dict(n2=3)),
    ("C % 8", dict(C=60, G=30)), ("G > 32", dict(G=64)), ("C % G", dict(G=24)), ("H 0", dict(H=0)),
    ("dy align", dict(dy=P(1) + OFF8)), ("x align", dict(x=P(2) + OFF8)), ("dx align", dict(dx=P(7) + OFF8)),
    ("accum2 align", dict(accum2=P(12) + OFF8)), ("dx2 align", dict(dx2=P(11) + OFF8, split_c=32)),
    ("split_c 0", dict(dx2=P(11), split_c=0)), ("split_c = C", dict(dx2=P(11), split_c=64)), ("split_c % 8", dict(dx2=P(11), split_c=36)),
    ("ldx < C", dict(ldx=32)), ("ldx % 8", dict(ldx=68)), ("partial align", dict(partial=P(10) + OFF8)),
]
GN_ROWS = GN_SHARED + [("accum align", dict(accum=P(12) + OFF8))]
GN_S2D_ROWS = [("dx2 null", dict(dx2=None, split_c=0)), ("H odd", dict(H=7)), ("W odd", dict(W=7))]
GNF_ROWS = [
    *[(f"{k} null", {k: None}) for k in ("dy", "x", "gamma", "beta", "mean", "rstd", "dx", "dgamma", "dbeta")],
    ("n2, nx 0", dict(n2=0, nx=0)), ("set_images 0", dict(set_images=0)), ("n2 % set_images", dict(set_images=3)),
    ("n2 % nx", dict(n2=3, nx=2)), ("C % G", dict(G=24)), ("nx > 65535", dict(n2=65536, nx=65536)),
    ("split_c 0", dict(dx2=P(11), split_c=0)), ("split_c = C", dict(dx2=P(11), split_c=64)), ("ldx < C", dict(ldx=32)),
]
GNSC = dict({k: v for k, v in GN.items() if k not in ("accum", "colsum_ld", "dy_compact")}, dout=P(13), ldo=64, wsc=P(14), K=64,
            gconst=P(15), s2d=0)
GNSC_ROWS = [r for r in GN_SHARED if r[0] != "H 0"] + [
    ("colsum given", dict(colsum=P(12))), ("dout null", dict(dout=None)), ("wsc null", dict(wsc=None)), ("gconst null", dict(gconst=None)),
    ("s2d without dx2", dict(s2d=1)), ("s2d, H odd", dict(s2d=1, H=9, **GN_SPLIT)), ("s2d, W odd", dict(s2d=1, W=9, **GN_SPLIT)),
    ("K 0", dict(K=0)), ("K % 64", dict(K=96, ldo=96)), ("ldo < K", dict(ldo=32)), ("ldo % 8", dict(ldo=68)),
    ("two channel slices", dict(C=2048)),
    ("dout align", dict(dout=P(13) + OFF8)), ("wsc align", dict(wsc=P(14) + OFF8)), ("gconst align", dict(gconst=P(15) + OFF8)),
    ("image < 64 rows", dict(H=4, W=4)), ("set rows >= 2^31", dict(H=6, W=6, n2=1 << 25, nx=1 << 25, set_images=1 << 25)),
]

# ---------------------------------------------------------------------------------------------------------------- flash attention
FAF = dict(q=P(1), ldq=320, k=P(2), ldk=320, v=P(3), ldv=320, o=P(4), ldo=320, lse2=P(5), B=2, H=8, Sq=256, Sk=77, D=40, scale=0.158,
           q_prescaled=0)
FAB = dict(FAF, d_o=P(6), lddo=320, delta=P(7), dq=P(8), lddq=320, dk=P(9), lddk=320, dv=P(10), lddv=320, nB=4)
FA_ROWS = [("q null", dict(q=None)), ("lse2 null", dict(lse2=None)), ("B 0", dict(B=0)), ("H 0", dict(H=0)), ("Sq 0", dict(Sq=0)),
           ("Sk 0", dict(Sk=0)), ("D % 8", dict(D=36)), ("D > 192", dict(D=200, ldq=1600, ldk=1600, ldv=1600, ldo=1600)),
           ("ldq % 8", dict(ldq=324)), ("ldk < H D", dict(ldk=312)), ("v align", dict(v=P(3) + OFF8)), ("o align", dict(o=P(4) + OFF8))]
FAB_ROWS = [r for r in FA_ROWS if r[0] not in ("B 0", "D > 192")] + [
    ("d_o null", dict(d_o=None)), ("delta null", dict(delta=None)), ("dv null", dict(dv=None)), ("nB < B", dict(nB=1)),
    ("nB % B", dict(nB=3)), ("lddk % 8", dict(lddk=324)), ("lddq < H D", dict(lddq=312)), ("dq align", dict(dq=P(8) + OFF8)),
    ("lse2 align", dict(lse2=P(5) + OFF8)), ("delta align", dict(delta=P(7) + OFF8))]
FAP = dict(q=P(1), k=P(2), v=P(3), o=P(4), lse2=P(5), BH=4, Sq_pad=128, Sk_pad=128, D_pad=64, valid_k=77, scale=0.125)
FAPB = dict({k: v for k, v in FAP.items() if k != "o"}, d_o=P(6), delta=P(7), dq=P(8), dk=P(9), dv=P(10), nBH=8)
FAP_ROWS = [("k null", dict(k=None)), ("BH 0", dict(BH=0)), ("Sq_pad % 64", dict(Sq_pad=96)), ("D_pad 96", dict(D_pad=96)),
            ("valid_k 0", dict(valid_k=0)), ("valid_k > Sk_pad", dict(valid_k=129)), ("q align", dict(q=P(1) + OFF8))]

TABLE = {
    "siss_gemm_nt": (NT, NT_ROWS),
    "siss_gemm_nt_qstats": (QS, [("qstats null", dict(qstats=None)), ("written null", dict(written=None)), ("Kp % 64", dict(Kp=96)),
                                 ("ldrb % 4", dict(rowbias=P(5), ldrb=130))]),
    "siss_gemm_nt_alpha_cols": (ACOLS, [("alpha_cols < 0", dict(alpha_cols=-4)), ("alpha_cols % 4", dict(alpha_cols=6)),
                                        ("ldr % 8", dict(R=P(4), ldr=132)), ("bias align", dict(bias=P(6) + OFF8))]),
    "siss_gemm_nt_mulsub": (MULSUB, [("R null", dict(R=None)), ("rowsub null", dict(rowsub=None)), ("strideC % 8", dict(strideC=4)),
                                     ("batch 0", dict(batch=0)), ("R align", dict(R=P(4) + OFF8))]),
    "siss_gemm_nt_geglu_fwd": (GEGLU_F, [("y null", dict(y=None)), ("F 0", dict(F=0)), ("F % 64", dict(F=96)), ("y align", dict(y=P(4) + OFF8)),
                                         ("h align", dict(h=P(3) + OFF8)), ("Kp % 64", dict(Kp=96))]),
    "siss_gemm_nt_geglu_bwd": (GEGLU_B, [("h null", dict(h=None)), ("rows_x 0", dict(rows_x=0)), ("h align", dict(h=P(4) + OFF8)),
                                         ("lda % 8", dict(lda=68)), ("M 0", dict(M=0))]),
    "siss_gemm_nt_d2s": (D2S, D2S_ROWS + [("ldr % 8", dict(R=P(4), ldr=132))]),
    "siss_gemm_nt_d2s_bias": (D2SB, D2S_ROWS + [("bias align", dict(bias=P(6) + OFF8))]),
    "siss_gemm_nt_d2s_phases": (PH, [("phase_p0 null", dict(phase_p0=None)), ("fewer than 4 panels", dict(phase_p0=[0, 1, 2, 3, 3])),
                                     ("more than 16 panels", dict(phase_p0=[0, 1, 2, 3, 17], shifts=[0] * 17, coffs=[0] * 17)),
                                     ("phase_p0[0] != 0", dict(phase_p0=[1, 2, 3, 4, 5], shifts=[0] * 5, coffs=[0] * 5)),
                                     ("an empty plane", dict(phase_p0=[0, 2, 2, 3, 4])), ("Hp 2", dict(M=160, rows_per_image=80, Hp=2, Wp=40)),
                                     ("shifts null", dict(shifts=None))]),
    "siss_conv3x3_sc": (SC, [("A2 null", dict(A2=None)), ("W2 null", dict(W2=None)), ("shifts null", dict(shifts=None)),
                             ("not a 3x3 filter's panels", dict(shifts=BROKEN_TAPS)), ("K2 0", dict(K2=0)), ("K2 % 64", dict(K2=96, lda2=96)),
                             ("image < 256 rows", dict(M=330 * 100, rows_per_image=100, Hp=10, Wp=10)), ("N % 128", dict(N=64)),
                             ("lda2 % 8", dict(lda2=68)), ("lda2 < K2", dict(lda2=32)), ("A2 align", dict(A2=P(7) + OFF8)),
                             ("W2 align", dict(W2=P(8) + OFF8)), ("bias2 align", dict(bias2=P(6) + OFF8)), ("lda % 8", dict(lda=68))]),
    "siss_conv3x3_dgrad_sc": (DSC, [("Wx null", dict(Wx=None)), ("Cx null", dict(Cx=None)), ("coffs null", dict(coffs=None)),
                                    ("not a 3x3 filter's panels", dict(shifts=BROKEN_TAPS)), ("Nx 0", dict(Nx=0)), ("Nx % 128", dict(Nx=64)),
                                    ("ldcx 0", dict(ldcx=0)), ("ldcx % 8", dict(ldcx=132)), ("ldcx < Nx", dict(ldcx=64)),
                                    ("Wx align", dict(Wx=P(7) + OFF8)), ("Cx align", dict(Cx=P(8) + OFF8)), ("ldr % 8", dict(R=P(4), ldr=132))]),
    "siss_gemm_nt_f32": (NTF, NTF_ROWS),
    "siss_gemm_nt_mulsub_f32": (MULSUB, MULSUB_F_ROWS),
    "siss_gemm_nt_d2s_f32": (D2S, D2S_F_ROWS),
    "siss_gemm_nt_d2s_bias_f32": (D2SB, D2S_F_ROWS),
    "siss_gemm_nt_d2s_phases_f32": (PH, [("phase_p0 null", dict(phase_p0=None)), ("phase_p0[0] != 0", dict(phase_p0=[1, 2, 3, 4, 5])),
                                         ("shifts null", dict(shifts=None)), ("coffs null", dict(coffs=None)), ("W null", dict(W=None)),
                                         ("Hp 2", dict(M=160, rows_per_image=80, Hp=2, Wp=40)), ("an empty plane", dict(phase_p0=[0, 0, 2, 3, 4])),
                                         ("Kp % 16", dict(Kp=72))]),
    "siss_conv3x3_sc_f32": (SC, [("A2 null", dict(A2=None)), ("W2 null", dict(W2=None)), ("K2 0", dict(K2=0)), ("K2 % 16", dict(K2=72)),
                                 ("lda2 % 4", dict(lda2=66)), ("A2 align", dict(A2=P(7) + OFF8)), ("Hp Wp != rows_per_image", dict(Hp=17))]),
    "siss_conv3x3_dgrad_sc_f32": (DSC, [("Wx null", dict(Wx=None)), ("Cx null", dict(Cx=None)), ("Nx 0", dict(Nx=0)),
                                        ("coffs null", dict(coffs=None)), ("Kp % 16", dict(Kp=72))]),
    "siss_gemm_tn": (TN, TN_ROWS),
    "siss_gemm_tn_bs": (dict(TN, bias_set_stride=256), TN_ROWS),
    "siss_gemm_tn_f32": (TN, TNF_ROWS),
    "siss_gemm_tn_bs_f32": (dict(TN, bias_set_stride=256), TNF_ROWS),
    "siss_groupnorm_bwd_ld": (GN, GN_ROWS),
    "siss_groupnorm_bwd": ({k: v for k, v in GN.items() if k != "ldx"}, [r for r in GN_ROWS if not r[0].startswith("ldx")]),
    "siss_groupnorm_bwd_ld_s2d": (dict(GN, **GN_SPLIT), GN_S2D_ROWS + [r for r in GN_ROWS if "split_c" not in r[0] and "dx2" not in r[0]]),
    "siss_groupnorm_bwd_sc": (GNSC, GNSC_ROWS),
    "siss_groupnorm_bwd_ld_f32": (GN, GNF_ROWS),
    "siss_groupnorm_bwd_ld_s2d_f32": (dict(GN, **GN_SPLIT), GN_S2D_ROWS + [r for r in GNF_ROWS if "split_c" not in r[0]] +
                                      [("split_c = C", dict(split_c=64))]),
    "siss_flash_attn_fwd_merged": (FAF, FA_ROWS),
    "siss_flash_attn_bwd_merged": (FAB, FAB_ROWS),
    "siss_flash_attn_fwd": (FAP, FAP_ROWS + [("o null", dict(o=None))]),
    "siss_flash_attn_bwd": (FAPB, FAP_ROWS + [("delta null", dict(delta=None)), ("nBH < BH", dict(nBH=2)), ("nBH % BH", dict(nBH=6)),
                                              ("dk align", dict(dk=P(9) + OFF8)), ("delta align", dict(delta=P(7) + OFF8))]),
}
ROWS = [(name, label, over) for name, (_, rows) in TABLE.items() for label, over in rows]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_base_arguments_pass_every_check(name):
    assert invoke(name, TABLE[name][0]) != 1


@pytest.mark.parametrize("name,label,over", ROWS, ids=[f"{n}-{l}" for n, l, _ in ROWS])
def test_one_broken_argument_is_refused(name, label, over):
    assert invoke(name, dict(TABLE[name][0], **over)) == 1


# ---- job tables: siss_gemm_tn_grouped / _capped / _pair and the f32 walk (tn_setup per job)
def grouped(name, jobs, njobs=None, **extra):
    fn = getattr(lib.load(), name)
    n = len(jobs) if njobs is None else njobs
    table = job_table(*jobs) if jobs else None
    if name == "siss_gemm_tn_grouped_capped":
        return fn(table, n, extra.get("max_blocks", 64), None)
    return fn(table, n, None)


@pytest.mark.parametrize("name", ["siss_gemm_tn_grouped", "siss_gemm_tn_grouped_capped", "siss_gemm_tn_grouped_f32"])
def test_grouped_weight_gradients_refuse(name):
    assert grouped(name, [tn_job(), tn_job(**JOB3)]) != 1
    assert grouped(name, []) == 1                                                       # jobs null
    assert grouped(name, [tn_job()], njobs=0) == 1
    assert grouped(name, [tn_job()] * 257) == 1
    rows = JOB_ROWS if name != "siss_gemm_tn_grouped_f32" else [r for r in JOB_ROWS if r[0] in ("Y null", "N 0", "row_end > rows_per_set")]
    for label, over in rows:
        jobs = [tn_job(), tn_job(**over)]                                                # the SECOND job is the broken one
        assert grouped(name, jobs[::-1] if name.endswith("_f32") else jobs) == 1, label  # (the f32 walk launches job by job)
    if name == "siss_gemm_tn_grouped_capped":
        assert grouped(name, [tn_job()], max_blocks=4) == 1
        assert grouped(name, [tn_job()], max_blocks=12) == 1


def test_paired_weight_gradients_refuse():
    fn = lib.load().siss_gemm_tn_pair
    pair = lambda a, b, maxb=256: fn(job_table(a) if a else None, job_table(b) if b else None, maxb, None)
    assert pair(tn_job(**JOB3), tn_job()) != 1
    assert pair(None, tn_job()) == 1 and pair(tn_job(**JOB3), None) == 1
    assert pair(tn_job(**JOB3), tn_job(), maxb=-1) == 1
    assert pair(tn_job(**JOB3), tn_job(), maxb=8) == 1                                   # fewer than 16 workgroups
    assert pair(tn_job(), tn_job()) == 1                                                 # job3 is not 3-tap
    assert pair(tn_job(**JOB3), tn_job(**JOB3)) == 1                                     # job1 is not one-panel
    assert pair(tn_job(**dict(JOB3, row_end=0)), tn_job()) == 1                          # no rows
    assert pair(tn_job(**dict(JOB3, shifts=[0, 2, 4])), tn_job()) == 1                   # three panels that are no filter row
    for label, over in JOB_ROWS:
        if label not in ("npanels 10", "N 0"):       # (the pair sizes its grid from the jobs' shapes before tn_setup sees them)
            assert pair(tn_job(**dict(JOB3, **over)), tn_job()) == 1, label
            assert pair(tn_job(**JOB3), tn_job(**over)) == 1, label
