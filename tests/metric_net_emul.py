"""What the two launchers of csrc/metric_conv.hip compute, by torch's f64 operations on host tensors (the arguments as lib.call gets
them), with the launchers' argument contract asserted: the one emulation the host tests of the four metric networks share.  The result
is rounded to the output buffer's dtype (f32 between layers, or f64 where a test keeps its activations in f64)."""
import torch
import torch.nn.functional as F


def call(name, *a):
    """Emulate `name` and return 0; None for a launcher that is not csrc/metric_conv.hip's (the caller's own branches take it)."""
    if name == "siss_metric_conv":
        (x, nchw, w, b, res, y, ws, ws_words, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, ph, pw, Kp, ldy, coff, relu, splits) = a
        assert tuple(x.shape) == ((N, Cin, H, W) if nchw else (N, H, W, Cin)) and x.is_contiguous()
        assert tuple(y.shape) == (N, Ho, Wo, ldy) and y.is_contiguous() and 0 <= coff and coff + Cout <= ldy
        assert (Cin <= 4 if nchw else (Cin % 32 == 0 or Cin <= 4)) and Kp % 32 == 0 and 0 <= Kp - KH * KW * Cin < 32
        assert 0 <= ph < KH and 0 <= pw < KW and H + 2 * ph >= KH and W + 2 * pw >= KW
        assert 1 <= splits <= Kp // 32 and (splits == 1 or ws_words >= splits * N * Ho * Wo * Cout)
        K = KH * KW * Cin
        assert tuple(w.shape) == (Cout, Kp) and not w[:, K:].any()
        wt = w[:, :K].reshape(Cout, KH, KW, Cin).permute(0, 3, 1, 2).double()
        o = F.conv2d((x if nchw else x.permute(0, 3, 1, 2)).double(), wt, b.double(), stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1)
        assert tuple(o.shape) == (N, Ho, Wo, Cout)
        if res is not None:
            assert tuple(res.shape) == (N, Ho, Wo, Cout) and coff == 0 and ldy == Cout
            o = o + res.double()
        y[..., coff:coff + Cout] = (F.relu(o) if relu else o).to(y.dtype)
    elif name == "siss_metric_maxpool3":
        x, y, N, H, W, C, Ho, Wo, stride, pad, ldy, coff = a
        assert tuple(x.shape) == (N, H, W, C) and tuple(y.shape) == (N, Ho, Wo, ldy) and 0 <= coff and coff + C <= ldy
        assert stride in (1, 2) and pad in (0, 1) and C % 4 == 0 and ldy % 4 == 0 and coff % 4 == 0
        o = F.max_pool2d(x.permute(0, 3, 1, 2), 3, stride, pad).permute(0, 2, 3, 1)
        assert tuple(o.shape) == (N, Ho, Wo, C)
        y[..., coff:coff + C] = o
    else:
        return None
    return 0
