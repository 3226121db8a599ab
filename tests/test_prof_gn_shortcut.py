"""siss_amd/prof.py's rule for siss_groupnorm_bwd_sc against figures worked by hand for the top-resolution site of the benchmark's
CelebA-HQ 256 B = 16 step (nx = 16 saved samples, n2 = 32 cotangent samples, 256 x 256 pixels, 256 -> 128 channels, split target)."""


def test_fused_shortcut_launcher_is_booked_with_its_product_and_its_bytes():
    from siss_amd import lib, prof
    names = lib.PARAMS["siss_groupnorm_bwd_sc"][:-1]
    a = dict.fromkeys(names, 0)
    a.update(dy=object(), x=object(), dx=object(), dout=object(), wsc=object(), dx2=object(), accum2=None, accumulate2=0, K=128,
             n2=32, nx=16, H=256, W=256, C=256, G=32, split_c=128)
    base, work, key, symbol, nbytes = prof.account("siss_groupnorm_bwd_sc", a)
    assert (base, symbol) == ("siss_groupnorm_bwd_sc", "gn_bwd_sc_kernel")
    assert key == ("n2", 32, "H", 256, "C", 256, "K", 128)
    px = 256 * 256
    assert work == 2.0 * 32 * px * 256 * 128                                 # 2 M N K over the true pixels
    # read x (16 samples x 256 channels), dy (32 x 256) and dout (32 x 128), write dx (32 x 256): bf16
    assert nbytes == 2.0 * px * (16 * 256 + 32 * 256 + 32 * 128 + 32 * 256) and type(nbytes) is float and type(work) is float
    # a running cotangent and an accumulated second part are one more read each
    a.update(accum2=object(), accumulate2=1)
    assert prof.account("siss_groupnorm_bwd_sc", a)[4] == nbytes + 2.0 * px * 256 * 32 * 2
    assert "siss_groupnorm_bwd_sc" not in prof._RULES and lib.KERNEL_IDS["gn_bwd_sc_kernel"] == 16
