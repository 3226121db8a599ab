"""Host side of the saliency mask (siss_amd/saliency.py, csrc/saliency.hip's argument checks), without a GPU:

* tests/saliency_ref.py against np.sort / plain loops on random, tied, denormal and signed-zero inputs;
* the k rule and the fraction rule; pack / unpack; save / load and the fingerprint refusals;
* deletion.saliency: absent from the four YAMLs, parsed and refused by name in check_supported, refused by the pre-training task;
* each new entry point returns status 1 for one broken argument each (the style of tests/test_refusals_host.py: made-up aligned
  pointers, so this part skips where a GPU is visible).
"""
import json
import os
import types

import numpy as np
import pytest
import torch

import saliency_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ================================================================ the reference
@pytest.mark.parametrize("kind", list(R.INPUTS))
@pytest.mark.parametrize("n", [1, 3, 4, 255, 1025, 40_003])
def test_reference_select_against_a_sort(kind, n):
    g = R.INPUTS[kind](n, n + 1)
    ks = R.keys(g)
    assert ks.dtype == np.uint32 and int(ks.max()) < 2 ** 31
    order = np.sort(ks)[::-1]
    for k in R.ranks(g, n):
        r = R.select(g, k)
        assert r["threshold_bits"] == int(order[k - 1])
        assert r["count_gt"] < k <= r["count_ge"]
        assert r["count_gt"] == int(np.searchsorted(-order.astype(np.int64), -int(order[k - 1]), side="left"))
        assert r["count_ge"] - r["count_gt"] == int((ks == order[k - 1]).sum())
        words = R.mask_words(g, r["threshold_bits"])
        assert words.dtype == np.uint32 and words.size == (n + 31) // 32
        flags = R.unpack(words, words.size * 32)
        assert int(flags.sum()) == r["count_ge"] and not flags[n:].any(), "tail bits must be zero"
        assert np.array_equal(flags[:n], ks >= order[k - 1])


def test_reference_ranks_by_bit_pattern():
    g = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -2e-38, 1.0, -1.0, np.inf, np.nan], dtype=np.float32)
    ks = R.keys(g)
    assert ks[0] == ks[1] == 0 and ks[2] == ks[3] == 1 and ks[6] == ks[7] == 0x3f800000
    assert R.select(g, 1)["nonfinite"] == 2 and R.select(g, 3)["threshold_bits"] == 0x3f800000
    assert R.select(g, 4) == dict(threshold_bits=0x3f800000, count_gt=2, count_ge=4, nonfinite=2)
    assert R.select(g, 8)["threshold_bits"] == 1 and R.select(g, 9)["threshold_bits"] == 0
    d = R.denormals(1000, 3)
    assert (np.abs(d) < 2.0 ** -125).all() and (R.keys(d) < 0x00800000).any() and (R.keys(d) >= 0x00800000).any()
    z = R.half_zeros(1000, 4)
    assert (np.signbit(z) & (z == 0)).any() and ((z == 0) & ~np.signbit(z)).any()


def test_pack_bit_order():
    flags = np.zeros(70, bool)
    flags[[0, 5, 31, 32, 69]] = True
    w = R.pack(flags)
    assert w.tolist() == [1 | 1 << 5 | 1 << 31, 1, 1 << 5]
    assert np.array_equal(R.unpack(w, 70), flags)
    from siss_amd.saliency import pack_bool, unpack_bool
    t = pack_bool(torch.from_numpy(flags))
    assert t.dtype == torch.int32 and np.array_equal(t.numpy().view(np.uint32), w)
    assert np.array_equal(unpack_bool(t, 70).numpy(), flags)
    from siss_amd.saliency import count_bits
    rng = np.random.default_rng(1)
    many = rng.random(32 * 257 + 9) < 0.37
    assert count_bits(pack_bool(torch.from_numpy(many))) == int(many.sum()) and count_bits(t) == 5
    assert count_bits(torch.full((3,), -1, dtype=torch.int32)) == 96
    # granule k's nibble, as the masked passes read it
    for k in range(17):
        assert (int(w[k >> 3]) >> ((k & 7) * 4)) & 0xf == sum(int(flags[4 * k + j]) << j for j in range(4) if 4 * k + j < 70)


# ================================================================ k, fraction, the parsed key
def test_k_and_fraction_rules():
    from siss_amd.saliency import check_fraction, mask_k
    assert mask_k(0.5, 1000) == 500 and mask_k(0.03, 1000) == 30 and mask_k(0.4999, 10) == 5 and mask_k(0.999, 3) == 3
    assert mask_k(0.25, 114_000_003) == round(0.25 * 114_000_003)
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, True, "0.5", None, float("nan")):
        with pytest.raises(ValueError, match="fraction"):
            check_fraction(bad)
    with pytest.raises(ValueError, match="no parameter"):
        mask_k(0.01, 10)


def test_parse_saliency():
    from siss_amd.saliency import parse_saliency
    assert parse_saliency(None) is None
    c = parse_saliency({})
    assert (c.fraction, c.batches, c.seed, c.path) == (0.5, 8, 0, None)
    c = parse_saliency(dict(fraction=0.25, batches=2, seed=7, path="/somewhere"))
    assert (c.fraction, c.batches, c.seed, c.path) == (0.25, 2, 7, "/somewhere")
    for bad, word in ((3, "mapping"), ([0.5], "mapping"), (dict(fractoin=0.5), "fractoin"), (dict(fraction=0), "fraction"),
                      (dict(fraction=1), "fraction"), (dict(fraction="half"), "fraction"), (dict(batches=0), "batches"),
                      (dict(batches=1.5), "batches"), (dict(seed="x"), "seed"), (dict(path=3), "path")):
        with pytest.raises(ValueError, match="deletion.saliency") as e:
            parse_saliency(bad)
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="deletion.trainable"):
        parse_saliency({}, trainable=["attn"])
    with pytest.raises(ValueError, match="deletion.lora"):
        parse_saliency({}, lora=dict(rank=4))


@pytest.mark.parametrize("config", ["delete_celeb", "delete_tshirt", "delete_sd"])
def test_tasks_read_the_key_and_refuse_it_in_check_supported(config):
    from siss_amd import hydra_lite as H

    def task(ov):
        cfg = H.compose(config, os.path.join(ROOT, "config"), ov)
        return H.instantiate(cfg.task, cfg=cfg, _recursive_=False)
    assert task([]).saliency_config() is None and task(["+deletion.saliency=null"]).saliency_config() is None
    task([]).check_supported()
    t = task(["+deletion.saliency={fraction:0.25,batches:2,seed:3}"])
    c = t.saliency_config()
    assert (c.fraction, c.batches, c.seed, c.path) == (0.25, 2, 3, None)
    t.check_supported()
    for ov, word in (("0.5", "mapping"), ("{fraction:0.5,rank:4}", "rank"), ("{fraction:0}", "fraction"), ("{fraction:1.0}", "fraction"),
                     ("{fraction:1.5}", "fraction"), ("{batches:0}", "batches")):
        with pytest.raises(ValueError, match="deletion.saliency") as e:
            task(["+deletion.saliency=" + ov]).check_supported()
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="deletion.trainable"):
        task(["+deletion.saliency={fraction:0.5}", "+deletion.trainable=[attn]"]).check_supported()
    with pytest.raises(ValueError, match="deletion.lora"):
        task(["+deletion.saliency={fraction:0.5}", "+deletion.lora={rank:4,targets:[attn]}"]).check_supported()


def test_the_yamls_lack_the_key_and_the_pretraining_task_refuses_it():
    from siss_amd import hydra_lite as H
    for config in ("delete_celeb", "delete_tshirt", "delete_sd", "train_tshirt_mnist"):
        assert "saliency" not in open(os.path.join(ROOT, "config", config + ".yaml")).read()
        assert "saliency" not in (H.compose(config, os.path.join(ROOT, "config"), []).get("deletion") or {})
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), ["+deletion.saliency={fraction:0.5}"])
    with pytest.raises(NotImplementedError, match="deletion.saliency"):
        H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()
    cfg = H.compose("train_tshirt_mnist", os.path.join(ROOT, "config"), [])
    H.instantiate(cfg.task, cfg=cfg, _recursive_=False).check_supported()


# ================================================================ the mask object: files and fingerprint
def fake_engine(numels=(70, 64, 5), align=64):
    specs, off = {}, 0
    for i, n in enumerate(numels):
        specs[f"w{i}"] = types.SimpleNamespace(name=f"w{i}", off=off, numel=n)
        off += -(-n // align) * align
    return types.SimpleNamespace(ps=types.SimpleNamespace(specs=specs, total=off), device=torch.device("cpu"))


def test_from_bool_ones_and_the_file_round_trip(tmp_path):
    from siss_amd.saliency import CONFIG_FILE, MASK_FILE, SaliencyMask
    eng = fake_engine()
    total = eng.ps.total
    assert total == 128 + 64 + 64
    rng = np.random.default_rng(0)
    flags = rng.random(total) < 0.5
    m = SaliencyMask.from_bool(eng, torch.from_numpy(flags))
    real = np.zeros(total, bool)
    for sp in eng.ps.specs.values():
        real[sp.off:sp.off + sp.numel] = True
    assert m.count == int((flags & real).sum()) and m.params == 139 and m.tensors == 3 and m.total == total
    assert np.array_equal(m.bits.numpy().view(np.uint32), R.pack(flags)) and np.array_equal(m.to_bool().numpy(), flags)
    ones = SaliencyMask.ones(eng)
    assert ones.count == 139 and bool(ones.to_bool().all()) and ones.bits.numel() == total // 32
    with pytest.raises(ValueError, match="flags"):
        SaliencyMask.from_bool(eng, torch.zeros(total - 1, dtype=torch.bool))
    m.k, m.threshold, m.fraction, m.batches, m.seed = 70, 0.125, 0.5, 2, 9
    m.save(str(tmp_path / "mask"))
    assert sorted(os.listdir(tmp_path / "mask")) == sorted([MASK_FILE, CONFIG_FILE]) and SaliencyMask.present(str(tmp_path / "mask"))
    assert not SaliencyMask.present(str(tmp_path)) and not SaliencyMask.present(None)
    c = json.load(open(tmp_path / "mask" / CONFIG_FILE))
    assert c == dict(fraction=0.5, k=70, count=m.count, threshold=0.125, batches=2, seed=9, total=total, tensors=3, real_params=139)
    back = SaliencyMask.load(str(tmp_path / "mask"), eng)
    assert torch.equal(back.bits, m.bits) and back.config() == m.config()
    assert back.log_fields() == dict(saliency_params=m.count, saliency_fraction=m.count / 139, saliency_threshold=0.125)
    for other, word in ((fake_engine((70, 64, 5, 1)), "total"), (fake_engine((70, 64, 4)), "real_params"), (fake_engine((70, 69)), "tensors")):
        with pytest.raises(ValueError, match=word):
            SaliencyMask.load(str(tmp_path / "mask"), other)


# ================================================================ argument checks of the four entry points
def P(k):
    """Fake device pointer number k (16-byte aligned, 1 MiB apart)."""
    return 0x1000000 + (k << 20)


SEL = dict(g=P(1), n=1000, k=500, work=P(2), result=P(3))
MSK = dict(g=P(1), n=1000, threshold_bits=0x3f800000, bits=P(2))
NRM = dict(gx=P(1), ga=P(2), n=1000, bits=P(3), mode=0, knob=5.0, max_norm=1.0, beta1=0.9, beta2=0.999, partials=P(4), scalars=P(5))
UPD = dict(gx=P(1), ga=P(2), p=P(3), m=P(4), v=P(5), shadow=P(6), g_out=P(7), n=1000, bits=P(8), lr=1e-4, beta1=0.9, beta2=0.999,
           eps=1e-8, wd=1e-2, scalars=P(9))
TABLE = {
    "siss_absf_select": (SEL, [("g null", dict(g=None)), ("work null", dict(work=None)), ("result null", dict(result=None)),
                               ("g align", dict(g=P(1) + 8)), ("work align", dict(work=P(2) + 4)), ("result align", dict(result=P(3) + 4)),
                               ("n 0", dict(n=0)), ("k 0", dict(k=0)), ("k > n", dict(k=1001)), ("k < 0", dict(k=-1))]),
    "siss_saliency_mask": (MSK, [("g null", dict(g=None)), ("bits null", dict(bits=None)), ("g align", dict(g=P(1) + 8)),
                                 ("bits align", dict(bits=P(2) + 2)), ("n 0", dict(n=0)), ("threshold < 0", dict(threshold_bits=-1))]),
    "siss_grad_norms_scale_masked": (NRM, [("gx null", dict(gx=None)), ("ga null", dict(ga=None)), ("bits null", dict(bits=None)),
                                           ("partials null", dict(partials=None)), ("scalars null", dict(scalars=None)),
                                           ("gx align", dict(gx=P(1) + 8)), ("bits align", dict(bits=P(3) + 4)), ("n 0", dict(n=0)),
                                           ("mode 3", dict(mode=3)), ("mode -1", dict(mode=-1))]),
    "siss_recombine_clip_adamw_masked": (UPD, [("gx null", dict(gx=None)), ("p null", dict(p=None)), ("m null", dict(m=None)),
                                               ("v null", dict(v=None)), ("bits null", dict(bits=None)), ("scalars null", dict(scalars=None)),
                                               ("p align", dict(p=P(3) + 8)), ("bits align", dict(bits=P(8) + 4)),
                                               ("shadow align", dict(shadow=P(6) + 4)), ("g_out align", dict(g_out=P(7) + 8)),
                                               ("n 0", dict(n=0))]),
}
ROWS = [(name, label, over) for name, (_, rows) in TABLE.items() for label, over in rows]
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device pointers: host-only test")


def invoke(name, kw):
    from siss_amd import lib
    assert set(kw) <= set(lib.PARAMS[name]), (name, set(kw) - set(lib.PARAMS[name]))
    return getattr(lib.load(), name)(*[kw.get(pname) for pname in lib.PARAMS[name]])


def test_the_entry_points_are_declared_and_sized():
    from siss_amd import lib
    from siss_amd.saliency import ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert lib.has(name) and lib.PARAMS[name][-1] == "stream" and name in lib.F32_SAME, name
    assert lib.query("siss_absf_select_work_bytes") == 2048 * 256 * 4 and lib.query("siss_absf_select_result_words") == 8
    # the whole-buffer pair's argument lists plus `bits` after n
    for masked, whole in (("siss_grad_norms_scale_masked", "siss_grad_norms_scale"), ("siss_recombine_clip_adamw_masked", "siss_recombine_clip_adamw")):
        assert tuple(p for p in lib.PARAMS[masked] if p != "bits") == lib.PARAMS[whole]
        assert lib.PARAMS[masked][lib.PARAMS[masked].index("n") + 1] == "bits"


@host_only
@pytest.mark.parametrize("name", sorted(TABLE))
def test_base_arguments_pass_every_check(name):
    assert invoke(name, TABLE[name][0]) != 1


@host_only
@pytest.mark.parametrize("name,label,over", ROWS, ids=[f"{n}-{l}" for n, l, _ in ROWS])
def test_one_broken_argument_is_refused(name, label, over):
    assert invoke(name, dict(TABLE[name][0], **over)) == 1
